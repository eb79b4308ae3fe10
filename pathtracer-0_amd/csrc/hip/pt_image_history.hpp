// pt_image_history.hpp — what the current image is a picture of: the camera record of every ring image, the generations of the scene, the validity
// of the mark (include/pt_motion.h) and of the hold (include/pt_validate.h), the keys of the four feature-record caches, and whose frame constants
// are on the device.  Plain C++: no HIP runtime call and no context.  pt_context.hpp, pt_stream_dev.hpp, pt_hip.hip and pt_image.hpp keep the device buffers these words describe and
// ask every question here; tests/c/image_history_check.cpp asks the same questions from scripts of calls, so every call order can be run on a CPU.
//
// THE RULES:
//   sceneGen   rises with every accepted upload of a scene buffer and with every texture; otherGen with those of them that are not geometry
//              (bindings 5 and 14, textures); camWrites with every write of a camera record, valid or not.  Nothing else moves a counter.
//   a camera   record is usable while sceneGen is the one it was written under, it was not rendered with DEBUG, and its Parameters give the image size
//   the mark   serves one pt_reproject_frame_moved, on the image it was taken on, while camWrites and otherGen are what they were
//   the hold   serves one pt_history_merge, on the image it was taken on, while that image's camera has the held frame inputs and sceneGen is what it was
//   a cache    serves while it is valid and is asked for the frame inputs (and, for the seen-through records, the rule) it was filled under; every
//              upload, accepted or not, and every texture invalidate all four
//   the frame  constants on the device are the running stream's from the moment it starts until a call of its own overwrites them
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include "../../../include/pt_through.h"

// images of the ring (the test builds the history once with another value)
#ifndef PT_HISTORY_IMAGES
#define PT_HISTORY_IMAGES 4
#endif

namespace ptp {

// the frame inputs: Parameters (binding 4), ORIGIN, ROTATION, MOUSE_POS (bindings 0, 1, 2) as k_frame_setup reads them
struct FrameIn { float params[12]; float origin[3]; float rotation[3]; float mouse[3]; };
static_assert(sizeof(FrameIn) == 84, "FrameIn is copied to the device and compared bytewise: 21 floats, no padding");

// of each kind of record one cache under the current inputs and one under the current image's camera (Rh; Sh, Yh)
enum RecordCache { RC_FEAT, RC_FEAT_H, RC_THRU, RC_THRU_H, RC_COUNT };

struct Refused { int code = 0; std::string msg; };      // code 0: not refused

// pt_reproject_frame*: refused; or nothing to map from (PT_OK); or whether the image's camera has the current inputs, and so which caches hold Rh and Sh / Yh
struct ReprojectPlan { Refused refused; bool nothing = false, sameCam = false; RecordCache rh = RC_FEAT, sh = RC_THRU; };

// every refusal and outcome below, one bit each (tests/test_image_history.py requires every one of them of its scripts)
enum HistoryBranch {
    HB_IN_UNSET, HB_IN_SIZE, HB_IN_DEBUG, HB_CAM_SCENE, HB_CAM_DEBUG, HB_CAM_SIZE, HB_MARK_NO_CAMERA, HB_MOVED_NO_MARK, HB_MOVED_OTHER_IMAGE,
    HB_MOVED_CAMERA, HB_MOVED_UPLOAD, HB_HOLD_NO_CAMERA, HB_MERGE_NO_HOLD, HB_MERGE_OTHER_IMAGE, HB_MERGE_NO_CAMERA, HB_MERGE_INPUTS, HB_MERGE_SCENE,
    HB_REPROJECT_NOTHING, HB_REPROJECT_SAME, HB_REPROJECT_OTHER, HB_CACHE_HIT, HB_CACHE_MISS, HB_CACHE_FILLED, HB_CACHE_INVALIDATED, HB_COUNT
};

class ImageHistory {
public:
    static constexpr int IMAGES = PT_HISTORY_IMAGES;
    struct Camera { FrameIn in{}; uint64_t sceneGen = 0; bool valid = false; };      // the frame inputs an image was rendered or written with, sceneGen then

    void create(int w, int h) { W = w; H = h; }
    int image() const { return cur; }
    int imageOfAge(int age) const { return (cur + IMAGES - age) % IMAGES; }
    const Camera& camera() const { return cam[cur]; }
    uint64_t sceneUploads() const { return sceneGen; }
    uint64_t otherUploads() const { return otherGen; }
    uint64_t cameraWrites() const { return camWrites; }
    bool markValid() const { return mark.valid; }
    bool holdValid() const { return hold.valid; }
    bool cacheValid(RecordCache k) const { return cache[k].valid; }
    uint64_t reached() const { return branches; }

    // ---- uploads.  pt_set_buffer: any upload may move the camera or the scene under the feature records, and they go before the binding is looked
    // at, so a refused upload drops them too; an accepted scene buffer (not ORIGIN, ROTATION, MOUSE_POS, Parameters) then counts
    void uploadBegins() { invalidateCaches(); }
    void sceneBufferAccepted(int binding) {
        sceneGen++;
        if (binding == PT_BIND_IMPLICITS || binding == PT_BIND_MATERIALS) otherGen++;      // not geometry (include/pt_motion.h)
    }
    void textureUploaded() { invalidateCaches(); sceneGen++; otherGen++; }

    // ---- camera writes of the current image: each counts
    void rendered(const FrameIn& in) { cam[cur] = Camera{in, sceneGen, true}; camWrites++; }      // a stream's batch, the DEBUG render
    // pt_write_frame, a stored reprojection or merge: the inputs current at the call (null: not set, and the record is no camera)
    void written(const FrameIn* in) {
        if (in) cam[cur].in = *in;
        cam[cur].valid = in != nullptr; cam[cur].sceneGen = sceneGen; camWrites++;
    }
    void reset() { cam[cur].valid = false; camWrites++; }
    int nextImage() const { return (cur + 1) % IMAGES; }
    void turnImage() { cur = nextImage(); cam[cur].valid = false; camWrites++; }      // pt_next_image

    // ---- whose the frame constants on the device are: the stream started with streamInputs(), or (a byte pattern no accepted Parameters have) nobody's
    void streamStarted(const FrameIn& in) { streamIn = in; }
    void frameConstantsTaken() { std::memset(&streamIn, 0xff, sizeof(FrameIn)); }
    bool streamHas(const FrameIn& in) const { return std::memcmp(&in, &streamIn, sizeof(FrameIn)) == 0; }
    const FrameIn& streamInputs() const { return streamIn; }

    // ---- the record caches: asked (hit: nothing to do), then beginFill (invalid from here: a failed fill leaves it so), then filled
    bool cached(RecordCache k, const FrameIn& in, const pt_through_rule* rule) {
        const Key& R = cache[k];
        const bool hit = R.valid && std::memcmp(&R.in, &in, sizeof(FrameIn)) == 0 && (!rule || std::memcmp(&R.rule, rule, sizeof(*rule)) == 0);
        note(hit ? HB_CACHE_HIT : HB_CACHE_MISS);
        return hit;
    }
    void beginFill(RecordCache k) { cache[k].valid = false; }
    void filled(RecordCache k, const FrameIn& in, const pt_through_rule* rule) {
        Key& R = cache[k];
        if (rule) R.rule = *rule;
        R.in = in; R.valid = true;
        note(HB_CACHE_FILLED);
    }

    // ---- the current inputs (null: Parameters, ORIGIN or ROTATION not set), refused unless they render surfaces at the image's size; toDo: what
    // the caller wants surfaces for
    Refused usableInputs(const FrameIn* in, const std::string& w, const char* toDo) {
        if (!in) return refuse(HB_IN_UNSET, PT_ERR_ARG, "Parameters / ORIGIN / ROTATION (bindings 4, 0, 1) not set");
        const float* P = in->params;
        if ((int)P[2] != W || (int)(P[2] * P[3]) != H)
            return refuse(HB_IN_SIZE, PT_ERR_ARG, "Parameters.resolution / screenHratio do not match the FRAME image size given to pt_create");
        if (P[10] != 0.0f) return refuse(HB_IN_DEBUG, PT_ERR_UNSUPPORTED, w + ": DEBUG != 0 renders the traversal heat map, which has no surfaces to " + toDo);
        return {};
    }
    // the current image's (valid) camera record, refused unless feature records under it describe the image: the scene as it was, surfaces, the size
    Refused usableCamera(const std::string& w) {
        const Camera& h = cam[cur];
        if (h.sceneGen != sceneGen) return refuse(HB_CAM_SCENE, PT_ERR_ARG, w + ": a scene buffer or texture was uploaded since the image's camera was recorded");
        if (h.in.params[10] != 0.0f) return refuse(HB_CAM_DEBUG, PT_ERR_UNSUPPORTED, w + ": the image was rendered with DEBUG != 0");
        if ((int)h.in.params[2] != W || (int)(h.in.params[2] * h.in.params[3]) != H)
            return refuse(HB_CAM_SIZE, PT_ERR_ARG, w + ": the image's camera has Parameters that do not match the image size");
        return {};
    }

    // ---- the mark.  takeMark: refused, or the old mark is gone from here and markTaken makes the new one
    Refused takeMark() {
        if (!cam[cur].valid) return refuse(HB_MARK_NO_CAMERA, PT_ERR_ARG, "pt_motion_mark: the current image has no camera (render or pt_write_frame first)");
        const Refused r = usableCamera("pt_motion_mark");
        if (!r.code) mark.valid = false;
        return r;
    }
    void markTaken() { mark.image = cur; mark.camWrites = camWrites; mark.otherGen = otherGen; mark.valid = true; }
    void markSpent() { mark.valid = false; }

    // ---- the hold.  takeHold: refused or not; the old hold is gone from holdBegins (after the caller has its buffers), holdTaken makes the new one
    Refused takeHold() {
        if (!cam[cur].valid) return refuse(HB_HOLD_NO_CAMERA, PT_ERR_ARG, "pt_history_hold: the current image has no camera (render or pt_write_frame first)");
        return {};
    }
    void holdBegins() { hold.valid = false; }
    void holdTaken() { hold.image = cur; hold.in = cam[cur].in; hold.sceneGen = sceneGen; hold.valid = true; }
    void holdSpent() { hold.valid = false; }
    Refused mergeHold() {
        if (!hold.valid) return refuse(HB_MERGE_NO_HOLD, PT_ERR_ARG, "pt_history_merge: no hold (pt_history_hold first; a hold serves one merge)");
        if (hold.image != cur) return refuse(HB_MERGE_OTHER_IMAGE, PT_ERR_ARG, "pt_history_merge: the hold belongs to another image");
        const Camera& h = cam[cur];
        if (!h.valid) return refuse(HB_MERGE_NO_CAMERA, PT_ERR_ARG, "pt_history_merge: the image has no camera (pt_reset_frame since the hold)");
        if (std::memcmp(&h.in, &hold.in, sizeof(FrameIn)) != 0)
            return refuse(HB_MERGE_INPUTS, PT_ERR_ARG,
                          "pt_history_merge: the image's camera no longer has the held frame inputs (a render or pt_write_frame under other inputs)");
        if (hold.sceneGen != sceneGen) return refuse(HB_MERGE_SCENE, PT_ERR_ARG, "pt_history_merge: a scene buffer or texture was uploaded since the hold");
        return {};
    }

    // ---- a reprojection of the current image to the (usable) inputs `now`.  moved: include/pt_motion.h's call, Rh from the mark; else Rh from the
    // image's camera, the same records as Rn when it is unchanged (and then one pair of seen-through records serves both sides as well)
    ReprojectPlan planReproject(const FrameIn& now, bool moved, const std::string& w) {
        ReprojectPlan p;
        const Camera& h = cam[cur];
        if (moved) {
            if (!mark.valid) p.refused = refuse(HB_MOVED_NO_MARK, PT_ERR_ARG, w + ": no mark (pt_motion_mark first; a mark serves one call)");
            else if (mark.image != cur) p.refused = refuse(HB_MOVED_OTHER_IMAGE, PT_ERR_ARG, w + ": the mark belongs to another image");
            else if (!h.valid || mark.camWrites != camWrites)
                p.refused = refuse(HB_MOVED_CAMERA, PT_ERR_ARG,
                                   w + ": the image's camera is no longer the marked one (a render, pt_write_frame, pt_reset_frame or pt_next_image since the mark)");
            else if (mark.otherGen != otherGen) p.refused = refuse(HB_MOVED_UPLOAD, PT_ERR_ARG, w + ": binding 5, binding 14 or a texture was uploaded since the mark");
        } else if (!h.valid) {
            p.nothing = true;                                     // no camera: nothing to map from
            note(HB_REPROJECT_NOTHING);
        } else {
            p.refused = usableCamera(w);
        }
        if (p.refused.code || p.nothing) return p;
        p.sameCam = std::memcmp(&h.in, &now, sizeof(FrameIn)) == 0;
        note(p.sameCam ? HB_REPROJECT_SAME : HB_REPROJECT_OTHER);
        p.rh = p.sameCam ? RC_FEAT : RC_FEAT_H; p.sh = p.sameCam ? RC_THRU : RC_THRU_H;
        return p;
    }

private:
    struct Key { bool valid = false; FrameIn in{}; pt_through_rule rule{}; };
    int W = 0, H = 0, cur = 0;
    Camera cam[IMAGES];
    uint64_t sceneGen = 0, otherGen = 0, camWrites = 0;
    struct { bool valid = false; int image = 0; uint64_t camWrites = 0, otherGen = 0; } mark;
    struct { bool valid = false; int image = 0; FrameIn in{}; uint64_t sceneGen = 0; } hold;
    Key cache[RC_COUNT];
    FrameIn streamIn{};             // frame inputs the running stream was started with
    uint64_t branches = 0;          // HistoryBranch bits

    void note(HistoryBranch b) { branches |= 1ull << b; }
    Refused refuse(HistoryBranch b, int code, const std::string& msg) { note(b); return Refused{code, msg}; }
    void invalidateCaches() {
        for (Key& k : cache) { if (k.valid) note(HB_CACHE_INVALIDATED); k.valid = false; }
    }
};

}  // namespace ptp
