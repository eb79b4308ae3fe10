// pt_group_plan.hpp — the host-only layout arithmetic of a group of streams (pt_multi.hpp): which pixels a tile shard owns and in which slots,
// the shape pt_create_multi_part gives a group (every refusal with its text, the runs of streams per device, the transport), and the gather of one
// image as plain data — staging sizes, copies, event edges and the arguments of the collective, naming shards, runs and offsets, never pointers.
// Plain C++: no HIP runtime call and no context.  initContext, pt_shard_slots, pt_shard_map, pt_unshard and pt_create_multi_part (pt_hip.hip) ask
// here, multiGather (pt_multi.hpp) walks the plan and issues the calls; tests/c/group_plan_check.cpp executes the same plan on host arrays.
#pragma once
#include "../../../include/pt_api.h"
#include "pt_image_history.hpp"      // ptp::Refused

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ptp {

// ---- tile sharding: the image in tiles, dealt round-robin to the shards
constexpr int SHARD_TILE_W = 32, SHARD_TILE_H = 8;      // TILE_W, TILE_H of pt_kernels.hpp
constexpr int SHARD_BLOCK = 256;                        // what a shard's slot count is rounded to (BLOCK of pt_kernels.hpp)

// tile-major enumeration of the pixels owned by `rank`: the order a context renders them in
inline void shardPixels(int W, int H, int rank, int count, std::vector<int32_t>& out) {
    out.clear();
    const int ntx = (W + SHARD_TILE_W - 1) / SHARD_TILE_W, nty = (H + SHARD_TILE_H - 1) / SHARD_TILE_H;
    for (int t = rank; t < ntx * nty; t += count) {
        const int tx = t % ntx, ty = t / ntx;
        for (int y = ty * SHARD_TILE_H; y < std::min(H, (ty + 1) * SHARD_TILE_H); y++)
            for (int x = tx * SHARD_TILE_W; x < std::min(W, (tx + 1) * SHARD_TILE_W); x++) out.push_back(y * W + x);
    }
}
// the accumulator slots of every one of `count` shards: the largest shard's pixels rounded up to whole blocks.  ONE shard is the image itself: its
// slot of a pixel is the pixel
inline size_t shardSlots(int W, int H, int count) {
    if (count == 1) return (size_t)W * H;
    size_t mx = 0; std::vector<int32_t> tmp;
    for (int r = 0; r < count; r++) { shardPixels(W, H, r, count, tmp); mx = std::max(mx, tmp.size()); }
    return (mx + SHARD_BLOCK - 1) / SHARD_BLOCK * SHARD_BLOCK;
}
// slot -> global pixel of one shard into out[0 .. nSlots): its pixels in tile-major order (one shard: the identity), then -1 = padding
inline Refused shardMap(int W, int H, int rank, int count, int32_t* out, size_t nSlots) {
    if (count == 1) { for (size_t i = 0; i < nSlots; i++) out[i] = i < (size_t)W * H ? (int32_t)i : -1; return {}; }
    std::vector<int32_t> px;
    shardPixels(W, H, rank, count, px);
    if (px.size() > nSlots) return Refused{PT_ERR_ARG, "pt_shard_map: n_slots too small"};
    for (size_t i = 0; i < nSlots; i++) out[i] = i < px.size() ? px[i] : -1;
    return {};
}
// ... of shards first .. first+count-1 of `total` into maps: nSlots per shard, shard-major
inline Refused shardMaps(int W, int H, int first, int count, int total, size_t nSlots, std::vector<int32_t>& maps) {
    maps.resize((size_t)count * nSlots);
    for (int r = 0; r < count; r++) { const Refused no = shardMap(W, H, first + r, total, maps.data() + (size_t)r * nSlots, nSlots); if (no.code) return no; }
    return {};
}

// ---- the shape of a group: what pt_create_multi_part decides from its arguments, the device count and the environment
struct GroupRun { int device, first, count; };          // the streams of one device: first .. first+count-1
struct GroupEnv {
    int virtualDevices = 0;          // PT_MULTI_VIRTUAL_DEVICES as a number (0: not set)
    bool forceRccl = false;          // PT_MULTI_FORCE_RCCL begins with '1'
    bool hwQueuesSet = false;        // GPU_MAX_HW_QUEUES is in the environment
};
struct GroupShape {
    std::vector<GroupRun> runs;
    bool useRccl = false;            // more than one run (or forced): the blocks of the runs travel in one collective
    bool virtualDevices = false;     // test mode: the runs share one GPU, the transport between them is device copies
    std::vector<int> streamsOnDevice;      // per stream: the group's streams on its GPU
    bool warnHwQueues = false;       // several streams share a GPU and nothing says they get hardware queues of their own
};

// the argument check of pt_create_multi_part, which comes before the question for a HIP device
inline Refused checkGroupArgs(bool out, const int* devices, int n, int W, int H, int first, int total) {
    if (!out || !devices || n < 1 || n > 64 || W < 1 || H < 1 || first < 0 || total < n || first + n > total) return Refused{PT_ERR_ARG, "pt_create_multi: bad argument"};
    return {};
}
// ... and everything after it.  nDev: the HIP devices there are (>= 1)
inline Refused planGroup(const int* devices, int n, int nDev, const GroupEnv& env, GroupShape& g) {
    g = GroupShape{};
    for (int i = 0; i < n; i++) if (devices[i] < 0 || devices[i] >= nDev) return Refused{PT_ERR_NO_DEVICE, "pt_create_multi: HIP device index out of range"};
    // the streams of one device are adjacent entries, every device carries the same number of them
    for (int i = 0; i < n; i++) {
        if (!g.runs.empty() && g.runs.back().device == devices[i]) { g.runs.back().count++; continue; }
        for (const GroupRun& r : g.runs)
            if (r.device == devices[i]) return Refused{PT_ERR_ARG, "pt_create_multi: the entries of one device must be adjacent ({0,0,1,1}, not {0,1,0,1})"};
        g.runs.push_back(GroupRun{devices[i], i, 1});
    }
    for (const GroupRun& r : g.runs) if (r.count != g.runs[0].count) return Refused{PT_ERR_ARG, "pt_create_multi: every device must be listed the same number of times"};
    // Test mode (tests/test_gpu_multi.py): PT_MULTI_VIRTUAL_DEVICES=k splits the streams of ONE device into k "virtual devices", so that a
    // one-GPU box runs the several-device code of the gather — a staging block per device, root and non-root arguments, block offsets,
    // the un-tiling of a gathered buffer — with the RCCL calls replaced by device copies to the offsets ncclGather writes (pt_multi.hpp).
    const int k = env.virtualDevices;
    if (k > 1) {
        if (g.runs.size() != 1 || n % k) return Refused{PT_ERR_ARG, "PT_MULTI_VIRTUAL_DEVICES=k needs ONE device listed a multiple of k times"};
        const int per = n / k, dev = g.runs[0].device;
        g.runs.clear();
        for (int v = 0; v < k; v++) g.runs.push_back(GroupRun{dev, v * per, per});
        g.virtualDevices = true;
    }
    g.useRccl = g.runs.size() > 1 || env.forceRccl;
    for (const GroupRun& r : g.runs) g.streamsOnDevice.insert(g.streamsOnDevice.end(), (size_t)r.count, g.virtualDevices ? n : r.count);
    g.warnHwQueues = n > (int)g.runs.size() && !env.hwQueuesSet;
    return {};
}

// ---- the gather of one image.  Every stream has completed its shard's image; ev[i] below is stream i's event
struct GatherCopy {                  // shard's image -> slot dstSlot of its run's staging block (toStaging) or of the gathered buffer, on stream `lead`
    int run, shard, lead; bool toStaging; size_t dstSlot;
    int waitFor;                     // -1, or the shard itself: its stream records ev[shard] and `lead` waits for it before the copy
};
struct GatherRelease { int run, lead, firstWaiter, waiters; };      // after the run's copies `lead` records ev[lead]; streams firstWaiter .. +waiters-1 wait for it
struct GatherSend {                  // rank `run` of the collective (root: rank 0), on stream `shard`'s
    int run, shard; bool fromImage;  // the send buffer: shard's own image, or the run's staging block
    size_t floats;                   // the element count of every rank
    bool recvIsGathered;             // the receive buffer: the gathered buffer (root), or the send buffer itself, which is never written
    size_t rootOffset;               // where this block lands in the root's receive buffer, in floats: run * floats
    bool rootWaits;                  // transport by device copies: the root's stream waits for ev[shard], recorded behind the copy
};
struct GatherPlan {
    std::vector<size_t> stagingBytes;      // per run; 0: the run has no staging block
    std::vector<GatherCopy> copies;        // in order, the copies of a run together; a run's release follows its copies
    std::vector<GatherRelease> releases;   // in run order
    std::vector<GatherSend> sends;         // in run order (empty without the collective)
    size_t totalSlots = 0;                 // the gathered buffer: n blocks of nSlots, shard-major
    bool untile = false;                   // the group holds the whole image: k_unshard writes it; else the packed block is handed out
};

inline GatherPlan planGather(const std::vector<GroupRun>& runs, int n, int shardTotal, size_t nSlots, bool useRccl, bool virtualDevices) {
    GatherPlan p;
    p.totalSlots = nSlots * (size_t)n;
    p.untile = shardTotal == n;
    p.stagingBytes.assign(runs.size(), 0);
    for (size_t r = 0; r < runs.size(); r++) {
        const GroupRun& run = runs[r];
        // 1. per device: its streams' accumulators side by side, on the device's first stream (one stream: nothing to copy).  Without the
        //    collective (one device) the block IS the gathered buffer.
        if (!(run.count == 1 && useRccl)) {
            if (useRccl) p.stagingBytes[r] = (size_t)run.count * nSlots * 16;
            for (int j = 0; j < run.count; j++)
                p.copies.push_back(GatherCopy{(int)r, run.first + j, run.first, useRccl, (useRccl ? 0 : (size_t)run.first * nSlots) + (size_t)j * nSlots, j > 0 ? run.first + j : -1});
            // the other streams must not rotate their image rings past this image before the copies have read it
            if (run.count > 1) p.releases.push_back(GatherRelease{(int)r, run.first, run.first + 1, run.count - 1});
        }
        // 2. across devices: ONE gather, a block per device, root = run 0
        if (useRccl) {
            const size_t floats = (size_t)run.count * nSlots * 4;
            p.sends.push_back(GatherSend{(int)r, run.first, run.count == 1, floats, r == 0, r * floats, virtualDevices && r > 0});
        }
    }
    return p;
}

}  // namespace ptp
