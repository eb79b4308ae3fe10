/* include/pt_rig_mix.h — layered clip blending with joint masks on the device: several keyed clips of one rig mixed into one set of locals where
 * the rig's records are made (libpt_hip.so).
 *
 * No reference counterpart.  A rig of include/pt_rig.h plays one clip; a character plays several at once: a cross-fade from walk to run, a wave
 * on the arm only, a lean on top of whatever is playing, a clip that loops.  With include/pt_rig.h alone each of those sends the caller back to
 * the host: sample the clips there, blend 12 floats per joint, upload the locals on every step.  A MIX keeps the clips where the rig's one clip
 * lies, so a step uploads a handful of floats.
 *
 * OBJECTS.  A rig gains
 *   PT_RIG_MIX_SLOTS (16) CLIP SLOTS.  A slot holds n_keys >= 1 strictly increasing finite times and n_keys * n_parts locals, key-major, exactly
 *     as in pt_rig_clip_attach; it is copied to the device at the attach (pt_rig_mix_clip).  A second attach to a slot replaces the first, and the
 *     rig changes only once the new allocation stands.  The slots are independent of pt_rig_clip_attach's single clip, which stays as it is.
 *   PT_RIG_MIX_MASKS (8) MASK SLOTS.  A mask holds one float per joint, finite and in [0, 1], on the device (pt_rig_mix_mask).
 * A LAYER (pt_rig_layer, 24 bytes) names a clip slot, a mask slot (-1: none), a mode (PT_RIG_MIX_OVERRIDE or PT_RIG_MIX_ADDITIVE), a wrap
 * (PT_RIG_MIX_CLAMP or PT_RIG_MIX_LOOP), a time t and a weight in [0, 1].  A call takes 1 to PT_RIG_MIX_MAX_LAYERS (8) layers and applies them in
 * the given order.  Layers may share a slot.
 *
 * THE RULE.  Binary32 throughout, every product rounded before every sum, in the written order, nothing fused; sqrt and / correctly rounded, as in
 * include/pt_rig.h, whose LOCAL (12 floats: t.x t.y t.z pad | q.x q.y q.z q.w | s.x s.y s.z pad) and whose steps 1-5 are meant below.
 *
 * 1. The time of a layer (host).  With CLAMP, t is taken as it is; step 5 of include/pt_rig.h clamps it to the clip.  With LOOP and n_keys > 1:
 *      D = T_last - T_0,   r = fmodf(t - T_0, D)  (the difference rounded once; fmodf is exact),   if r < 0 then r = r + D,   t' = T_0 + r
 *    and t' is taken.  The interval and u of that time are step 5's; with one key, key 0 is taken.  The kernel receives (ka, kb, u) per layer: at a
 *    key (u == 0 or u == 1 in step 5) or clamped, ka == kb is that key and u == 0.
 * 2. The sample S of a layer at joint j.  With u == 0, S is key ka's local bit for bit.  Otherwise S is step 5's blend of keys ka and kb under u:
 *    v = 1 - u, t and s per component v*a + u*b, q with d = ((a.x*b.x + a.y*b.y) + a.z*b.z) + a.w*b.w, u' = d < 0 ? -u : u, v*a + u'*b — the
 *    shorter-arc lerp, not normalised.
 * 3. The effective weight e = weight * mask[j], one rounded product; with mask -1, e = weight exactly.
 * 4. Layer 0 is the base: acc = S_0.  It must be OVERRIDE with mask -1 and weight 1.
 * 5. An OVERRIDE layer l >= 1.  e == 0 leaves acc as it is, bit for bit; e == 1 sets acc = S bit for bit; otherwise acc = the blend of step 2 with
 *    a = acc, b = S, u = e:  v = 1 - e;  t and s per component v*acc + e*S;  q with d = ((acc.x*S.x + acc.y*S.y) + acc.z*S.z) + acc.w*S.w,
 *    e' = d < 0 ? -e : e, per component v*acc + e'*S.
 *    NOTHING IS NORMALISED BETWEEN LAYERS; step 1 of include/pt_rig.h normalises once at the end.  What that costs: a blend of two unit
 *    quaternions is shorter than 1, at its midpoint by the cosine of half their 4-D angle, so a later layer, blended against that shorter acc,
 *    has its weight off by that factor (a layer of weight e over an acc of length c acts with weight e / (v*c + e) against the normalised acc).
 *    This is the same order as the normalised lerp's known deviation from the slerp, and the caller's remedy is the same: more keys, or layers
 *    that lie closer together.
 * 6. An ADDITIVE layer l >= 1 adds the clip's departure from its own key 0.  R is key 0's local of that slot at joint j; its quaternion is the
 *    caller's to keep unit.  e == 0 leaves acc bit for bit.  Otherwise
 *      t and s, per component:  acc = acc + e * (S - R)        the difference rounded, then the product, then the sum
 *      q:  dq = S.q (x) conj(R.q);  if dq.w < 0, dq is negated (exact);  dq' = (e*dq.x, e*dq.y, e*dq.z, (1 - e) + e*dq.w);  acc.q = dq' (x) acc.q
 *    with p (x) q, in this order,
 *      w = ((p.w*q.w - p.x*q.x) - p.y*q.y) - p.z*q.z
 *      x = ((p.w*q.x + p.x*q.w) + p.y*q.z) - p.z*q.y
 *      y = ((p.w*q.y - p.x*q.z) + p.y*q.w) + p.z*q.x
 *      z = ((p.w*q.z + p.x*q.y) - p.y*q.x) + p.z*q.w
 *    and conj negating x, y and z.  Consequence, to rounding: an additive layer at e == 1 over a base that equals R gives S.
 * 7. Output.  The two padding floats of an output local are written as 0.  The result is a LOCAL of include/pt_rig.h: steps 1-4 run on it where it
 *    lies.
 * A NaN in a key reaches the locals, the records and the pose as a NaN, and the pose refuses it (PT_ERR_SCENE) as it refuses every NaN.
 *
 * CONTRACTS.
 *   pt_rig_mix_locals is the mix alone, downloaded: n_parts locals.  pt_rig_mix_records(layers) equals pt_rig_records of what
 *   pt_rig_mix_locals(layers) returns, bit for bit.  Neither changes anything of the pose or the context.
 *   pt_rig_mix_pose_geometry leaves the context, the pose and what a later settle delivers exactly as pt_pose_geometry with those records would:
 *   return codes, refusals and slow paths, in_place and root_cost, the image history, the last accepted state and its rerun after a refusal
 *   (pt_rig_pose_geometry's contract, through the same path).  On the in-place path no local and no record is uploaded: the call uploads nothing
 *   but its kernel arguments and downloads R, as the rig's calls do.
 *   One OVERRIDE / CLAMP layer on a slot equals pt_rig_clip_records of the same clip at the same t, bit for bit.
 *   The calls of include/pt_rig.h behave exactly as before.
 *   While goals are set (include/pt_rig_ik.h) pt_rig_mix_records and pt_rig_mix_pose_geometry solve them over the mixed locals; pt_rig_mix_locals stays the mix alone.
 *
 * REFUSALS, all PT_ERR_ARG, in this order (the first failing check answers):
 *   pt_rig_mix_clip           a null or destroyed rig; a slot outside [0, 16); n_keys < 1; null times, or null values with n_parts > 0;
 *                             time_bytes != n_keys * 4; value_bytes != n_keys * n_parts * 48; times not finite or not strictly increasing.
 *   pt_rig_mix_mask           a null or destroyed rig; a slot outside [0, 8); null weights with n_parts > 0; weight_bytes != n_parts * 4;
 *                             a weight that is not finite or lies outside [0, 1].
 *   pt_rig_mix_locals, pt_rig_mix_records, pt_rig_mix_pose_geometry
 *                             (geometry) null ctx; a null or destroyed rig; (geometry) a rig whose pose was created on another context;
 *                             null layers; layer_bytes no multiple of 24, or fewer than 1 or more than 8 layers; then per layer, in the order of
 *                             the table: a clip slot outside [0, 16) or empty; a mask outside [-1, 8) or empty; an unknown mode; an unknown
 *                             wrap; a NaN t; an infinite t with LOOP; a weight that is not finite or lies outside [0, 1]; then layer 0 not
 *                             OVERRIDE with mask -1 and weight 1; then the output: (locals) null locals_out, local_bytes != n_parts * 48;
 *                             (records) null records_out, record_bytes != n_parts * 96; (geometry) ellip_bytes not a multiple of 4, then
 *                             pt_pose_geometry's PT_ERR_SCENE refusals under this call's name.
 *
 * OWNERSHIP, ORDER and threads: as include/pt_rig.h; the slots go with their rig.  pt_debug_rig_mix_time (include/pt_debug.h) times the mix's
 * launch.
 *
 * NOT BUILT: sparse per-channel tracks, slerp, cubic keys, morph-weight tracks in a clip, per-layer time scaling and blend trees above the flat
 * layer list, more than 8 layers, joints that write no record.
 */
#ifndef PT_RIG_MIX_H
#define PT_RIG_MIX_H
#include "pt_rig.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PT_RIG_MIX_SLOTS 16
#define PT_RIG_MIX_MASKS 8
#define PT_RIG_MIX_MAX_LAYERS 8
#define PT_RIG_MIX_OVERRIDE 0
#define PT_RIG_MIX_ADDITIVE 1
#define PT_RIG_MIX_CLAMP 0
#define PT_RIG_MIX_LOOP 1

typedef struct pt_rig_layer {
    int32_t clip, mask, mode, wrap;     /* a clip slot; a mask slot or -1; PT_RIG_MIX_OVERRIDE / ADDITIVE; PT_RIG_MIX_CLAMP / LOOP */
    float t, weight;
} pt_rig_layer;

int pt_rig_mix_clip(pt_rig* rig, int slot, int n_keys, const float* times, size_t time_bytes, const float* values, size_t value_bytes);
int pt_rig_mix_mask(pt_rig* rig, int slot, const float* weights, size_t weight_bytes);
int pt_rig_mix_locals(pt_rig* rig, const pt_rig_layer* layers, size_t layer_bytes, float* locals_out, size_t local_bytes);
int pt_rig_mix_records(pt_rig* rig, const pt_rig_layer* layers, size_t layer_bytes, float* records_out, size_t record_bytes);
int pt_rig_mix_pose_geometry(pt_ctx* ctx, pt_rig* rig, const pt_rig_layer* layers, size_t layer_bytes,
                             const float* ellip, size_t ellip_bytes, double* root_cost, int* in_place);

#ifdef __cplusplus
}
#endif
#endif
