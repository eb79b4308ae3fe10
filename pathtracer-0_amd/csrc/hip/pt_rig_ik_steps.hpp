// pt_rig_ik_steps.hpp — steps 0-7 of include/pt_rig_ik.h on one constraint, written once for both statements of the rule: ptp::rigIk
// (pt_rig_ik_rule.hpp, g++ or hipcc's host pass) and k_rig_ik (pt_rig_ik.hip, the device pass).  Plain floats and small arrays, no HIP type, so
// that a host compiler reads it; PT_IK_FN is the only thing that differs between the two.  The independent statement is the numpy model of the
// tests.  Binary32 throughout, every product rounded before every sum, in the written order: compiled with -ffp-contract=off wherever it is
// compiled, and on the device with the correctly rounded sqrt and /.  Clamps are comparisons and selects, never fmin / fmax: a NaN goes
// through them the same way everywhere.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PT_IK_FN __host__ __device__ inline
#else
#define PT_IK_FN inline
#endif

namespace ptik {

PT_IK_FN bool ok(float x) { return x != 0.0f && fabsf(x) <= 3.402823466e+38f; }
PT_IK_FN float dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
PT_IK_FN float len(const float* a) { return sqrtf(dot(a, a)); }
PT_IK_FN void cross(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
PT_IK_FN void over(const float* a, float d, float* o) { o[0] = a[0] / d; o[1] = a[1] / d; o[2] = a[2] / d; }

// n(q): include/pt_rig.h step 1's normalisation, (x y z w)
PT_IK_FN void unit(const float* q, float* n) {
    const float l = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    n[0] = q[0] / l; n[1] = q[1] / l; n[2] = q[2] / l; n[3] = q[3] / l;
}

// R(q): the nine expressions of include/pt_rig.h step 1 on q as it is, row-major
PT_IK_FN void rot(const float* q, float* R) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = 1.0f - 2.0f * (yy + zz); R[1] = 2.0f * (xy - wz); R[2] = 2.0f * (xz + wy);
    R[3] = 2.0f * (xy + wz); R[4] = 1.0f - 2.0f * (xx + zz); R[5] = 2.0f * (yz - wx);
    R[6] = 2.0f * (xz - wy); R[7] = 2.0f * (yz + wx); R[8] = 1.0f - 2.0f * (xx + yy);
}
// column c times s_c
PT_IK_FN void scaledCols(const float* R, const float* s, float* L) {
    for (int i = 0; i < 3; i++)
        for (int c = 0; c < 3; c++) L[3 * i + c] = R[3 * i + c] * s[c];
}
PT_IK_FN void apply(const float* M, const float* v, float* o) {
    for (int i = 0; i < 3; i++) o[i] = (M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2];
}

// p (x) q of include/pt_rig_mix.h step 6 on (x y z w); o is neither p nor q
PT_IK_FN void mul(const float* p, const float* q, float* o) {
    o[0] = ((p[3] * q[0] + p[0] * q[3]) + p[1] * q[2]) - p[2] * q[1];
    o[1] = ((p[3] * q[1] - p[0] * q[2]) + p[1] * q[3]) + p[2] * q[0];
    o[2] = ((p[3] * q[2] + p[0] * q[1]) - p[1] * q[0]) + p[2] * q[3];
    o[3] = ((p[3] * q[3] - p[0] * q[0]) - p[1] * q[1]) - p[2] * q[2];
}

// STEP 4's fromTo(u, v), the fallback axis included
PT_IK_FN void fromTo(const float* u, const float* v, float* q) {
    const float m[3] = {u[0] + v[0], u[1] + v[1], u[2] + v[2]};
    const float ml = len(m);
    if (ml == 0.0f) {
        const float k[3] = {0.0f, u[2], -u[1]};                       // cross(u, X)
        const float kl = len(k);
        if (kl == 0.0f) { q[0] = 0.0f; q[1] = 0.0f; q[2] = 1.0f; q[3] = 0.0f; return; }
        over(k, kl, q);
        q[3] = 0.0f;
        return;
    }
    float mh[3];
    over(m, ml, mh);
    cross(u, mh, q);
    q[3] = dot(u, mh);
}

// STEP 1.  P: 12 floats, rows (p_i0 p_i1 p_i2 p_i3), read only with hasP (false: the first joint is a root).  The cofactors and the determinant once, then
// any number of points
struct Frame { float c[9]; float det; float p3[3]; bool has; };
PT_IK_FN void frameOf(const float* P, bool hasP, Frame& F) {
    F.has = hasP;
    F.det = 1.0f;
    if (!F.has) return;
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
            F.c[3 * i + k] = P[4 * i1 + k1] * P[4 * i2 + k2] - P[4 * i1 + k2] * P[4 * i2 + k1];
        }
    F.det = (P[0] * F.c[0] + P[1] * F.c[1]) + P[2] * F.c[2];
    F.p3[0] = P[3]; F.p3[1] = P[7]; F.p3[2] = P[11];
}
PT_IK_FN void intoFrame(const Frame& F, const float* x, float* o) {
    if (!F.has) { o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; return; }
    const float d[3] = {x[0] - F.p3[0], x[1] - F.p3[1], x[2] - F.p3[2]};
    for (int k = 0; k < 3; k++) o[k] = ((F.c[k] * d[0] + F.c[3 + k] * d[1]) + F.c[6 + k] * d[2]) / F.det;
}

// STEP 6: n and q* under a weight that is not 0
PT_IK_FN void weighted(const float* n, const float* qs, float e, float* o) {
    if (e == 1.0f) { o[0] = qs[0]; o[1] = qs[1]; o[2] = qs[2]; o[3] = qs[3]; return; }
    const float v = 1.0f - e;
    const float d = ((n[0] * qs[0] + n[1] * qs[1]) + n[2] * qs[2]) + n[3] * qs[3];
    const float eq = d < 0.0f ? -e : e;
    for (int f = 0; f < 4; f++) o[f] = v * n[f] + eq * qs[f];
}

PT_IK_FN bool hasNan(const float* x) { return x[0] != x[0] || x[1] != x[1] || x[2] != x[2]; }

// STEPS 0-4, 6, 7 of a TWO_BONE constraint.  root, mid: 12-float locals; tipT: the tip's translation; P, hasP: the world matrix of root's parent, if any.
// true: qRoot and qMid are the new quaternions; false: the joints stay as they are
PT_IK_FN bool twoBone(const float* P, bool hasP, const float* root, const float* mid, const float* tipT, const float* target, const float* pole, bool usePole, float weight,
                      float* qRoot, float* qMid) {
    if (weight == 0.0f || hasNan(target)) return false;
    Frame F;
    frameOf(P, hasP, F);
    float g[3], pF[3] = {0.0f, 0.0f, 0.0f};
    intoFrame(F, target, g);
    if (usePole) intoFrame(F, pole, pF);
    // step 2
    float n0[4], n1[4], R[9], L0[9], L1[9];
    unit(root + 4, n0); unit(mid + 4, n1);
    rot(n0, R); scaledCols(R, root + 8, L0);
    rot(n1, R); scaledCols(R, mid + 8, L1);
    const float* a = root;
    float b[3], c[3], in[3], x[3];
    apply(L0, mid, x);
    for (int i = 0; i < 3; i++) b[i] = x[i] + a[i];
    apply(L1, tipT, x);
    for (int i = 0; i < 3; i++) in[i] = x[i] + mid[i];
    apply(L0, in, x);
    for (int i = 0; i < 3; i++) c[i] = x[i] + a[i];
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]}, v[3] = {g[0] - a[0], g[1] - a[1], g[2] - a[2]};
    const float l1 = len(e1), l2 = len(e2), dist = len(v);
    float eh[3];
    over(v, dist, eh);
    // step 3
    const float lo = fabsf(l1 - l2), hi = l1 + l2;
    float d = dist < lo ? lo : dist;
    d = d > hi ? hi : d;
    float cosA = ((l1 * l1 + d * d) - l2 * l2) / ((2.0f * l1) * d);
    cosA = cosA < -1.0f ? -1.0f : cosA;
    cosA = cosA > 1.0f ? 1.0f : cosA;
    const float sinA = sqrtf(1.0f - cosA * cosA);
    float h0[3];
    for (int i = 0; i < 3; i++) h0[i] = usePole ? pF[i] - a[i] : e1[i];
    const float along = dot(h0, eh);
    const float h[3] = {h0[0] - eh[0] * along, h0[1] - eh[1] * along, h0[2] - eh[2] * along};
    const float hl = len(h);
    float hh[3], u1[3], bp[3], cp[3];
    over(h, hl, hh);
    for (int i = 0; i < 3; i++) {
        u1[i] = cosA * eh[i] + sinA * hh[i];
        bp[i] = a[i] + l1 * u1[i];
        cp[i] = a[i] + d * eh[i];
    }
    // step 4
    float r1[4], r2[4], e1h[3], e2p[3], e2h[3], wh[3];
    over(e1, l1, e1h);
    fromTo(e1h, u1, r1);
    rot(r1, R);
    apply(R, e2, e2p);
    const float l2p = len(e2p);
    const float w[3] = {cp[0] - bp[0], cp[1] - bp[1], cp[2] - bp[2]};
    const float wl = len(w);
    over(e2p, l2p, e2h);
    over(w, wl, wh);
    fromTo(e2h, wh, r2);
    float q0[4], q1[4], t0[4], t1[4];
    mul(r1, n0, q0);
    const float conj[4] = {-q0[0], -q0[1], -q0[2], q0[3]};
    mul(conj, r2, t0);
    mul(t0, q0, t1);
    mul(t1, n1, q1);
    // step 7
    if (!(ok(F.det) && ok(l1) && ok(l2) && ok(dist) && ok(hl) && ok(l2p) && ok(wl))) return false;
    weighted(n0, q0, weight, qRoot);
    weighted(n1, q1, weight, qMid);
    return true;
}

// STEPS 0, 1, 5-7 of an AIM constraint on the joint with local `j`
PT_IK_FN bool aim(const float* P, bool hasP, const float* j, const float* axis, const float* target, float weight, float* qOut) {
    if (weight == 0.0f || hasNan(target)) return false;
    Frame F;
    frameOf(P, hasP, F);
    float g[3], n[4], R[9], u[3], wh[3], r[4], q[4];
    intoFrame(F, target, g);
    unit(j + 4, n);
    rot(n, R);
    apply(R, axis, u);
    const float w[3] = {g[0] - j[0], g[1] - j[1], g[2] - j[2]};
    const float wl = len(w);
    over(w, wl, wh);
    fromTo(u, wh, r);
    mul(r, n, q);
    if (!(ok(F.det) && ok(wl))) return false;
    weighted(n, q, weight, qOut);
    return true;
}

}  // namespace ptik
