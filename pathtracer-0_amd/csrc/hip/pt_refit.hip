// pt_refit.hip — refit a scene's BVHs to moved triangles (include/pt_refit.h): the boxes of binding 10 recomputed bottom-up over the topology of
// bindings 11-13, which pt_refit_plan.hpp has validated and ordered by height on the host.
//
//   k_refit_leaves   one lane per reachable leaf: min / max over the nine vertex floats of its triangles (three float4 loads per triangle, the
//                    first 48 bytes of the 160-byte record), the leaf's cost term, the NaN flag
//   k_refit_level    one lane per node of one height: the union of its two children's boxes, which an earlier launch wrote
//   k_refit_tail     the upper heights once all their nodes fit one block: one launch, __syncthreads() between heights
//   k_refit_roots    root_cost[r] = S(root r)
// Kernel boundaries (and, inside the one block of k_refit_tail, the block barrier) are the only ordering between a child's store and its parent's
// load; there is no counter or flag hand-off between blocks.  min / max run on order-preserving 32-bit keys, so that -0.0 < +0.0 as in Java's
// Math.min / Math.max and pt_bvh.hip; they do not round, so the result is independent of the order.  The cost is binary64 in the written order;
// the file is compiled with -ffp-contract=off like the rest of the library.  Every index a kernel follows was range-checked by planRefit.
#include <hip/hip_runtime.h>

#include "pt_refit_state.hpp"

#include <cstdint>
#include <mutex>
#include <set>
#include <string>
#include <vector>

int pt_set_error_(int code, const std::string& msg);     // pt_hip.hip

namespace {

constexpr int BLOCK = ptr::TAIL_BLOCK;

std::mutex g_plansMutex;
std::set<pt_refit_plan*> g_plans;                        // the live plans: a destroyed one is refused, not followed

__device__ __forceinline__ unsigned fkey(float f) { unsigned b = __float_as_uint(f); return (b >> 31) ? ~b : (b | 0x80000000u); }

struct Box6 {
    float mn[3], mx[3];
    __device__ void grow(float x, float y, float z) {
        const float v[3] = {x, y, z};
        for (int k = 0; k < 3; k++) {
            if (fkey(v[k]) < fkey(mn[k])) mn[k] = v[k];
            if (fkey(v[k]) > fkey(mx[k])) mx[k] = v[k];
        }
    }
    __device__ double area() const {
        const double sx = (double)mx[0] - (double)mn[0], sy = (double)mx[1] - (double)mn[1], sz = (double)mx[2] - (double)mn[2];
        return (sx * sy + sx * sz) + sy * sz;
    }
    __device__ void load(const float* row) {
        const float4 a = *reinterpret_cast<const float4*>(row);
        const float2 b = *reinterpret_cast<const float2*>(row + 4);
        mn[0] = a.x; mn[1] = a.y; mn[2] = a.z; mx[0] = a.w; mx[1] = b.x; mx[2] = b.y;
    }
    __device__ void store(float* row) const {            // floats 6 and 7 of the row stay
        *reinterpret_cast<float4*>(row) = make_float4(mn[0], mn[1], mn[2], mx[0]);
        *reinterpret_cast<float2*>(row + 4) = make_float2(mx[1], mx[2]);
    }
};

__global__ void __launch_bounds__(BLOCK) k_refit_leaves(const float* __restrict__ tris, const int32_t* __restrict__ leafTris, const int32_t* __restrict__ order,
                                                       int nLeaves, float* data, double* S, int* nanFlag) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= nLeaves) return;
    const int node = order[p];
    float* row = data + 8 * (size_t)node;
    const float2 range = *reinterpret_cast<const float2*>(row + 6);
    const int start = (int)range.x, end = (int)range.y;
    Box6 b;
    if (start == end) {                                  // an empty leaf keeps its box
        b.load(row);
        S[node] = b.area() * 0.0;
        return;
    }
    bool bad = false;
    for (int k = start; k < end; k++) {
        const float4* t = reinterpret_cast<const float4*>(tris + 40 * (size_t)leafTris[k]);
        const float4 v0 = t[0], v1 = t[1], v2 = t[2];
        bad = bad || v0.x != v0.x || v0.y != v0.y || v0.z != v0.z || v1.x != v1.x || v1.y != v1.y || v1.z != v1.z || v2.x != v2.x || v2.y != v2.y || v2.z != v2.z;
        if (k == start) { b.mn[0] = b.mx[0] = v0.x; b.mn[1] = b.mx[1] = v0.y; b.mn[2] = b.mx[2] = v0.z; }
        else b.grow(v0.x, v0.y, v0.z);
        b.grow(v1.x, v1.y, v1.z);
        b.grow(v2.x, v2.y, v2.z);
    }
    if (bad) *nanFlag = 1;
    b.store(row);
    S[node] = b.area() * (double)(end - start);
}

// the node at position p of the schedule: the union of its children's stored boxes, S = A + (S(left) + S(right))
__device__ __forceinline__ void refitInner(int node, const int32_t* __restrict__ tree, float* data, double* S) {
    const int l = tree[3 * (size_t)node + 1], r = tree[3 * (size_t)node + 2];
    Box6 a, c;
    a.load(data + 8 * (size_t)l);
    c.load(data + 8 * (size_t)r);
    for (int k = 0; k < 3; k++) {
        if (fkey(c.mn[k]) < fkey(a.mn[k])) a.mn[k] = c.mn[k];
        if (fkey(c.mx[k]) > fkey(a.mx[k])) a.mx[k] = c.mx[k];
    }
    a.store(data + 8 * (size_t)node);
    S[node] = a.area() + (S[l] + S[r]);
}

__global__ void __launch_bounds__(BLOCK) k_refit_level(const int32_t* __restrict__ tree, const int32_t* __restrict__ order, int first, int last, float* data, double* S) {
    const int p = first + blockIdx.x * BLOCK + threadIdx.x;
    if (p < last) refitInner(order[p], tree, data, S);
}

// heights [hFirst, hLast]: together at most BLOCK nodes, so no height has more; one block
__global__ void __launch_bounds__(BLOCK) k_refit_tail(const int32_t* __restrict__ tree, const int32_t* __restrict__ order, const int32_t* __restrict__ levelStart,
                                                     int hFirst, int hLast, float* data, double* S) {
    for (int h = hFirst; h <= hLast; h++) {
        const int p = levelStart[h] + (int)threadIdx.x;
        if (p < levelStart[h + 1]) refitInner(order[p], tree, data, S);
        __syncthreads();
    }
}

__global__ void k_refit_roots(const int32_t* __restrict__ roots, int nRoots, const double* __restrict__ S, double* out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nRoots) out[r] = S[roots[r]];
}

#define REFIT_TRY(x)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (x);                                                                           \
        if (e_ != hipSuccess) return pt_set_error_(PT_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

int uploadPlan(pt_refit_plan& P, const ptr::RefitInput& in) {
    const ptr::RefitSchedule& s = P.s;
    REFIT_TRY(hipStreamCreate(&P.stream));
    const hipStream_t st = P.stream;
    REFIT_TRY(P.dData.upload(in.data, in.dataBytes, st));
    REFIT_TRY(P.dTree.upload(in.tree, in.treeBytes, st));
    REFIT_TRY(P.dLeaf.upload(in.leaf, in.leafBytes, st));
    REFIT_TRY(P.dOrder.upload(s.order.data(), s.order.size() * 4, st));
    REFIT_TRY(P.dLevelStart.upload(s.levelStart.data(), s.levelStart.size() * 4, st));
    REFIT_TRY(P.dRoots.upload(s.roots.data(), s.roots.size() * 4, st));
    REFIT_TRY(P.dTris.reset(P.nTris ? (size_t)P.nTris * 160 : 16));
    REFIT_TRY(P.dS.reset(s.nNodes ? (size_t)s.nNodes * 8 : 16));
    REFIT_TRY(P.dRootCost.reset(s.nRoots ? (size_t)s.nRoots * 8 : 16));
    REFIT_TRY(P.dFlag.reset(16));
    REFIT_TRY(hipStreamSynchronize(st));                 // the schedule's vectors are pageable: the copies have left them by now
    return PT_OK;
}

}  // namespace

extern "C" int pt_refit_create(int device, const float* bvh_data, size_t data_bytes, const int32_t* bvh_tree, size_t tree_bytes, const int32_t* leaf_tris,
                               size_t leaf_bytes, const int32_t* obj_roots, size_t roots_bytes, int64_t n_tris, pt_refit_plan** out) {
    if (!out) return pt_set_error_(PT_ERR_ARG, "pt_refit_create: null out pointer");
    ptr::RefitInput in;
    in.data = bvh_data; in.dataBytes = data_bytes; in.tree = bvh_tree; in.treeBytes = tree_bytes; in.leaf = leaf_tris; in.leafBytes = leaf_bytes;
    in.roots = obj_roots; in.rootsBytes = roots_bytes; in.nTris = n_tris;
    pt_refit_plan* P = new pt_refit_plan();
    std::string err;
    int rc = ptr::planRefit(in, P->s, err);
    if (rc) { delete P; return pt_set_error_(rc, err); }
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || nDev < 1) { delete P; return pt_set_error_(PT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)"); }
    if (device < 0 || device >= nDev) { delete P; return pt_set_error_(PT_ERR_NO_DEVICE, "pt_refit_create: HIP device index out of range"); }
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess || std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        delete P;
        return pt_set_error_(PT_ERR_NO_DEVICE, "pt_refit_create: the device is not a usable gfx950 (this library is built for gfx950 only)");
    }
    P->device = device; P->dataBytes = data_bytes; P->nTris = n_tris;
    P->digest = ptr::topologyDigest(bvh_tree, tree_bytes / 4, leaf_tris, leaf_bytes / 4, obj_roots, roots_bytes / 4, bvh_data, data_bytes / 4);
    rc = uploadPlan(*P, in);
    if (rc) { delete P; return rc; }
    { std::lock_guard<std::mutex> g(g_plansMutex); g_plans.insert(P); }
    *out = P;
    return PT_OK;
}

bool pt_refit_live_(pt_refit_plan* P) {
    std::lock_guard<std::mutex> g(g_plansMutex);
    return P && g_plans.count(P);
}

int pt_refit_device_(pt_refit_plan* P, const float* tris, size_t tri_bytes, const char* who) {
    REFIT_TRY(hipSetDevice(P->device));
    if (tri_bytes) REFIT_TRY(hipMemcpyAsync(P->dTris, tris, tri_bytes, hipMemcpyHostToDevice, P->stream));
    return pt_refit_kernels_(P, who);
}

int pt_refit_kernels_(pt_refit_plan* P, const char* who) {
    const ptr::RefitSchedule& s = P->s;
    const hipStream_t st = P->stream;
    REFIT_TRY(hipSetDevice(P->device));
    REFIT_TRY(hipMemsetAsync(P->dFlag, 0, 4, st));
    const int nLeaves = s.nLeaves();
    if (nLeaves > 0)
        hipLaunchKernelGGL(k_refit_leaves, dim3((nLeaves + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, P->dTris, P->dLeaf, P->dOrder, nLeaves, P->dData, P->dS, P->dFlag);
    const int tail = s.tailFrom();
    for (int h = 1; h < tail; h++) {
        const int first = s.levelStart[h], last = s.levelStart[h + 1];
        hipLaunchKernelGGL(k_refit_level, dim3((last - first + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, P->dTree, P->dOrder, first, last, P->dData, P->dS);
    }
    if (tail >= 1 && tail <= s.maxHeight)
        hipLaunchKernelGGL(k_refit_tail, dim3(1), dim3(BLOCK), 0, st, P->dTree, P->dOrder, P->dLevelStart, tail, s.maxHeight, P->dData, P->dS);
    if (s.nRoots > 0)
        hipLaunchKernelGGL(k_refit_roots, dim3((s.nRoots + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, P->dRoots, s.nRoots, P->dS, P->dRootCost);
    REFIT_TRY(hipGetLastError());
    int flag = 0;
    REFIT_TRY(hipMemcpyAsync(&flag, P->dFlag, 4, hipMemcpyDeviceToHost, st));
    REFIT_TRY(hipStreamSynchronize(st));
    if (flag) return pt_set_error_(PT_ERR_SCENE, std::string(who) + ": NaN coordinate in a referenced triangle");
    return PT_OK;
}

extern "C" int pt_refit_run(pt_refit_plan* P, const float* tris, size_t tri_bytes, float* bvh_data_out, double* root_cost) {
    if (!pt_refit_live_(P)) return pt_set_error_(PT_ERR_ARG, "pt_refit_run: null or destroyed plan");
    if (!tris || !bvh_data_out) return pt_set_error_(PT_ERR_ARG, "pt_refit_run: null pointer");
    if (tri_bytes != (size_t)P->nTris * 160) return pt_set_error_(PT_ERR_ARG, "pt_refit_run: tri_bytes != n_tris * 160");
    if (const int rc = pt_refit_device_(P, tris, tri_bytes, "pt_refit_run")) return rc;
    const ptr::RefitSchedule& s = P->s;
    const hipStream_t st = P->stream;
    if (P->dataBytes) REFIT_TRY(hipMemcpyAsync(bvh_data_out, P->dData, P->dataBytes, hipMemcpyDeviceToHost, st));
    if (root_cost && s.nRoots > 0) REFIT_TRY(hipMemcpyAsync(root_cost, P->dRootCost, (size_t)s.nRoots * 8, hipMemcpyDeviceToHost, st));
    REFIT_TRY(hipStreamSynchronize(st));
    return PT_OK;
}

extern "C" void pt_refit_destroy(pt_refit_plan* P) {
    if (!P) return;
    {
        std::lock_guard<std::mutex> g(g_plansMutex);
        if (!g_plans.erase(P)) return;                   // not a live plan: destroyed already
    }
    delete P;
}
