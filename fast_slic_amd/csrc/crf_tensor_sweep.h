// crf_tensor_sweep.h -- the device code that the sweep (crf_tensor.hip) and its adjoint (crf_tensor_grad.hip) both run: the clamp of a
// pair of row bounds, the coordinates of a sweep block, and the forward's message, exponential and class sum.  The adjoint recomputes
// the forward through these very functions, so the two have the same bits by construction.  Device code only.
#pragma once
#include "crf.h"
#include "crf_tensor.h"

// The roundings are crf.hip's (see there and crf.h): products fused exactly where the reference build fuses them, nothing else.
#pragma clang fp contract(off)

namespace fslic {

// The bounds offsets[g], offsets[g + 1] clamped into [0, nnz] and to non-decreasing: whatever the offsets hold, 0 <= x <= y <= nnz,
// and nothing indexed by an entry number is touched outside x <= k < y.
static __device__ __forceinline__ uint2 crf_clamped_bounds(const int64_t* __restrict__ offsets, size_t g, long long nnz) {
    long long k0 = offsets[g], k1 = offsets[g + 1];
    k0 = k0 < 0 ? 0 : (k0 > nnz ? nnz : k0);
    k1 = k1 < 0 ? 0 : (k1 > nnz ? nnz : k1);
    if (k1 < k0) k1 = k0;
    return make_uint2((uint32_t)k0, (uint32_t)k1);
}

// A thread of a sweep block (crf_tensor_sweep_shape): its node, its class slice (classes wave, wave + waves, ...) and its columns of
// the block's two [C] planes.  m[cls * stride] is the message of (node, cls), x[cls * stride] the second plane's value.
struct CrfSweepThread {
    int w, i;                   // the frame, the node
    int lane, wave, waves;
    bool live;                  // i < K (a lane past the frame's end only keeps the barriers)
    bool has_prev, has_next;    // temporal links towards w - 1 and w + 1
    size_t CK, base;            // C * K; w * C * K, where the frame's [C][K] planes begin
    float* m;
    float* x;
    size_t stride;
};
// LDS: the planes are lds[2][C][64].  Otherwise they are [N][C][K] planes in memory, above kCrfTensorLdsClasses classes.
template <bool LDS>
static __device__ __forceinline__ CrfSweepThread crf_sweep_thread(const CrfTensorParams& dp, float* lds, float* msg, float* second) {
    CrfSweepThread t;
    const int tiles = (dp.K + kCrfTensorNodes - 1) / kCrfTensorNodes;
    t.w = blockIdx.x / tiles;
    t.lane = threadIdx.x % kCrfTensorNodes, t.wave = threadIdx.x / kCrfTensorNodes, t.waves = blockDim.x / kCrfTensorNodes;
    t.i = (blockIdx.x - t.w * tiles) * kCrfTensorNodes + t.lane;
    t.live = t.i < dp.K;
    t.CK = (size_t)dp.C * dp.K, t.base = (size_t)t.w * t.CK;
    t.m = LDS ? lds + t.lane : msg + t.base + t.i;
    t.x = LDS ? lds + (size_t)dp.C * kCrfTensorNodes + t.lane : second + t.base + t.i;
    t.stride = LDS ? (size_t)kCrfTensorNodes : (size_t)dp.K;
    t.has_prev = dp.temporal && t.w > 0, t.has_next = dp.temporal && t.w < dp.N - 1;
    return t;
}

// Message passing (simple-crf.cpp:71-102) for (the thread's node, cls): neighbours in list order, then t-1, then t+1; each term
// fma(e * q, factor, message).  r and tl are the node's row bounds and temporal entry.
static __device__ __forceinline__ float crf_sweep_message(const CrfSweepThread& t, int K, uint2 r, float4 tl,
                                                          const int32_t* __restrict__ idx, const float2* __restrict__ edge,
                                                          const float* __restrict__ q_in, int cls) {
    const float* qc = q_in + t.base + (size_t)cls * K;
    float message = 0.0f;
    for (uint32_t k = r.x; k < r.y; ++k) {
        const float2 es = edge[k];
        if (es.y == kCrfDeadEntry) continue;                                   // idx[k] is outside [0, K)
        message = __builtin_fmaf(es.x * qc[idx[k]], es.y, message);
    }
    if (t.has_prev) message = __builtin_fmaf(tl.x * qc[t.i - (ptrdiff_t)t.CK], tl.y, message);
    if (t.has_next) message = __builtin_fmaf(tl.z * qc[t.i + t.CK], tl.w, message);
    return message;
}

// Compatibility transform (:104-114) for (the thread's node, cls), behind the barrier that follows the messages: the Potts sum over
// the other classes in ascending order (fused), then expf.
static __device__ __forceinline__ float crf_sweep_exp(const CrfSweepThread& t, int C, int K, const float* __restrict__ compat,
                                                      const float* __restrict__ unary, int cls) {
    float gathered = 0.0f;
    for (int o = 0; o < cls; ++o) gathered = __builtin_fmaf(compat[o], t.m[o * t.stride], gathered);
    for (int o = cls + 1; o < C; ++o) gathered = __builtin_fmaf(compat[o], t.m[o * t.stride], gathered);
    return crf_expf(-(unary[t.base + (size_t)cls * K + t.i] + gathered));
}

// Normalisation (:116-133), behind the barrier that follows the exponentials in t.x: their sum over the classes in ascending order
// from 0.0f.  The reference clamps it at 1e-5 by crf_sweep_clamps, a double comparison as written there.
static __device__ __forceinline__ float crf_sweep_class_sum(const CrfSweepThread& t, int C) {
    float sum = 0.0f;
    for (int cls = 0; cls < C; ++cls) sum += t.x[cls * t.stride];
    return sum;
}
static __device__ __forceinline__ bool crf_sweep_clamps(float sum) { return (double)sum < 1e-5; }

}  // namespace fslic
