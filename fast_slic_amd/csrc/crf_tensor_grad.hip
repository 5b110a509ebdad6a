// crf_tensor_grad.hip -- the backward of SimpleCRF inference on device tensors (crf_tensor_grad.h; the forward is crf_tensor.hip, the
// C ABI is in crfapi.cpp).  One sweep is, per (node i, class c),
//   m[i,c] = sum_k e_k f_k q[j_k,c] + a_i q[n-1,i,c] + b_i q[n+1,i,c],  g[i,c] = sum_{o != c} compat[o] m[i,o],
//   ex = crf_expf(-(u + g)),  s_i = max(sum_c ex, 1e-5),  q' = ex / s_i,
// and its adjoint, with G' the gradient with respect to q',
//   d_i = sum_c G'[i,c] q'[i,c] (0 where the forward's sum was clamped),  da[i,c] = -q'[i,c] (G'[i,c] - d_i),  du += da,
//   S[i,o] = sum_{c != o} da[i,c],  dcompat[o] += sum_{n,i} m[i,o] S[i,o],  dm[i,o] = compat[o] S[i,o],
//   G[j,c] = sum_{k: j_k = j} e_k f_k dm[row(k),c] + a_(n+1,j) dm[n+1,j,c] + b_(n-1,j) dm[n-1,j,c].
//   k_crf_tensor_sweep_bwd   one launch per sweep, last sweep first, in the forward sweep's block shape: 64 consecutive nodes of one
//                            frame (the lanes) times one wavefront per class slice.  Thread (node, class) gathers its G' over the
//                            TRANSPOSED row (crf_grad_gather; the first launch reads the incoming gradient), recomputes its message
//                            from the saved q with the forward's operations, then the compatibility sum, the exponential and the
//                            node's clamped sum as the forward takes them; d_i and S come from [C][64] planes, every thread adding
//                            the classes in ascending order itself.  Two planes: the messages, and one that holds the exponentials,
//                            then G' q', then da (a barrier between the last read of one and the first write of the next).  G' of a
//                            thread waits in its own cell of dm_out, which it overwrites with dm at the end.  Above
//                            kCrfTensorLdsClasses classes both planes are the workspace's.
//   k_crf_tensor_grad_close  one thread per cell: the last gather, then dq0 = G or du += -q_start G.
//   k_crf_tensor_grad_compat one thread per class: the blocks' slots added in ascending block order.
// Determinism: no atomics.  Every output cell and every slot has one owner thread, every sum one fixed order: du and dm belong to
// thread (node, class), a slot to lane 0 of the wavefront of (block, class) after the fixed-order wave_reduce_add, the launches of a
// call follow each other on one stream.  That is why G is a gather over the transposed lists and not a scatter.
// Memory safety with a CSR that is not one: the transposed bounds are clamped as the forward clamps a row's; a transposed entry
// counts only when its source row is a node of the gathering frame, the entry number lies inside that row's clamped bounds in `rows`
// (so it is below nnz and edge[] of it was written by k_crf_tensor_edges), and the entry is live.
// Every grid is exact (one trip), as the forward's.
#include "crf.h"
#include "crf_tensor_grad.h"
#include "device_common.h"

// The recomputed message, exponential and sum must be the forward's bits: the same operations under the same contraction rule.
#pragma clang fp contract(off)

namespace fslic {

struct CrfGradLists {
    const uint2* rows;
    const float2* edge;
    const float4* temporal;
    CrfTensorTransposed tr;
};

// The bounds of the transposed row of (frame, node) g, clamped into [0, nnz] and to non-decreasing.
static __device__ __forceinline__ uint2 crf_grad_bounds(const CrfTensorParams& dp, const int64_t* __restrict__ offsets, size_t g) {
    long long t0 = offsets[g], t1 = offsets[g + 1];
    t0 = t0 < 0 ? 0 : (t0 > dp.nnz ? dp.nnz : t0);
    t1 = t1 < 0 ? 0 : (t1 > dp.nnz ? dp.nnz : t1);
    if (t1 < t0) t1 = t0;
    return make_uint2((uint32_t)t0, (uint32_t)t1);
}

// G[w, cls, i] from the dm of the sweep that read it: the transposed entries in list order, then frame w + 1, then frame w - 1.
static __device__ __forceinline__ float crf_grad_gather(const CrfTensorParams& dp, const CrfGradLists& L, const float* __restrict__ dm,
                                                        uint2 tb, int w, int i, int cls) {
    const int K = dp.K;
    const size_t CK = (size_t)dp.C * K;
    const float* dc = dm + (size_t)w * CK + (size_t)cls * K;
    const uint32_t first_row = (uint32_t)w * (uint32_t)K;
    float G = 0.0f;
    for (uint32_t t = tb.x; t < tb.y; ++t) {
        const uint32_t node = (uint32_t)L.tr.rows[t] - first_row;             // the source row as a node of this frame
        if (node >= (uint32_t)K) continue;
        const uint32_t k = (uint32_t)L.tr.entries[t];
        const uint2 r = L.rows[first_row + node];
        if (k < r.x || k >= r.y) continue;                                     // r.y <= nnz: edge[k] exists and was written
        const float2 es = L.edge[k];
        if (es.y == kCrfDeadEntry) continue;
        G = __builtin_fmaf(es.x * dc[node], es.y, G);
    }
    if (dp.temporal && w < dp.N - 1) {                                         // node i of w + 1 read this cell as its t - 1
        const float4 t = L.temporal[(size_t)(w + 1) * K + i];
        G = __builtin_fmaf(t.x * dc[i + CK], t.y, G);
    }
    if (dp.temporal && w > 0) {                                                // node i of w - 1 read it as its t + 1
        const float4 t = L.temporal[(size_t)(w - 1) * K + i];
        G = __builtin_fmaf(t.z * dc[i - (ptrdiff_t)CK], t.w, G);
    }
    return G;
}

// m[cls * stride] and x[cls * stride] are the message and the second plane's value of (the thread's node, cls): LDS, or the workspace's
// planes above kCrfTensorLdsClasses classes.
template <bool LDS>
__global__ __launch_bounds__(kCrfTensorNodes * kCrfTensorWaves) void k_crf_tensor_sweep_bwd(
        CrfTensorParams dp, CrfGradLists L, const int32_t* __restrict__ idx, const float* __restrict__ unary,
        const float* __restrict__ compat, const float* __restrict__ q_in, const float* __restrict__ q_new,
        const float* __restrict__ grad_new, const float* __restrict__ dm_in, float* __restrict__ dm_out, float* __restrict__ du,
        float* __restrict__ slots, float* msg, float* xpl, int first) {
    extern __shared__ float s_crf_grad[];
    const int C = dp.C, K = dp.K;
    const int tiles = (K + kCrfTensorNodes - 1) / kCrfTensorNodes;
    const int w = blockIdx.x / tiles;                                          // the frame
    const int lane = threadIdx.x % kCrfTensorNodes, wave = threadIdx.x / kCrfTensorNodes, waves = blockDim.x / kCrfTensorNodes;
    const int i = (blockIdx.x - w * tiles) * kCrfTensorNodes + lane;           // the node
    const bool live = i < K;                                                   // (a lane past the frame's end only keeps the barriers)
    const size_t CK = (size_t)C * K, base = (size_t)w * CK;
    float* m = LDS ? s_crf_grad + lane : msg + base + i;
    float* x = LDS ? s_crf_grad + (size_t)C * kCrfTensorNodes + lane : xpl + base + i;
    const size_t stride = LDS ? (size_t)kCrfTensorNodes : (size_t)K;
    const bool has_prev = dp.temporal && w > 0, has_next = dp.temporal && w < dp.N - 1;

    // G' of every class of the slice into the thread's own cells of dm_out; the message as k_crf_tensor_sweep takes it
    if (live) {
        const uint2 r = L.rows[(size_t)w * K + i];
        const float4 t = L.temporal[(size_t)w * K + i];
        const uint2 tb = grad_new ? make_uint2(0u, 0u) : crf_grad_bounds(dp, L.tr.offsets, (size_t)w * K + i);
        for (int cls = wave; cls < C; cls += waves) {
            const size_t cell = base + (size_t)cls * K + i;
            dm_out[cell] = grad_new ? grad_new[cell] : crf_grad_gather(dp, L, dm_in, tb, w, i, cls);
            const float* qc = q_in + base + (size_t)cls * K;
            float message = 0.0f;
            for (uint32_t k = r.x; k < r.y; ++k) {
                const float2 es = L.edge[k];
                if (es.y == kCrfDeadEntry) continue;
                message = __builtin_fmaf(es.x * qc[idx[k]], es.y, message);
            }
            if (has_prev) message = __builtin_fmaf(t.x * qc[i - (ptrdiff_t)CK], t.y, message);
            if (has_next) message = __builtin_fmaf(t.z * qc[i + CK], t.w, message);
            m[cls * stride] = message;
        }
    }
    __syncthreads();
    // the compatibility sum and the exponential, as the forward
    if (live) {
        for (int cls = wave; cls < C; cls += waves) {
            float gathered = 0.0f;
            for (int o = 0; o < cls; ++o) gathered = __builtin_fmaf(compat[o], m[o * stride], gathered);
            for (int o = cls + 1; o < C; ++o) gathered = __builtin_fmaf(compat[o], m[o * stride], gathered);
            x[cls * stride] = crf_expf(-(unary[base + (size_t)cls * K + i] + gathered));
        }
    }
    __syncthreads();
    // the forward's own clamp decision: where it clamped, the sum was a constant
    bool clamped = false;
    if (live) {
        float sum = 0.0f;
        for (int cls = 0; cls < C; ++cls) sum += x[cls * stride];
        clamped = (double)sum < 1e-5;
    }
    __syncthreads();                                                           // every sum is taken before the plane is reused
    if (live)
        for (int cls = wave; cls < C; cls += waves) {
            const size_t cell = base + (size_t)cls * K + i;
            x[cls * stride] = dm_out[cell] * q_new[cell];
        }
    __syncthreads();
    float d = 0.0f;
    if (live && !clamped)
        for (int cls = 0; cls < C; ++cls) d += x[cls * stride];
    __syncthreads();
    if (live)
        for (int cls = wave; cls < C; cls += waves) {
            const size_t cell = base + (size_t)cls * K + i;
            const float da = -q_new[cell] * (dm_out[cell] - d);
            x[cls * stride] = da;
            du[cell] = first ? da : du[cell] + da;
        }
    __syncthreads();
    // S over the other classes in ascending order; dm; the block's part of dcompat (the loop is uniform over the wavefront)
    float* slot = slots ? slots + (size_t)blockIdx.x * C : nullptr;
    for (int cls = wave; cls < C; cls += waves) {
        float S = 0.0f, part = 0.0f;
        if (live) {
            for (int o = 0; o < cls; ++o) S += x[o * stride];
            for (int o = cls + 1; o < C; ++o) S += x[o * stride];
            dm_out[base + (size_t)cls * K + i] = compat[cls] * S;
            if (slot) part = m[cls * stride] * S;
        }
        if (slot) {
            const float total = wave_reduce_add<float>(part);
            if (lane == 0) slot[cls] = first ? total : slot[cls] + total;
        }
    }
}

__global__ __launch_bounds__(256) void k_crf_tensor_grad_close(CrfTensorParams dp, CrfGradLists L, const float* __restrict__ q_start,
                                                               const float* __restrict__ grad_start, const float* __restrict__ dm_in,
                                                               float* __restrict__ du, float* __restrict__ dq0, int first) {
    const size_t n = (size_t)dp.N * dp.C * dp.K;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int K = dp.K, C = dp.C;
    const int plane = (int)(p / (size_t)K), i = (int)(p - (size_t)plane * K);
    const int w = plane / C, cls = plane - w * C;
    const float G = grad_start ? grad_start[p] : crf_grad_gather(dp, L, dm_in, crf_grad_bounds(dp, L.tr.offsets, (size_t)w * K + i), w, i, cls);
    if (dq0) {
        dq0[p] = G;
        if (first) du[p] = 0.0f;
    } else {                                                                   // q_start = crf_expf(-u)
        const float v = -(q_start[p] * G);
        du[p] = first ? v : du[p] + v;
    }
}

__global__ __launch_bounds__(256) void k_crf_tensor_grad_compat(const float* __restrict__ slots, size_t blocks, int C, float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.0f;
    for (size_t b = 0; b < blocks; ++b) s += slots[b * C + c];
    out[c] = s;
}

void launch_crf_tensor_sweep_bwd(const CrfTensorParams& dp, const uint2* rows, const int32_t* indices, const float2* edge,
                                 const float4* temporal, const CrfTensorTransposed& tr, const float* unaries, const float* compat,
                                 const float* q_in, const float* q_new, const float* grad_new, const float* dm_in, float* dm_out,
                                 float* grad_unaries, float* slots, float* msg, float* x, bool first, hipStream_t st) {
    // the forward sweep's block shape (launch_crf_tensor_sweep)
    const int per = (dp.C + kCrfTensorWaves - 1) / kCrfTensorWaves, waves = (dp.C + per - 1) / per;
    const dim3 grid((unsigned)crf_tensor_grad_blocks(dp.N, dp.K)), block(kCrfTensorNodes * waves);
    const CrfGradLists L = {rows, edge, temporal, tr};
    if (dp.C <= kCrfTensorLdsClasses)
        launch(k_crf_tensor_sweep_bwd<true>, grid, block, (unsigned)(2 * sizeof(float) * kCrfTensorNodes * dp.C), st,
               dp, L, indices, unaries, compat, q_in, q_new, grad_new, dm_in, dm_out, grad_unaries, slots, msg, x, (int)first);
    else
        launch(k_crf_tensor_sweep_bwd<false>, grid, block, 0, st,
               dp, L, indices, unaries, compat, q_in, q_new, grad_new, dm_in, dm_out, grad_unaries, slots, msg, x, (int)first);
}

void launch_crf_tensor_grad_close(const CrfTensorParams& dp, const uint2* rows, const float2* edge, const float4* temporal,
                                  const CrfTensorTransposed& tr, const float* q_start, const float* grad_start, const float* dm_in,
                                  float* grad_unaries, float* grad_q0, bool first, hipStream_t st) {
    const size_t n = (size_t)dp.N * dp.C * dp.K;
    const CrfGradLists L = {rows, edge, temporal, tr};
    launch(k_crf_tensor_grad_close, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dp, L, q_start, grad_start, dm_in, grad_unaries,
           grad_q0, (int)first);
}

void launch_crf_tensor_grad_compat(const float* slots, size_t blocks, int C, float* grad_compat, hipStream_t st) {
    launch(k_crf_tensor_grad_compat, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, slots, blocks, C, grad_compat);
}

}  // namespace fslic
