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
// The gradients of the energies and of the seven params:
//   k_crf_tensor_energy_grad one launch behind each k_crf_tensor_sweep_bwd launch.  One thread per neighbour entry, named by its
//                            position in the transposed lists (a permutation of the entries, checked as crf_grad_gather checks it):
//                            ge[k] += f_k sum_c dm[row(k),c] q[j_k,c]; behind them one thread per (frame, node):
//                            gl[n,0,i] += f_prev sum_c dm[n,c,i] q[n-1,c,i] and gl[n,1,i] likewise with n + 1.  Classes in ascending
//                            order, the sweeps last to first, the cells zeroed on the stream before the first launch.  Neighbouring
//                            threads share their target, so q[j_k,c] is one address per run and dm a gather.  A thread per
//                            (frame, node) walking its row, the first design, had 25 wavefronts at K = 1600 and took longer
//                            than the sweep's adjoint itself.
//   k_crf_tensor_param_grad  the energies' backward: one thread per (frame, node) over its row and its two links, every term formed in
//                            double from the float inputs and added in entry order; a butterfly over the wavefront (every lane the same
//                            fixed order), lane 0 of each wavefront into LDS, one thread per name adding the four wavefronts in
//                            ascending order into the block's slot row of seven doubles.
//   k_crf_tensor_param_grad_close  one thread per name: the slot rows in ascending block order, in double, stored as float.
// Determinism: no atomics.  Every output cell and every slot has one owner thread, every sum one fixed order: du and dm belong to
// thread (node, class), a slot to lane 0 of the wavefront of (block, class) after the fixed-order wave_reduce_add, the launches of a
// call follow each other on one stream.  That is why G is a gather over the transposed lists and not a scatter.
// Memory safety with a CSR that is not one: the transposed bounds are clamped as the forward clamps a row's; a transposed entry
// counts only when its source row is a node of the gathering frame, the entry number lies inside that row's clamped bounds in `rows`
// (so it is below nnz and edge[] of it was written by k_crf_tensor_edges), and the entry is live.
// Every grid is exact (one trip), as the forward's.
#include "crf_tensor_grad.h"
#include "crf_tensor_sweep.h"
#include "device_common.h"

// The recomputed message, exponential and sum must be the forward's bits: the same operations under the same contraction rule.
#pragma clang fp contract(off)

namespace fslic {

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

// The second plane holds the exponentials, then G' q', then da: LDS, or the workspace's x above kCrfTensorLdsClasses classes
// (crf_tensor_sweep.h).
template <bool LDS>
__global__ __launch_bounds__(kCrfTensorNodes * kCrfTensorWaves) void k_crf_tensor_sweep_bwd(
        CrfTensorParams dp, CrfGradLists L, const int32_t* __restrict__ idx, const float* __restrict__ unary,
        const float* __restrict__ compat, const float* __restrict__ q_in, const float* __restrict__ q_new,
        const float* __restrict__ grad_new, const float* __restrict__ dm_in, float* __restrict__ dm_out, float* __restrict__ du,
        float* __restrict__ slots, float* msg, float* xpl, int first) {
    extern __shared__ float s_crf_grad[];
    const int C = dp.C, K = dp.K;
    const CrfSweepThread t = crf_sweep_thread<LDS>(dp, s_crf_grad, msg, xpl);

    // G' of every class of the slice into the thread's own cells of dm_out; then the forward's message, exponential and sum
    if (t.live) {
        const uint2 r = L.rows[(size_t)t.w * K + t.i];
        const float4 tl = L.temporal[(size_t)t.w * K + t.i];
        const uint2 tb = grad_new ? make_uint2(0u, 0u) : crf_clamped_bounds(L.tr.offsets, (size_t)t.w * K + t.i, dp.nnz);
        for (int cls = t.wave; cls < C; cls += t.waves) {
            const size_t cell = t.base + (size_t)cls * K + t.i;
            dm_out[cell] = grad_new ? grad_new[cell] : crf_grad_gather(dp, L, dm_in, tb, t.w, t.i, cls);
            t.m[cls * t.stride] = crf_sweep_message(t, K, r, tl, idx, L.edge, q_in, cls);
        }
    }
    __syncthreads();
    if (t.live)
        for (int cls = t.wave; cls < C; cls += t.waves) t.x[cls * t.stride] = crf_sweep_exp(t, C, K, compat, unary, cls);
    __syncthreads();
    // the forward's own clamp decision: where it clamped, the sum was a constant
    const bool clamped = t.live && crf_sweep_clamps(crf_sweep_class_sum(t, C));
    __syncthreads();                                                           // every sum is taken before the plane is reused
    if (t.live)
        for (int cls = t.wave; cls < C; cls += t.waves) {
            const size_t cell = t.base + (size_t)cls * K + t.i;
            t.x[cls * t.stride] = dm_out[cell] * q_new[cell];
        }
    __syncthreads();
    float d = 0.0f;
    if (t.live && !clamped)
        for (int cls = 0; cls < C; ++cls) d += t.x[cls * t.stride];
    __syncthreads();
    if (t.live)
        for (int cls = t.wave; cls < C; cls += t.waves) {
            const size_t cell = t.base + (size_t)cls * K + t.i;
            const float da = -q_new[cell] * (dm_out[cell] - d);
            t.x[cls * t.stride] = da;
            du[cell] = first ? da : du[cell] + da;
        }
    __syncthreads();
    // S over the other classes in ascending order; dm; the block's part of dcompat (the loop is uniform over the wavefront)
    float* slot = slots ? slots + (size_t)blockIdx.x * C : nullptr;
    for (int cls = t.wave; cls < C; cls += t.waves) {
        float S = 0.0f, part = 0.0f;
        if (t.live) {
            for (int o = 0; o < cls; ++o) S += t.x[o * t.stride];
            for (int o = cls + 1; o < C; ++o) S += t.x[o * t.stride];
            dm_out[t.base + (size_t)cls * K + t.i] = compat[cls] * S;
            if (slot) part = t.m[cls * t.stride] * S;
        }
        if (slot) {
            const float total = wave_reduce_add<float>(part);
            if (t.lane == 0) slot[cls] = first ? total : slot[cls] + total;
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
    const float G = grad_start ? grad_start[p]
                               : crf_grad_gather(dp, L, dm_in, crf_clamped_bounds(L.tr.offsets, (size_t)w * K + i, dp.nnz), w, i, cls);
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

// The sum over the classes of dm[w, c, i] * q[c * K] in ascending order: d = dm + w * C * K + i, q the other node's column.
static __device__ __forceinline__ float crf_class_dot(const float* __restrict__ d, const float* __restrict__ q, int C, int K) {
    float s = 0.0f;
    for (int c = 0; c < C; ++c) s = __builtin_fmaf(d[(size_t)c * K], q[(size_t)c * K], s);
    return s;
}

__global__ __launch_bounds__(256) void k_crf_tensor_energy_grad(CrfTensorParams dp, CrfGradLists L, const int32_t* __restrict__ idx,
                                                                const float* __restrict__ dm, const float* __restrict__ q_in,
                                                                float* __restrict__ ge, float* __restrict__ gl, uint32_t entries) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const int C = dp.C, K = dp.K;
    const uint32_t n = (uint32_t)dp.N * (uint32_t)K;
    const size_t CK = (size_t)C * K;
    if (p < entries) {
        // one neighbour entry, named by position p of the transposed lists (a permutation of the entries): the check of crf_grad_gather
        const uint32_t row = (uint32_t)L.tr.rows[p];
        if (row >= n) return;                                                  // behind the last row
        const uint32_t k = (uint32_t)L.tr.entries[p];
        const uint2 r = L.rows[row];
        if (k < r.x || k >= r.y) return;                                       // r.y <= nnz: edge[k], idx[k] and ge[k] exist
        const float2 es = L.edge[k];
        if (es.y == kCrfDeadEntry) return;                                     // idx[k] is outside [0, K): its gradient stays 0.0
        const uint32_t w = row / (uint32_t)K, i = row - w * (uint32_t)K;
        ge[k] += es.y * crf_class_dot(dm + (size_t)w * CK + i, q_in + (size_t)w * CK + idx[k], C, K);
        return;
    }
    const uint32_t g = p - entries;                                            // one (frame, node): its two link cells
    if (g >= n || !gl || !dp.temporal) return;
    const int w = (int)(g / (uint32_t)K), i = (int)(g - (uint32_t)w * (uint32_t)K);
    const float* d = dm + (size_t)w * CK + i;
    const float* q = q_in + (size_t)w * CK + i;
    const float4 t = L.temporal[g];
    const size_t link = ((size_t)w * 2) * K + i;
    if (w > 0) gl[link] += t.y * crf_class_dot(d, q - (ptrdiff_t)CK, C, K);
    if (w < dp.N - 1) gl[link + K] += t.w * crf_class_dot(d, q + CK, C, K);
}

// The sum over the wavefront in every lane: a butterfly, so each lane adds the same pairs in the same order.
static __device__ __forceinline__ double crf_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(kCrfParamGradBlock) void k_crf_tensor_param_grad(
        CrfTensorParams dp, const float* __restrict__ params, const float* __restrict__ yxrgb, const int64_t* __restrict__ offsets,
        const int32_t* __restrict__ idx, const float* __restrict__ ge, const float* __restrict__ gl, double* __restrict__ slots) {
    __shared__ double s_part[kCrfParamGradBlock / 64][kCrfParamCount];
    const int n = dp.N * dp.K;
    const int g = blockIdx.x * kCrfParamGradBlock + threadIdx.x;
    double acc[kCrfParamCount] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};         // in the order of fslic_crf_params
    if (g < n) {
        const int K = dp.K;
        const int w = g / K, i = g - w * K;
        const float* planes = yxrgb + (size_t)w * 5 * K;
        const double yi = planes[i], xi = planes[K + i], ri = planes[2 * (size_t)K + i], gi = planes[3 * (size_t)K + i], bi = planes[4 * (size_t)K + i];
        if (ge) {
            const double sw = params[0], srgb = params[2], sxy = params[4], ssw = params[5], ssxy = params[6];
            const uint2 r = crf_clamped_bounds(offsets, (size_t)g, dp.nnz);
            for (uint32_t k = r.x; k < r.y; ++k) {
                const int32_t j = idx[k];
                if ((uint32_t)j >= (uint32_t)K || j == i) continue;            // a dead entry, a self-loop: the energy is the constant 0
                const double dy = yi - (double)planes[j], dx = xi - (double)planes[K + j];
                const double dr = ri - (double)planes[2 * (size_t)K + j], dg = gi - (double)planes[3 * (size_t)K + j], db = bi - (double)planes[4 * (size_t)K + j];
                const double Drgb = dr * dr + dg * dg + db * db, Dxy = dx * dx + dy * dy;
                const double E1 = exp(-(Drgb / (srgb * srgb) + Dxy / (sxy * sxy)) * 0.5), E2 = exp(-(Dxy / (ssxy * ssxy)) * 0.5);
                const double up = ge[k];
                acc[0] += up * E1;
                acc[2] += up * (sw * E1 * Drgb / (srgb * srgb * srgb));
                acc[4] += up * (sw * E1 * Dxy / (sxy * sxy * sxy));
                acc[5] += up * E2;
                acc[6] += up * (ssw * E2 * Dxy / (ssxy * ssxy * ssxy));
            }
        }
        if (gl && dp.temporal) {
            const double tw = params[1], tsrgb = params[3];
            const size_t link = ((size_t)w * 2) * K + i;
            for (int side = 0; side < 2; ++side) {                             // towards w - 1, then towards w + 1
                if (side == 0 ? w == 0 : w == dp.N - 1) continue;
                const float* other = side == 0 ? planes - (size_t)5 * K : planes + (size_t)5 * K;
                const double dr = ri - (double)other[2 * (size_t)K + i], dg = gi - (double)other[3 * (size_t)K + i], db = bi - (double)other[4 * (size_t)K + i];
                const double Drgb = dr * dr + dg * dg + db * db;
                const double Et = exp(-(Drgb / (tsrgb * tsrgb)) * 0.5);
                const double up = gl[link + (size_t)side * K];
                acc[1] += up * Et;
                acc[3] += up * (tw * Et * Drgb / (tsrgb * tsrgb * tsrgb));
            }
        }
    }
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    for (int p = 0; p < kCrfParamCount; ++p) {
        const double total = crf_wave_sum(acc[p]);
        if (lane == 0) s_part[wave][p] = total;
    }
    __syncthreads();
    if (threadIdx.x < kCrfParamCount) {
        double s = 0.0;
        for (int v = 0; v < kCrfParamGradBlock / 64; ++v) s += s_part[v][threadIdx.x];
        slots[(size_t)blockIdx.x * kCrfParamCount + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void k_crf_tensor_param_grad_close(const double* __restrict__ slots, size_t blocks, float* __restrict__ out) {
    if (threadIdx.x >= kCrfParamCount) return;
    double s = 0.0;
    for (size_t b = 0; b < blocks; ++b) s += slots[b * kCrfParamCount + threadIdx.x];
    out[threadIdx.x] = (float)s;
}

void launch_crf_tensor_energy_grad(const CrfTensorParams& dp, const CrfGradLists& lists, const int32_t* indices, const float* dm,
                                   const float* q_in, float* grad_edge, float* grad_links, hipStream_t st) {
    // one thread per neighbour entry (none without grad_edge), then one per (frame, node) for the links; below 2^32 because nnz and N * K are below 2^31
    const uint32_t entries = grad_edge ? (uint32_t)dp.nnz : 0u;
    const uint32_t n = entries + (grad_links && dp.temporal ? (uint32_t)dp.N * (uint32_t)dp.K : 0u);
    if (n == 0) return;
    launch(k_crf_tensor_energy_grad, dim3((n + 255) / 256), dim3(256), 0, st, dp, lists, indices, dm, q_in, grad_edge, grad_links, entries);
}

void launch_crf_tensor_param_grad(const CrfTensorParams& dp, const float* params, const float* yxrgb, const int64_t* offsets,
                                  const int32_t* indices, const float* grad_edge, const float* grad_links, double* slots,
                                  float* grad_params, hipStream_t st) {
    const size_t blocks = crf_tensor_param_grad_blocks(dp.N, dp.K);
    launch(k_crf_tensor_param_grad, dim3((unsigned)blocks), dim3(kCrfParamGradBlock), 0, st, dp, params, yxrgb, offsets, indices, grad_edge,
           grad_links, slots);
    launch(k_crf_tensor_param_grad_close, dim3(1), dim3(64), 0, st, (const double*)slots, blocks, grad_params);
}

void launch_crf_tensor_sweep_bwd(const CrfTensorParams& dp, const CrfGradLists& lists, const int32_t* indices, const float* unaries,
                                 const float* compat, const float* q_in, const float* q_new, const float* grad_new, const float* dm_in,
                                 float* dm_out, float* grad_unaries, float* slots, float* msg, float* x, bool first, hipStream_t st) {
    const CrfSweepShape sh = crf_tensor_sweep_shape(dp.N, dp.C, dp.K);
    launch(sh.lds ? k_crf_tensor_sweep_bwd<true> : k_crf_tensor_sweep_bwd<false>, dim3(sh.grid), dim3(sh.block), sh.lds, st, dp, lists,
           indices, unaries, compat, q_in, q_new, grad_new, dm_in, dm_out, grad_unaries, slots, msg, x, (int)first);
}

void launch_crf_tensor_grad_close(const CrfTensorParams& dp, const CrfGradLists& lists, const float* q_start, const float* grad_start,
                                  const float* dm_in, float* grad_unaries, float* grad_q0, bool first, hipStream_t st) {
    const size_t n = (size_t)dp.N * dp.C * dp.K;
    launch(k_crf_tensor_grad_close, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dp, lists, q_start, grad_start, dm_in, grad_unaries,
           grad_q0, (int)first);
}

void launch_crf_tensor_grad_compat(const float* slots, size_t blocks, int C, float* grad_compat, hipStream_t st) {
    launch(k_crf_tensor_grad_compat, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, slots, blocks, C, grad_compat);
}

}  // namespace fslic
