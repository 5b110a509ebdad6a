// attend.hip -- attention over neighbour lists, gfx950 (fast_slic_amd/attention.py states the rules; layout, checks and the launch
// shapes are attend.h's).
//   k_attend_dot             : one thread per (head, entry); the channels of the head in ascending order, two loads, a product and an
//                              addition each, no cross-lane reduction.  Consecutive entries share their row: `a` is a broadcast
//                              within a few lanes, `b` a gather beside it, the store is coalesced.
//   k_attend_softmax<false>  : a lane owns a (row, head).  Three walks of the row: the maximum; e = crf_expf(s - m) into the place of
//                              s and the fold Z of e; e / Z.  No register holds a row, so a row may have any length.
//   k_attend_softmax<true>   : the same item; t = the fold of alpha * g, then alpha * (g - t).
//   k_attend_apply<BACK, ..> : the walk of k_aggregate<kAggSum, true, BACK> (aggregate.hip) with the weight window taken from
//                              weight + h * nnz, h the head of the wave's eight channels; two item shapes (attend.h).
// This file is compiled with -ffp-contract=off: every product, sum, difference and quotient is one IEEE float operation rounded on its
// own, and the division is HIP's correctly rounded one.  crf_expf (crf.h) writes its fused operations out with __builtin_fma, which
// that switch leaves alone: the bits of the host's crf_expf.  No atomics, and no kernel waits for another block.
#include "attend.h"
#include "aggregate.h"
#include "crf.h"
#include "launch.h"

namespace fslic {

namespace {

__global__ __launch_bounds__(256) void k_attend_dot(const int32_t* __restrict__ rows, const int32_t* __restrict__ indices, const float* __restrict__ a,
                                                    const float* __restrict__ b, float* __restrict__ out, int C, int D, uint32_t K, uint32_t R,
                                                    uint32_t nnz, uint32_t total) {
    // total = heads * nnz < 2^31, and a round of the grid is 2^19 threads: q does not wrap
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
        const uint32_t h = q / nnz, p = q - h * nnz;
        const uint32_t r = (uint32_t)rows[p], j = (uint32_t)indices[p];
        float acc = 0.0f;
        if (r < R && j < K) {
            const uint32_t f = r / K, i = r - f * K;
            const size_t head0 = ((size_t)f * (size_t)C + (size_t)h * (size_t)D) * K;      // of the head's first channel, node 0 of the frame
            const float* __restrict__ ap = a + head0 + i;
            const float* __restrict__ bp = b + head0 + j;
            for (int c = 0; c < D; ++c, ap += K, bp += K) acc = acc + *ap * *bp;
        }
        out[q] = acc;
    }
}

template <bool BACK>
__global__ __launch_bounds__(256) void k_attend_softmax(const long long* __restrict__ offsets, const int32_t* __restrict__ indices,
                                                        const float* __restrict__ in, const float* __restrict__ grad, float* out, uint32_t K,
                                                        uint32_t R, int nnz, uint32_t heads, uint32_t groups, unsigned long long items) {
    __shared__ int s_idx[kAggStage];
    __shared__ float s_a[kAttendHeads][kAggStage];                                     // scores, then e, then alpha (backward: alpha, then the gradient)
    __shared__ float s_g[BACK ? kAttendHeads : 1][BACK ? kAggStage : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x) {      // (the same trips for every thread of a block)
        const uint32_t tile = (uint32_t)(item / groups), group = (uint32_t)(item - (unsigned long long)tile * groups);
        const uint32_t row0 = tile * (uint32_t)kAggRows;                               // < R
        const uint32_t rows_end = R - row0 < (uint32_t)kAggRows ? R : row0 + (uint32_t)kAggRows;
        const uint32_t h = group * (uint32_t)kAttendHeads + wave;
        const bool active = h < heads;                                                 // the same in every lane of a wave
        const size_t hoff = (size_t)h * (size_t)nnz;                                   // (used by an active wave only)
        const int lo = row_bound(offsets, row0, nnz), hi = row_bound(offsets, rows_end, nnz);
        const int staged = nnz - lo < kAggStage ? nnz - lo : kAggStage;
        const int own = hi <= lo ? 0 : hi - lo < staged ? hi - lo : staged;            // the part of the window that belongs to this tile
        __syncthreads();                                                               // the stores of the item before are over
        for (int t = threadIdx.x; t < staged; t += 256) s_idx[t] = indices[lo + t];
        if (active) {
            for (int t = lane; t < staged; t += 64) {
                s_a[wave][t] = in[hoff + (size_t)(lo + t)];
                if (BACK) s_g[wave][t] = grad[hoff + (size_t)(lo + t)];
            }
        }
        __syncthreads();
        const uint32_t r = row0 + lane;
        if (active && r < R) {
            const int begin = row_bound(offsets, r, nnz);
            int end = row_bound(offsets, r + 1u, nnz);
            if (end < begin) end = begin;
            // (a row before the window wraps beyond it: t is unsigned)
            if (!BACK) {
                float m = -INFINITY;
                for (int pos = begin; pos < end; ++pos) {
                    const uint32_t t = (uint32_t)(pos - lo);
                    const bool win = t < (uint32_t)staged;
                    if ((uint32_t)(win ? s_idx[t] : indices[pos]) >= K) continue;
                    const float s = win ? s_a[wave][t] : in[hoff + (size_t)pos];
                    m = s > m ? s : m;
                }
                float Z = 0.0f;
                for (int pos = begin; pos < end; ++pos) {
                    const uint32_t t = (uint32_t)(pos - lo);
                    const bool win = t < (uint32_t)staged;
                    float e = 0.0f;
                    if ((uint32_t)(win ? s_idx[t] : indices[pos]) < K) {
                        e = crf_expf((win ? s_a[wave][t] : in[hoff + (size_t)pos]) - m);
                        Z = Z + e;
                    }
                    if (win) s_a[wave][t] = e;
                    else out[hoff + (size_t)pos] = e;
                }
                for (int pos = begin; pos < end; ++pos) {
                    const uint32_t t = (uint32_t)(pos - lo);
                    const bool win = t < (uint32_t)staged;
                    if ((uint32_t)(win ? s_idx[t] : indices[pos]) >= K) continue;      // (its +0.0 is written)
                    if (win) s_a[wave][t] = s_a[wave][t] / Z;
                    else out[hoff + (size_t)pos] = out[hoff + (size_t)pos] / Z;        // this lane's own store of the walk before
                }
            } else {
                float sum = 0.0f;
                for (int pos = begin; pos < end; ++pos) {
                    const uint32_t t = (uint32_t)(pos - lo);
                    const bool win = t < (uint32_t)staged;
                    if ((uint32_t)(win ? s_idx[t] : indices[pos]) >= K) continue;
                    const float al = win ? s_a[wave][t] : in[hoff + (size_t)pos], g = win ? s_g[wave][t] : grad[hoff + (size_t)pos];
                    sum = sum + al * g;
                }
                for (int pos = begin; pos < end; ++pos) {
                    const uint32_t t = (uint32_t)(pos - lo);
                    const bool win = t < (uint32_t)staged;
                    float v = 0.0f;
                    if ((uint32_t)(win ? s_idx[t] : indices[pos]) < K) {
                        const float al = win ? s_a[wave][t] : in[hoff + (size_t)pos], g = win ? s_g[wave][t] : grad[hoff + (size_t)pos];
                        v = al * (g - sum);
                    }
                    if (win) s_a[wave][t] = v;
                    else out[hoff + (size_t)pos] = v;
                }
            }
        }
        __syncthreads();                                                               // the window holds the results of the tile's rows
        if (active) {
            for (int t = lane; t < own; t += 64) out[hoff + (size_t)(lo + t)] = s_a[wave][t];
            // entries that lie in no row are not valid: +0.0 in front of the first row and behind the last one
            if (tile == 0u)
                for (int p = lane; p < lo; p += 64) out[hoff + (size_t)p] = 0.0f;
            if (rows_end == R)
                for (int p = hi + (int)lane; p < nnz; p += 64) out[hoff + (size_t)p] = 0.0f;
        }
    }
}

// PACK: wave w of an item takes the eight-channel chunk 4 * group + w of the sequence (head, chunk of the head), with the weight
// window of its own head; otherwise an item is 32 channels of one head and the block shares one weight window.
template <bool BACK, bool PACK>
__global__ __launch_bounds__(256) void k_attend_apply(const long long* __restrict__ offsets, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
                                                      const float* __restrict__ weight, const float* __restrict__ src, float* __restrict__ dst, int C,
                                                      int D, uint32_t K, uint32_t R, int nnz, uint32_t heads, uint32_t groups,
                                                      unsigned long long items) {
    constexpr int kWaves = kAggBlockChannels / kAggWaveChannels;
    __shared__ int s_node[kAggStage];
    __shared__ int s_p[BACK ? kAggStage : 1];
    __shared__ float s_w[PACK ? kWaves : 1][kAggStage];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t slot = PACK ? wave : 0u;
    const uint32_t per_head = ((uint32_t)D + (PACK ? kAggWaveChannels : kAggBlockChannels) - 1u) / (PACK ? kAggWaveChannels : kAggBlockChannels);
    for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x) {      // (the same trips for every thread of a block)
        const uint32_t tile = (uint32_t)(item / groups), group = (uint32_t)(item - (unsigned long long)tile * groups);
        const uint32_t row0 = tile * (uint32_t)kAggRows;                               // < R
        const uint32_t part = PACK ? group * (uint32_t)kWaves + wave : group;          // of the sequence (head, part of the head)
        const uint32_t h = part / per_head;
        const bool has_head = h < heads;                                               // (a block's last waves may lie behind the last head)
        const int cend = has_head ? (int)(h + 1u) * D : 0;                             // behind the head's last channel
        const int c0 = !has_head ? 0
                                 : (int)h * D + (int)(part - h * per_head) * (PACK ? kAggWaveChannels : kAggBlockChannels) + (PACK ? 0 : (int)wave * kAggWaveChannels);
        const bool active = c0 < cend;                                                 // the same in every lane of a wave
        const size_t hoff = has_head ? (size_t)h * (size_t)nnz : 0;
        const int lo = row_bound(offsets, row0, nnz);
        const int staged = nnz - lo < kAggStage ? nnz - lo : kAggStage;
        __syncthreads();                                                               // the walks of the item before are over
        for (int t = threadIdx.x; t < staged; t += 256) {
            if (!BACK) {
                s_node[t] = ia[lo + t];
            } else {
                const int p = ia[lo + t], r = ib[lo + t];                              // t_entries, t_rows
                s_node[t] = (uint32_t)p < (uint32_t)nnz && (uint32_t)r < R ? r : -1;
                s_p[t] = p;
            }
        }
        if (BACK) __syncthreads();                                                     // the transposed window's weights are gathered through s_p
        if (PACK ? active : has_head) {
            for (int t = PACK ? lane : threadIdx.x; t < staged; t += PACK ? 64 : 256)
                s_w[slot][t] = !BACK ? weight[hoff + (size_t)(lo + t)] : s_node[t] >= 0 ? weight[hoff + (size_t)s_p[t]] : 0.0f;
        }
        __syncthreads();
        const uint32_t r = row0 + lane;
        if (!active || r >= R) continue;                                               // (no barrier below this line)
        const int begin = row_bound(offsets, r, nnz);
        int end = row_bound(offsets, r + 1u, nnz);
        if (end < begin) end = begin;
        const uint32_t f = r / K, i = r - f * K;
        const size_t cell0 = ((size_t)f * (size_t)C + (size_t)c0) * K;                 // of channel c0, node 0 of the frame
        const int base = BACK ? (int)(f * K) : 0;
        float acc[kAggWaveChannels];
#pragma unroll
        for (int q = 0; q < kAggWaveChannels; ++q) acc[q] = 0.0f;
        for (int pos = begin; pos < end; ++pos) {
            const uint32_t t = (uint32_t)(pos - lo);                                   // (a row before the window wraps beyond it)
            int node;
            float w;
            if (t < (uint32_t)staged) {
                node = s_node[t];
                w = s_w[slot][t];
            } else if (!BACK) {
                node = ia[pos];
                w = weight[hoff + (size_t)pos];
            } else {
                const int p = ia[pos], rr = ib[pos];
                const bool ok = (uint32_t)p < (uint32_t)nnz && (uint32_t)rr < R;
                node = ok ? rr : -1;
                w = ok ? weight[hoff + (size_t)p] : 0.0f;
            }
            const uint32_t j = (uint32_t)(node - base);
            if (j >= K) continue;
#pragma unroll
            for (int q = 0; q < kAggWaveChannels; ++q) {
                if (c0 + q >= cend) break;
                acc[q] = acc[q] + w * src[cell0 + (size_t)q * K + j];
            }
        }
#pragma unroll
        for (int q = 0; q < kAggWaveChannels; ++q) {
            if (c0 + q >= cend) break;
            dst[cell0 + (size_t)q * K + i] = acc[q];
        }
    }
}

}  // namespace

void launch_attend_dot(const int32_t* rows, const int32_t* indices, const float* a, const float* b, float* out, int N, int C, int K, long long nnz,
                       int heads, hipStream_t st) {
    // one (head, entry) a thread and round, with at most the 2048 blocks of 256 threads the chip holds at once (as aggregate.hip's weight kernel)
    const unsigned long long total = (unsigned long long)heads * (unsigned long long)nnz;
    const int blocks = tile_grid(total, 256);
    launch(k_attend_dot, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, rows, indices, a, b, out, C, C / heads, (uint32_t)K,
           (uint32_t)N * (uint32_t)K, (uint32_t)nnz, (uint32_t)total);
}

void launch_attend_softmax(const long long* offsets, const int32_t* indices, const float* in, const float* grad, float* out, int N, int K,
                           long long nnz, int heads, hipStream_t st) {
    const uint32_t R = (uint32_t)N * (uint32_t)K, tiles = (R + kAggRows - 1u) / kAggRows, groups = ((uint32_t)heads + kAttendHeads - 1u) / kAttendHeads;
    const unsigned long long items = (unsigned long long)tiles * groups;
    const dim3 grid((unsigned)tile_grid(items, 1)), block(256);
    if (grad) launch(k_attend_softmax<true>, grid, block, 0, st, offsets, indices, in, grad, out, (uint32_t)K, R, (int)nnz, (uint32_t)heads, groups, items);
    else launch(k_attend_softmax<false>, grid, block, 0, st, offsets, indices, in, grad, out, (uint32_t)K, R, (int)nnz, (uint32_t)heads, groups, items);
}

void launch_attend_apply(bool transposed, const long long* offsets, const int32_t* ia, const int32_t* ib, const float* weight, const float* src,
                         float* dst, int N, int C, int K, long long nnz, int heads, hipStream_t st) {
    const int D = C / heads;
    const bool pack = attend_pack(D);
    const int part = pack ? kAggWaveChannels : kAggBlockChannels;
    const uint32_t R = (uint32_t)N * (uint32_t)K, tiles = (R + kAggRows - 1u) / kAggRows;
    const unsigned long long parts = (unsigned long long)heads * (unsigned long long)((D + part - 1) / part);      // <= C
    const uint32_t groups = (uint32_t)(pack ? (parts + 3ull) / 4ull : parts);
    const unsigned long long items = (unsigned long long)tiles * groups;
    const dim3 grid((unsigned)tile_grid(items, 1)), block(256);
#define FSLIC_ATTEND(BACK, PACK)                                                                                                         \
    launch(k_attend_apply<BACK, PACK>, grid, block, 0, st, offsets, ia, ib, weight, src, dst, C, D, (uint32_t)K, R, (int)nnz, (uint32_t)heads, groups, items)
    if (transposed && pack) FSLIC_ATTEND(true, true);
    else if (transposed) FSLIC_ATTEND(true, false);
    else if (pack) FSLIC_ATTEND(false, true);
    else FSLIC_ATTEND(false, false);
#undef FSLIC_ATTEND
}

}  // namespace fslic
