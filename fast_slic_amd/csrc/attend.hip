// attend.hip -- attention over neighbour lists, gfx950 (fast_slic_amd/attention.py states the rules; layout, checks, the tile and its
// walk are lists.h's, the launch shapes attend.h's).
//   k_attend_dot             : one thread per (head, entry); the channels of the head in ascending order, two loads, a product and an
//                              addition each, no cross-lane reduction.  Consecutive entries share their row: `a` is a broadcast
//                              within a few lanes, `b` a gather beside it, the store is coalesced.  At one head also the gradient of
//                              graph_aggregate's weight.
//   k_attend_softmax<false>  : a lane owns a (row, head).  Three walks of the row: the maximum; e = crf_expf(s - m) into the place of
//                              s and the fold Z of e; e / Z.  No register holds a row, so a row may have any length.
//   k_attend_softmax<true>   : the same item; t = the fold of alpha * g, then alpha * (g - t).
//   k_attend_apply<BACK, ..> : a lane owns a row and eight channels and folds weight[h][p] * x over the row's valid positions, the
//                              weight window taken from weight + h * nnz, h the head of the wave's eight channels; two item shapes
//                              (attend.h).  <.., false> at one head is graph_aggregate's weighted sum.
// This file is compiled with -ffp-contract=off: every product, sum, difference and quotient is one IEEE float operation rounded on its
// own, and the division is HIP's correctly rounded one.  crf_expf (crf.h) writes its fused operations out with __builtin_fma, which
// that switch leaves alone: the bits of the host's crf_expf.  No atomics, and no kernel waits for another block.
#include "attend.h"
#include "crf.h"

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
        const ListTile T = list_tile(item, groups, offsets, nnz);
        const ListTileOwn own = list_tile_own(T, offsets, R, nnz);
        const uint32_t h = T.group * (uint32_t)kAttendHeads + wave;
        const bool active = h < heads;                                                 // the same in every lane of a wave
        const size_t hoff = (size_t)h * (size_t)nnz;                                   // (used by an active wave only)
        __syncthreads();                                                               // the stores of the item before are over
        list_stage<false, false>(T, indices, nullptr, R, nnz, (LdsInt*)s_idx, nullptr);
        if (active) {
            list_stage_floats<false>(T, in + hoff, nullptr, (LdsFloat*)s_a[wave], lane);
            if (BACK) list_stage_floats<false>(T, grad + hoff, nullptr, (LdsFloat*)s_g[wave], lane);
        }
        __syncthreads();
        const uint32_t r = T.row0 + lane;
        if (active && r < R) {
            const ListRow row = list_row(offsets, r, K, nnz);
            // a position's value and its result live in the window, or in global memory beyond it
            LdsFloat* const a_win = (LdsFloat*)s_a[wave];                              // (with their address space: lists.h)
            const LdsFloat* const g_win = (const LdsFloat*)s_g[BACK ? wave : 0u];
            const auto at = [&](int pos) { return list_at<false, false>(T, row, pos, indices, nullptr, K, R, nnz, (LdsInt*)s_idx, nullptr); };
            const auto get = [&](const LdsFloat* w, const float* g, const ListPos& e, int pos) { return e.win ? w[e.t] : g[hoff + (size_t)pos]; };
            const auto put = [&](const ListPos& e, int pos, float v) {
                if (e.win) a_win[e.t] = v;
                else out[hoff + (size_t)pos] = v;
            };
            if (!BACK) {
                float m = -INFINITY, Z = 0.0f;
                for (int pos = row.begin; pos < row.end; ++pos) {
                    const ListPos e = at(pos);
                    if (!e.valid) continue;
                    const float s = get(a_win, in, e, pos);
                    m = s > m ? s : m;
                }
                for (int pos = row.begin; pos < row.end; ++pos) {
                    const ListPos e = at(pos);
                    float v = 0.0f;
                    if (e.valid) {
                        v = crf_expf(get(a_win, in, e, pos) - m);
                        Z = Z + v;
                    }
                    put(e, pos, v);
                }
                for (int pos = row.begin; pos < row.end; ++pos) {
                    const ListPos e = at(pos);
                    if (e.valid) put(e, pos, get(a_win, out, e, pos) / Z);         // (the +0.0 of the others is written; beyond the window: this lane's own store)
                }
            } else {
                float sum = 0.0f;
                for (int pos = row.begin; pos < row.end; ++pos) {
                    const ListPos e = at(pos);
                    if (e.valid) sum = sum + get(a_win, in, e, pos) * get(g_win, grad, e, pos);
                }
                for (int pos = row.begin; pos < row.end; ++pos) {
                    const ListPos e = at(pos);
                    put(e, pos, e.valid ? get(a_win, in, e, pos) * (get(g_win, grad, e, pos) - sum) : 0.0f);
                }
            }
        }
        __syncthreads();                                                               // the window holds the results of the tile's rows
        if (active) {
            for (int t = lane; t < own.own; t += 64) out[hoff + (size_t)(T.lo + t)] = s_a[wave][t];
            // entries that lie in no row are not valid: +0.0 in front of the first row and behind the last one
            if (T.tile == 0u)
                for (int p = lane; p < T.lo; p += 64) out[hoff + (size_t)p] = 0.0f;
            if (own.rows_end == R)
                for (int p = own.hi + (int)lane; p < nnz; p += 64) out[hoff + (size_t)p] = 0.0f;
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
        const ListTile T = list_tile(item, groups, offsets, nnz);
        const uint32_t part = PACK ? T.group * (uint32_t)kWaves + wave : T.group;      // of the sequence (head, part of the head)
        const uint32_t h = part / per_head;
        const bool has_head = h < heads;                                               // (a block's last waves may lie behind the last head)
        const int cend = has_head ? (int)(h + 1u) * D : 0;                             // behind the head's last channel
        const int c0 = !has_head ? 0
                                 : (int)h * D + (int)(part - h * per_head) * (PACK ? kAggWaveChannels : kAggBlockChannels) + (PACK ? 0 : (int)wave * kAggWaveChannels);
        const bool active = c0 < cend;                                                 // the same in every lane of a wave
        const size_t hoff = has_head ? (size_t)h * (size_t)nnz : 0;
        __syncthreads();                                                               // the walks of the item before are over
        if (PACK) {
            list_stage<BACK, BACK>(T, ia, ib, R, nnz, (LdsInt*)s_node, (LdsInt*)s_p);
            if (BACK) __syncthreads();                                                 // the transposed window's weights are gathered through s_p
            if (active) list_stage_floats<BACK>(T, weight + hoff, (LdsInt*)s_p, (LdsFloat*)s_w[wave], lane);
        } else {
            list_stage<BACK, BACK, true>(T, ia, ib, R, nnz, (LdsInt*)s_node, (LdsInt*)s_p, weight + hoff, (LdsFloat*)s_w[0]);      // (hoff = 0 behind the last head: staged, not used)
        }
        __syncthreads();
        const uint32_t r = T.row0 + lane;
        if (!active || r >= R) continue;                                               // (no barrier below this line)
        const ListRow row = list_row(offsets, r, K, nnz);
        const size_t cell0 = ((size_t)row.f * (size_t)C + (size_t)c0) * K;             // of channel c0, node 0 of the frame
        float acc[kAggWaveChannels];
#pragma unroll
        for (int q = 0; q < kAggWaveChannels; ++q) acc[q] = 0.0f;
        for (int pos = row.begin; pos < row.end; ++pos) {
            const ListPos e = list_at<BACK, BACK>(T, row, pos, ia, ib, K, R, nnz, (LdsInt*)s_node, (LdsInt*)s_p);
            if (!e.valid) continue;
            const float w = e.win ? ((const LdsFloat*)s_w[slot])[e.t] : weight[hoff + (size_t)e.p];      // (a ds_read or a global_load: lists.h)
#pragma unroll
            for (int q = 0; q < kAggWaveChannels; ++q) {
                if (c0 + q >= cend) break;
                acc[q] = acc[q] + w * src[cell0 + (size_t)q * K + e.j];
            }
        }
#pragma unroll
        for (int q = 0; q < kAggWaveChannels; ++q) {
            if (c0 + q >= cend) break;
            dst[cell0 + (size_t)q * K + row.i] = acc[q];
        }
    }
}

}  // namespace

void launch_attend_dot(const int32_t* rows, const int32_t* indices, const float* a, const float* b, float* out, int N, int C, int K, long long nnz,
                       int heads, hipStream_t st) {
    const unsigned long long total = (unsigned long long)heads * (unsigned long long)nnz;      // one (head, entry) a thread and round
    launch(k_attend_dot, entry_grid(total), dim3(256), 0, st, rows, indices, a, b, out, C, C / heads, (uint32_t)K, (uint32_t)N * (uint32_t)K,
           (uint32_t)nnz, (uint32_t)total);
}

void launch_attend_softmax(const long long* offsets, const int32_t* indices, const float* in, const float* grad, float* out, int N, int K,
                           long long nnz, int heads, hipStream_t st) {
    const ListLaunch g = list_launch(N, K, ((uint32_t)heads + kAttendHeads - 1u) / kAttendHeads);
    launch(grad ? k_attend_softmax<true> : k_attend_softmax<false>, g.grid, dim3(256), 0, st, offsets, indices, in, grad, out, (uint32_t)K, g.R, (int)nnz,
           (uint32_t)heads, g.groups, g.items);
}

void launch_attend_apply(bool transposed, bool pack, const long long* offsets, const int32_t* ia, const int32_t* ib, const float* weight,
                         const float* src, float* dst, int N, int C, int K, long long nnz, int heads, hipStream_t st) {
    const int D = C / heads, part = pack ? kAggWaveChannels : kAggBlockChannels;
    const unsigned long long parts = (unsigned long long)heads * (unsigned long long)((D + part - 1) / part);      // <= C
    const ListLaunch g = list_launch(N, K, (uint32_t)(pack ? (parts + 3ull) / 4ull : parts));
    const auto kernel = transposed ? (pack ? k_attend_apply<true, true> : k_attend_apply<true, false>)
                                   : (pack ? k_attend_apply<false, true> : k_attend_apply<false, false>);
    launch(kernel, g.grid, dim3(256), 0, st, offsets, ia, ib, weight, src, dst, C, D, (uint32_t)K, g.R, (int)nnz, (uint32_t)heads, g.groups, g.items);
}

}  // namespace fslic
