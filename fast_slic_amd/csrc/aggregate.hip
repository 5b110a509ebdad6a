// aggregate.hip -- aggregation of node features over neighbour lists, gfx950 (fast_slic_amd/propagate.py states the rules; layout,
// checks and the launch shape are aggregate.h's).
//   k_aggregate<MODE, HAS_W, false> : forward.  A lane owns a row (frame, node) and eight channels; it walks the row's entries in
//                                     ascending order and folds weight[p] * x[indices[p]] (sum), x (mean, then one division by the
//                                     count of valid entries), or keeps the first largest x and its entry (max).
//   k_aggregate<MODE, HAS_W, true>  : backward to the values.  The same walk over the transposed lists: a lane owns a target and folds
//                                     weight[p] * g[row(p)] (sum), g[row(p)] / float(degree[row(p)]) (mean), or g[row(p)] where
//                                     argmax[row(p)] == p (max).  The gather of the forward becomes a gather again: no atomics.
//   k_aggregate_backward_weight     : one thread per entry, the channels in ascending order, no cross-lane reduction.
// This file is compiled with -ffp-contract=off: a product and the addition behind it are two IEEE float operations, each rounded on
// its own, and the division is HIP's correctly rounded one, which is what the numpy model of the tests reproduces bit for bit.
// Lanes run along the nodes, K innermost: the loads of a row's own cells and every store are coalesced, and the gathers of a SLIC
// graph land in the few cache lines around the node.  No kernel waits for another block.
#include "aggregate.h"
#include "launch.h"

namespace fslic {

namespace {

// One position of the lists as the walk takes it: `node` is the neighbour (forward) or the row over (frame, node) of the entry
// (backward; -1 for an entry or a row outside its range), `p` the entry, `w` the weight of p, or float(degree[row]) for the mean's
// backward.  pos is inside [0, nnz).
struct AggEntry {
    int node, p;
    float w;
};
template <int MODE, bool HAS_W, bool BACK>
__device__ __forceinline__ AggEntry load_entry(int pos, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib, const float* __restrict__ weight,
                                               const int32_t* __restrict__ degree, uint32_t R, int nnz) {
    AggEntry e;
    e.w = 1.0f;
    if (!BACK) {
        e.node = ia[pos];
        e.p = pos;
        if (HAS_W) e.w = weight[pos];
    } else {
        e.p = ia[pos];                                                         // t_entries
        const int r = ib[pos];                                                 // t_rows
        const bool ok = (uint32_t)e.p < (uint32_t)nnz && (uint32_t)r < R;
        e.node = ok ? r : -1;
        if (HAS_W) e.w = ok ? weight[e.p] : 0.0f;
        if (MODE == kAggMean) e.w = ok ? (float)degree[r] : 1.0f;
    }
    return e;
}

template <int MODE, bool HAS_W, bool BACK>
__global__ __launch_bounds__(256) void k_aggregate(const long long* __restrict__ offsets, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
                                                   const float* __restrict__ weight, const float* __restrict__ src, float* __restrict__ dst,
                                                   int32_t* argmax, int32_t* degree, int C, uint32_t K, uint32_t R, int nnz, uint32_t groups,
                                                   unsigned long long items) {
    constexpr bool kUseW = HAS_W || (BACK && MODE == kAggMean), kUseP = BACK && MODE == kAggMax;
    __shared__ int s_node[kAggStage];
    __shared__ float s_w[kUseW ? kAggStage : 1];
    __shared__ int s_p[kUseP ? kAggStage : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x) {      // (the same trips for every thread of a block)
        const uint32_t tile = (uint32_t)(item / groups), group = (uint32_t)(item - (unsigned long long)tile * groups);
        const uint32_t row0 = tile * (uint32_t)kAggRows;                               // < R
        const int lo = row_bound(offsets, row0, nnz);
        const int staged = nnz - lo < kAggStage ? nnz - lo : kAggStage;
        __syncthreads();                                                               // the walks of the item before are over
        for (int t = threadIdx.x; t < staged; t += 256) {
            const AggEntry e = load_entry<MODE, HAS_W, BACK>(lo + t, ia, ib, weight, degree, R, nnz);
            s_node[t] = e.node;
            if (kUseW) s_w[t] = e.w;
            if (kUseP) s_p[t] = e.p;
        }
        __syncthreads();
        const uint32_t r = row0 + lane;
        if (r >= R) continue;                                                          // (no barrier below this line)
        const int begin = row_bound(offsets, r, nnz);
        int end = row_bound(offsets, r + 1u, nnz);
        if (end < begin) end = begin;
        const uint32_t f = r / K, i = r - f * K;
        const int c0 = (int)group * kAggBlockChannels + (int)wave * kAggWaveChannels;  // the same in every lane of a wave
        const size_t cell0 = ((size_t)f * (size_t)C + (size_t)c0) * K;                 // of channel c0, node 0 of the frame
        const int base = BACK ? (int)(f * K) : 0;
        float acc[kAggWaveChannels];
        int arg[kAggWaveChannels];
#pragma unroll
        for (int q = 0; q < kAggWaveChannels; ++q) acc[q] = 0.0f, arg[q] = -1;
        int d = 0;
        for (int pos = begin; pos < end; ++pos) {
            const uint32_t t = (uint32_t)(pos - lo);                                   // (a row before the window wraps beyond it)
            AggEntry e;
            if (t < (uint32_t)staged) {
                e.node = s_node[t];
                e.w = kUseW ? s_w[t] : 1.0f;
                e.p = kUseP ? s_p[t] : pos;
            } else {
                e = load_entry<MODE, HAS_W, BACK>(pos, ia, ib, weight, degree, R, nnz);
            }
            const uint32_t j = (uint32_t)(e.node - base);
            if (j >= K) continue;
            ++d;
#pragma unroll
            for (int q = 0; q < kAggWaveChannels; ++q) {
                if (c0 + q >= C) break;
                const size_t cell = cell0 + (size_t)q * K + j;
                const float v = src[cell];
                if (MODE == kAggSum) {
                    acc[q] = acc[q] + (HAS_W ? e.w * v : v);
                } else if (MODE == kAggMean) {
                    acc[q] = acc[q] + (BACK ? v / e.w : v);
                } else if (!BACK) {
                    if (arg[q] < 0 || v > acc[q]) acc[q] = v, arg[q] = e.p;
                } else if (argmax[cell] == e.p) {
                    acc[q] = acc[q] + v;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kAggWaveChannels; ++q) {
            if (c0 + q >= C) break;
            const size_t cell = cell0 + (size_t)q * K + i;
            dst[cell] = MODE == kAggMean && !BACK ? (d > 0 ? acc[q] / (float)d : 0.0f) : acc[q];
            if (MODE == kAggMax && !BACK) argmax[cell] = arg[q];
        }
        if (MODE == kAggMean && !BACK && c0 == 0) degree[r] = d;
    }
}

__global__ __launch_bounds__(256) void k_aggregate_backward_weight(const int32_t* __restrict__ rows, const int32_t* __restrict__ indices,
                                                                   const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ gw,
                                                                   int C, uint32_t K, uint32_t R, int nnz) {
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < (long long)nnz; p += (long long)gridDim.x * 256) {
        const uint32_t r = (uint32_t)rows[p], j = (uint32_t)indices[p];
        float acc = 0.0f;
        if (r < R && j < K) {
            const uint32_t f = r / K, i = r - f * K;
            const float* __restrict__ xp = x + (size_t)f * (size_t)C * K + j;
            const float* __restrict__ gp = g + (size_t)f * (size_t)C * K + i;
            for (int c = 0; c < C; ++c, xp += K, gp += K) acc = acc + *xp * *gp;
        }
        gw[p] = acc;
    }
}

template <bool BACK>
void launch_lists(int reduce, const long long* offsets, const int32_t* ia, const int32_t* ib, const float* weight, const float* src, float* dst,
                  int32_t* argmax, int32_t* degree, int N, int C, int K, long long nnz, hipStream_t st) {
    const uint32_t R = (uint32_t)N * (uint32_t)K, tiles = (R + kAggRows - 1u) / kAggRows, groups = ((uint32_t)C + kAggBlockChannels - 1u) / kAggBlockChannels;
    const unsigned long long items = (unsigned long long)tiles * groups;
    const dim3 grid((unsigned)tile_grid(items, 1)), block(256);
#define FSLIC_AGG(MODE, HAS_W)                                                                                                           \
    launch(k_aggregate<MODE, HAS_W, BACK>, grid, block, 0, st, offsets, ia, ib, weight, src, dst, argmax, degree, C, (uint32_t)K, R, (int)nnz, groups, items)
    if (reduce == kAggMean) FSLIC_AGG(kAggMean, false);
    else if (reduce == kAggMax) FSLIC_AGG(kAggMax, false);
    else if (weight) FSLIC_AGG(kAggSum, true);
    else FSLIC_AGG(kAggSum, false);
#undef FSLIC_AGG
}

}  // namespace

void launch_aggregate_forward(int reduce, const long long* offsets, const int32_t* indices, const float* weight, const float* values, float* out,
                              int32_t* argmax, int32_t* degree, int N, int C, int K, long long nnz, hipStream_t st) {
    launch_lists<false>(reduce, offsets, indices, nullptr, weight, values, out, argmax, degree, N, C, K, nnz, st);
}

void launch_aggregate_backward_values(int reduce, const long long* t_offsets, const int32_t* t_entries, const int32_t* t_rows, const float* weight,
                                      const int32_t* argmax, const int32_t* degree, const float* grad_out, float* grad_values, int N, int C, int K,
                                      long long nnz, hipStream_t st) {
    launch_lists<true>(reduce, t_offsets, t_entries, t_rows, weight, grad_out, grad_values, const_cast<int32_t*>(argmax), const_cast<int32_t*>(degree),
                       N, C, K, nnz, st);
}

void launch_aggregate_backward_weight(const int32_t* rows, const int32_t* indices, const float* values, const float* grad_out, float* grad_weight,
                                      int N, int C, int K, long long nnz, hipStream_t st) {
    // one entry a thread and round, with at most the 2048 blocks of 256 threads the chip holds at once (as region.hip's edge kernel)
    const int blocks = tile_grid((unsigned long long)nnz, 256);
    launch(k_aggregate_backward_weight, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, rows, indices, values, grad_out, grad_weight,
           C, (uint32_t)K, (uint32_t)N * (uint32_t)K, (int)nnz);
}

}  // namespace fslic
