// aggregate.hip -- aggregation of node features over neighbour lists, gfx950 (fast_slic_amd/propagate.py states the rules; layout,
// checks, the tile and its walk are lists.h's, the launch shape aggregate.h's).
//   k_aggregate<MODE, false> : forward, unweighted.  A lane owns a row (frame, node) and eight channels; it walks the row's entries in
//                              ascending order and folds x[indices[p]] (sum; mean, then one division by the count of valid entries),
//                              or keeps the first largest x and its entry (max).
//   k_aggregate<MODE, true>  : backward to the values.  The same walk over the transposed lists: a lane owns a target and folds
//                              g[row(p)] (sum), g[row(p)] / float(degree[row(p)]) (mean), or g[row(p)] where argmax[row(p)] == p
//                              (max).  The gather of the forward becomes a gather again: no atomics.
// The weighted sum, its backward to the values and its backward to the weight are attend.hip's apply and dot at one head: the same
// item, the same fold, the same bits.
// This file is compiled with -ffp-contract=off: a product and the addition behind it are two IEEE float operations, each rounded on
// its own, and the division is HIP's correctly rounded one, which is what the numpy model of the tests reproduces bit for bit.
// Lanes run along the nodes, K innermost: the loads of a row's own cells and every store are coalesced, and the gathers of a SLIC
// graph land in the few cache lines around the node.  No kernel waits for another block.
#include "aggregate.h"
#include "attend.h"

namespace fslic {

namespace {

template <int MODE, bool BACK>
__global__ __launch_bounds__(256) void k_aggregate(const long long* __restrict__ offsets, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
                                                   const float* __restrict__ src, float* __restrict__ dst, int32_t* argmax, int32_t* degree, int C,
                                                   uint32_t K, uint32_t R, int nnz, uint32_t groups, unsigned long long items) {
    constexpr bool kUseD = BACK && MODE == kAggMean, kUseP = BACK && MODE == kAggMax;
    __shared__ int s_node[kAggStage];
    __shared__ float s_d[kUseD ? kAggStage : 1];                                       // float(degree) of the position's row
    __shared__ int s_p[kUseP ? kAggStage : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x) {      // (the same trips for every thread of a block)
        const ListTile T = list_tile(item, groups, offsets, nnz);
        __syncthreads();                                                               // the walks of the item before are over
        list_stage<BACK, kUseP>(T, ia, ib, R, nnz, (LdsInt*)s_node, (LdsInt*)s_p);
        if (kUseD)                                                                     // of the places this thread staged itself: no barrier
            for (int t = threadIdx.x; t < T.staged; t += 256) s_d[t] = s_node[t] >= 0 ? (float)degree[s_node[t]] : 1.0f;
        __syncthreads();
        const uint32_t r = T.row0 + lane;
        if (r >= R) continue;                                                          // (no barrier below this line)
        const ListRow row = list_row(offsets, r, K, nnz);
        const int c0 = (int)T.group * kAggBlockChannels + (int)wave * kAggWaveChannels;  // the same in every lane of a wave
        const size_t cell0 = ((size_t)row.f * (size_t)C + (size_t)c0) * K;             // of channel c0, node 0 of the frame
        float acc[kAggWaveChannels];
        int arg[kAggWaveChannels];
#pragma unroll
        for (int q = 0; q < kAggWaveChannels; ++q) acc[q] = 0.0f, arg[q] = -1;
        int d = 0;
        for (int pos = row.begin; pos < row.end; ++pos) {
            const ListPos e = list_at<BACK, kUseP>(T, row, pos, ia, ib, K, R, nnz, (LdsInt*)s_node, (LdsInt*)s_p);
            if (!e.valid) continue;
            ++d;
            const float dr = !kUseD ? 1.0f : e.win ? s_d[e.t] : (float)degree[row.base + e.j];
#pragma unroll
            for (int q = 0; q < kAggWaveChannels; ++q) {
                if (c0 + q >= C) break;
                const size_t cell = cell0 + (size_t)q * K + e.j;
                const float v = src[cell];
                if (MODE == kAggSum) {
                    acc[q] = acc[q] + v;
                } else if (MODE == kAggMean) {
                    acc[q] = acc[q] + (BACK ? v / dr : v);
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
            const size_t cell = cell0 + (size_t)q * K + row.i;
            dst[cell] = MODE == kAggMean && !BACK ? (d > 0 ? acc[q] / (float)d : 0.0f) : acc[q];
            if (MODE == kAggMax && !BACK) argmax[cell] = arg[q];
        }
        if (MODE == kAggMean && !BACK && c0 == 0) degree[r] = d;
    }
}

template <bool BACK>
void launch_lists(int reduce, const long long* offsets, const int32_t* ia, const int32_t* ib, const float* weight, const float* src, float* dst,
                  int32_t* argmax, int32_t* degree, int N, int C, int K, long long nnz, hipStream_t st) {
    if (reduce == kAggSum && weight) return launch_attend_apply(BACK, false, offsets, ia, ib, weight, src, dst, N, C, K, nnz, 1, st);      // (the sum)
    const ListLaunch g = list_launch(N, K, ((uint32_t)C + kAggBlockChannels - 1u) / kAggBlockChannels);
#define FSLIC_AGG(MODE) \
    launch(k_aggregate<MODE, BACK>, g.grid, dim3(256), 0, st, offsets, ia, ib, src, dst, argmax, degree, C, (uint32_t)K, g.R, (int)nnz, g.groups, g.items)
    if (reduce == kAggMean) FSLIC_AGG(kAggMean);
    else if (reduce == kAggMax) FSLIC_AGG(kAggMax);
    else FSLIC_AGG(kAggSum);
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
    launch_attend_dot(rows, indices, grad_out, values, grad_weight, N, C, K, nnz, 1, st);
}

}  // namespace fslic
