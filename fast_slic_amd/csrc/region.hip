// region.hip -- the features of merged regions, gfx950 (fast_slic_amd/regions.py): the sums of node values over the groups of a
// mapping, exact and independent of the order, and the weight of every edge of a graph from the means of its two regions.
//   k_region_accumulate : one thread per (frame, channel, node); a node whose group is in [0, K2) adds its value to the group's
//                         fixed-point accumulator (fix_add of fixsum.h: one or two 64-bit integer atomics), and with channel 0 its
//                         count to the group's count (one integer atomic).
//   k_region_finalize   : one thread per (frame, channel, group): the accumulator rounded once to f32 (fix_to_float).
//   k_region_weights    : one thread per edge; the frame by merge.h's search, the two counts, then per channel two divisions, a
//                         difference, a square and an addition, in ascending channel order; a square root (mean) or the Ward factor.
// This file is compiled with -ffp-contract=off: every float operation of k_region_weights is one IEEE operation, rounded on its
// own (division and square root are HIP's correctly rounded ones), which is what the numpy model of the tests reproduces bit for bit.
// No float atomics anywhere.  No kernel waits for another block.
#include "device_common.h"
#include "fixsum.h"
#include "region.h"
#include <algorithm>

namespace fslic {

// the count of a node or a group as the atomics take it
static __device__ __forceinline__ void count_add(int32_t* p, int32_t v) { atomicAdd(p, v); }
static __device__ __forceinline__ void count_add(int64_t* p, int64_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

template <class M>
__global__ __launch_bounds__(256) void k_region_accumulate(const float* __restrict__ values, const int32_t* __restrict__ mapping, const M* __restrict__ counts,
                                                           unsigned long long* acc, M* counts_out, uint32_t C, uint32_t K, uint32_t K2,
                                                           unsigned long long total) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull, CK = (unsigned long long)C * K;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < total; i += stride) {
        const unsigned long long n = i / CK, r = i - n * CK, c = r / K, v = r - c * K;
        const uint32_t g = (uint32_t)mapping[n * K + v];                       // (-1 is above any K2)
        if (g >= K2) continue;
        fix_add(acc + (n * C + c) * (unsigned long long)kPoolLimbs * K2 + g, (size_t)K2, values[i]);
        if (counts && c == 0) count_add(counts_out + n * K2 + g, counts[n * K + v]);
    }
}

__global__ __launch_bounds__(256) void k_region_finalize(const unsigned long long* __restrict__ acc, float* __restrict__ sums, uint32_t K2,
                                                         unsigned long long total) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < total; i += stride) {
        const unsigned long long nc = i / K2, g = i - nc * K2;
        sums[i] = fix_to_float(acc + nc * (unsigned long long)kPoolLimbs * K2 + g, (size_t)K2);
    }
}

template <class M>
__global__ __launch_bounds__(256) void k_region_weights(const long long* __restrict__ ei, const long long* __restrict__ offsets, const float* __restrict__ sums,
                                                        const M* __restrict__ counts, float* __restrict__ weight, int N, int C, uint32_t K, long long E,
                                                        int mode) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const unsigned long long a = (unsigned long long)ei[e], b = (unsigned long long)ei[E + e];
        float w = __builtin_inff();
        if (a < K && b < K) {
            const size_t f = (size_t)frame_of(offsets, N, e);
            const M ca = counts[f * K + a], cb = counts[f * K + b];
            if (ca > M(0) && cb > M(0)) {
                const float na = (float)ca, nb = (float)cb;
                const float* __restrict__ p = sums + f * (size_t)C * K;
                float s = 0.0f;
                for (int c = 0; c < C; ++c, p += K) {
                    const float d = p[a] / na - p[b] / nb;
                    s = s + d * d;                                             // (the first addition is exact: 0 + q)
                }
                w = mode == kRegionWard ? ((na * nb) / (na + nb)) * s : sqrtf(s);
            }
        }
        weight[e] = w;
    }
}

template <class M>
static void region_sums_as(const float* values, const int32_t* mapping, const M* counts, float* sums, M* counts_out, void* workspace,
                           int N, int C, int K, int K2, hipStream_t st) {
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(workspace);
    const unsigned long long in = (unsigned long long)N * (unsigned long long)C * (unsigned long long)K;
    const unsigned long long out = (unsigned long long)N * (unsigned long long)C * (unsigned long long)K2;
    launch(k_region_accumulate<M>, dim3(tile_grid(in, 256)), dim3(256), 0, st, values, mapping, counts, acc, counts_out, (uint32_t)C, (uint32_t)K,
           (uint32_t)K2, in);
    launch(k_region_finalize, dim3(tile_grid(out, 256)), dim3(256), 0, st, acc, sums, (uint32_t)K2, out);
}

void launch_region_sums(const float* values, const int32_t* mapping, const void* counts, int counts_type, float* sums, void* counts_out,
                        void* workspace, int N, int C, int K, int K2, hipStream_t st) {
    if (counts && counts_type == kLabelI64)
        region_sums_as(values, mapping, reinterpret_cast<const int64_t*>(counts), sums, reinterpret_cast<int64_t*>(counts_out), workspace, N, C, K, K2, st);
    else
        region_sums_as(values, mapping, reinterpret_cast<const int32_t*>(counts), sums, reinterpret_cast<int32_t*>(counts_out), workspace, N, C, K, K2, st);
}

void launch_region_edge_weights(const long long* edge_index, const long long* offsets, const float* sums, const void* counts, int counts_type,
                                int mode, float* weight, int N, int C, int K, long long E, hipStream_t st) {
    const dim3 grid = entry_grid((unsigned long long)E), block(256);               // one edge a thread and round
    if (counts_type == kLabelI64)
        launch(k_region_weights<int64_t>, grid, block, 0, st, edge_index, offsets, sums, reinterpret_cast<const int64_t*>(counts), weight, N, C, (uint32_t)K, E, mode);
    else
        launch(k_region_weights<int32_t>, grid, block, 0, st, edge_index, offsets, sums, reinterpret_cast<const int32_t*>(counts), weight, N, C, (uint32_t)K, E, mode);
}

}  // namespace fslic
