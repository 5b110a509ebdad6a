// message.hip -- messages over neighbour lists, gfx950 (fast_slic_amd/messages.py states the rules; layout, checks and the launch
// shapes are message.h's).
//   k_message_gather         : one thread per (feature, entry); the value of the entry's own node or of its neighbour, optionally
//                              divided by the node's degree (the backward of the mean) or kept only where the node's argmax names the
//                              entry (the backward of the max and the min).  A plain load and a plain store: a copy, bit for bit.
//   k_message_reduce<M, BACK>: a lane owns a (row, feature) and walks the row's positions in ascending order, from the LDS window or
//                              from global memory beyond it: sum, mean (one division by the count of the terms), or the first largest
//                              / smallest message and its entry.  BACK: the same walk over the transposed lists, the window's
//                              messages gathered through the staged entry numbers.
// This file is compiled with -ffp-contract=off: every sum and quotient is one IEEE float operation rounded on its own, and the
// division is HIP's correctly rounded one.  No atomics, and no kernel waits for another block.
#include "message.h"
#include "aggregate.h"
#include "launch.h"

namespace fslic {

namespace {

__global__ __launch_bounds__(256) void k_message_gather(const int32_t* __restrict__ rows, const int32_t* __restrict__ indices, const float* __restrict__ x,
                                                        const int32_t* __restrict__ degree, const int32_t* __restrict__ argmax, float* __restrict__ out,
                                                        int source, int C, uint32_t K, uint32_t R, uint32_t nnz, uint32_t total) {
    // total = C * nnz < 2^31, and a round of the grid is 2^19 threads: q does not wrap
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
        const uint32_t c = q / nnz, p = q - c * nnz;
        const uint32_t r = (uint32_t)rows[p], j = (uint32_t)indices[p];
        float v = 0.0f;
        if (r < R && j < K) {
            const uint32_t f = r / K, node = source ? j : r - f * K;
            const size_t cell = ((size_t)f * (size_t)C + (size_t)c) * K + node;
            v = x[cell];
            if (degree) v = v / (float)degree[(size_t)f * K + node];                   // (the same in every thread of the launch)
            if (argmax && argmax[cell] != (int32_t)p) v = 0.0f;
        }
        out[q] = v;
    }
}

template <int MODE, bool BACK>
__global__ __launch_bounds__(256) void k_message_reduce(const long long* __restrict__ offsets, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
                                                        const float* __restrict__ m, float* __restrict__ out, int32_t* __restrict__ argmax,
                                                        int32_t* __restrict__ degree, int F, uint32_t K, uint32_t R, int nnz, uint32_t groups,
                                                        unsigned long long items) {
    __shared__ int s_a[kAggStage];                                                     // the index of the position; BACK: its entry, -1 outside [0, nnz)
    __shared__ int s_r[BACK ? kAggStage : 1];                                          // BACK: the row of that entry
    __shared__ float s_m[kMsgFeatures][kAggStage];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x) {      // (the same trips for every thread of a block)
        const uint32_t tile = (uint32_t)(item / groups), group = (uint32_t)(item - (unsigned long long)tile * groups);
        const uint32_t row0 = tile * (uint32_t)kAggRows;                               // < R
        const uint32_t c = group * (uint32_t)kMsgFeatures + wave;
        const bool active = c < (uint32_t)F;                                           // the same in every lane of a wave
        const size_t hoff = (size_t)c * (size_t)nnz;                                   // (used by an active wave only)
        const int lo = row_bound(offsets, row0, nnz);
        const int staged = nnz - lo < kAggStage ? nnz - lo : kAggStage;
        __syncthreads();                                                               // the walks of the item before are over
        for (int t = threadIdx.x; t < staged; t += 256) {
            if (!BACK) {
                s_a[t] = ia[lo + t];
            } else {
                const int p = ia[lo + t];                                              // t_entries
                s_a[t] = (uint32_t)p < (uint32_t)nnz ? p : -1;
                s_r[t] = ib[lo + t];                                                   // t_rows
            }
        }
        if (BACK) __syncthreads();                                                     // the transposed window's messages are gathered through s_a
        if (active) {
            for (int t = lane; t < staged; t += 64) s_m[wave][t] = !BACK ? m[hoff + (size_t)(lo + t)] : s_a[t] >= 0 ? m[hoff + (size_t)s_a[t]] : 0.0f;
        }
        __syncthreads();
        const uint32_t r = row0 + lane;
        if (!active || r >= R) continue;                                               // (no barrier below this line)
        const int begin = row_bound(offsets, r, nnz);
        int end = row_bound(offsets, r + 1u, nnz);
        if (end < begin) end = begin;
        const uint32_t f = r / K, i = r - f * K, base = f * K;
        float acc = 0.0f;
        int arg = -1, d = 0;
        for (int pos = begin; pos < end; ++pos) {
            const uint32_t t = (uint32_t)(pos - lo);                                   // (a row before the window wraps beyond it)
            const bool win = t < (uint32_t)staged;
            int p = pos;
            float v;
            if (!BACK) {
                if ((uint32_t)(win ? s_a[t] : ia[pos]) >= K) continue;
                v = win ? s_m[wave][t] : m[hoff + (size_t)pos];
            } else {
                p = win ? s_a[t] : ia[pos];
                const uint32_t rr = (uint32_t)(win ? s_r[t] : ib[pos]);
                if ((uint32_t)p >= (uint32_t)nnz || rr - base >= K) continue;          // an entry outside the lists, a row outside the target's frame
                v = win ? s_m[wave][t] : m[hoff + (size_t)p];
            }
            ++d;
            if (MODE == kMsgSum || MODE == kMsgMean) {
                acc = acc + v;
            } else if (arg < 0 || (MODE == kMsgMax ? v > acc : v < acc)) {
                acc = v, arg = p;
            }
        }
        const size_t cell = ((size_t)f * (size_t)F + (size_t)c) * K + i;
        out[cell] = MODE == kMsgMean ? (d > 0 ? acc / (float)d : 0.0f) : acc;
        if (MODE == kMsgMax || MODE == kMsgMin) argmax[cell] = arg;
        if (MODE == kMsgMean && c == 0u) degree[r] = d;
    }
}

}  // namespace

void launch_message_gather(int end, const int32_t* rows, const int32_t* indices, const float* values, const int32_t* scale_degree,
                           const int32_t* argmax, float* out, int N, int C, int K, long long nnz, hipStream_t st) {
    // one (feature, entry) a thread and round, with at most the 2048 blocks of 256 threads the chip holds at once (as attend.hip's dot)
    const unsigned long long total = (unsigned long long)C * (unsigned long long)nnz;
    const int blocks = tile_grid(total, 256);
    launch(k_message_gather, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, rows, indices, values, scale_degree, argmax, out,
           end == kMsgSource ? 1 : 0, C, (uint32_t)K, (uint32_t)N * (uint32_t)K, (uint32_t)nnz, (uint32_t)total);
}

void launch_message_reduce(int reduce, bool transposed, const long long* offsets, const int32_t* ia, const int32_t* ib, const float* messages,
                           float* out, int32_t* argmax, int32_t* degree, int N, int C, int K, long long nnz, hipStream_t st) {
    const uint32_t R = (uint32_t)N * (uint32_t)K, tiles = (R + kAggRows - 1u) / kAggRows, groups = ((uint32_t)C + kMsgFeatures - 1u) / kMsgFeatures;
    const unsigned long long items = (unsigned long long)tiles * groups;
    const dim3 grid((unsigned)tile_grid(items, 1)), block(256);
#define FSLIC_MSG(MODE)                                                                                                                  \
    do {                                                                                                                                 \
        if (transposed) launch(k_message_reduce<MODE, true>, grid, block, 0, st, offsets, ia, ib, messages, out, argmax, degree, C, (uint32_t)K, R, (int)nnz, groups, items); \
        else launch(k_message_reduce<MODE, false>, grid, block, 0, st, offsets, ia, ib, messages, out, argmax, degree, C, (uint32_t)K, R, (int)nnz, groups, items); \
    } while (0)
    if (reduce == kMsgMean) FSLIC_MSG(kMsgMean);
    else if (reduce == kMsgMax) FSLIC_MSG(kMsgMax);
    else if (reduce == kMsgMin) FSLIC_MSG(kMsgMin);
    else FSLIC_MSG(kMsgSum);
#undef FSLIC_MSG
}

}  // namespace fslic
