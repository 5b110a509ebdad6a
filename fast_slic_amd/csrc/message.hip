// message.hip -- messages over neighbour lists, gfx950 (fast_slic_amd/messages.py states the rules; layout, checks and the launch
// shapes are message.h's; the tile and its walk are lists.h's).
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
    __shared__ int s_node[kAggStage];
    __shared__ int s_p[BACK ? kAggStage : 1];
    __shared__ float s_m[kMsgFeatures][kAggStage];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x) {      // (the same trips for every thread of a block)
        const ListTile T = list_tile(item, groups, offsets, nnz);
        const uint32_t c = T.group * (uint32_t)kMsgFeatures + wave;
        const bool active = c < (uint32_t)F;                                           // the same in every lane of a wave
        const size_t hoff = (size_t)c * (size_t)nnz;                                   // (used by an active wave only)
        __syncthreads();                                                               // the walks of the item before are over
        list_stage<BACK, BACK>(T, ia, ib, R, nnz, (LdsInt*)s_node, (LdsInt*)s_p);
        if (BACK) __syncthreads();                                                     // the transposed window's messages are gathered through s_p
        if (active) list_stage_floats<BACK>(T, m + hoff, (LdsInt*)s_p, (LdsFloat*)s_m[wave], lane);
        __syncthreads();
        const uint32_t r = T.row0 + lane;
        if (!active || r >= R) continue;                                               // (no barrier below this line)
        const ListRow row = list_row(offsets, r, K, nnz);
        float acc = 0.0f;
        int arg = -1, d = 0;
        for (int pos = row.begin; pos < row.end; ++pos) {
            const ListPos e = list_at<BACK, BACK>(T, row, pos, ia, ib, K, R, nnz, (LdsInt*)s_node, (LdsInt*)s_p);
            if (!e.valid) continue;
            const float v = e.win ? ((const LdsFloat*)s_m[wave])[e.t] : m[hoff + (size_t)e.p];      // (a ds_read or a global_load: lists.h)
            ++d;
            if (MODE == kMsgSum || MODE == kMsgMean) {
                acc = acc + v;
            } else if (arg < 0 || (MODE == kMsgMax ? v > acc : v < acc)) {
                acc = v, arg = e.p;
            }
        }
        const size_t cell = ((size_t)row.f * (size_t)F + (size_t)c) * K + row.i;
        out[cell] = MODE == kMsgMean ? (d > 0 ? acc / (float)d : 0.0f) : acc;
        if (MODE == kMsgMax || MODE == kMsgMin) argmax[cell] = arg;
        if (MODE == kMsgMean && c == 0u) degree[r] = d;
    }
}

}  // namespace

void launch_message_gather(int end, const int32_t* rows, const int32_t* indices, const float* values, const int32_t* scale_degree,
                           const int32_t* argmax, float* out, int N, int C, int K, long long nnz, hipStream_t st) {
    const unsigned long long total = (unsigned long long)C * (unsigned long long)nnz;          // one (feature, entry) a thread and round
    launch(k_message_gather, entry_grid(total), dim3(256), 0, st, rows, indices, values, scale_degree, argmax, out, end == kMsgSource ? 1 : 0, C,
           (uint32_t)K, (uint32_t)N * (uint32_t)K, (uint32_t)nnz, (uint32_t)total);
}

void launch_message_reduce(int reduce, bool transposed, const long long* offsets, const int32_t* ia, const int32_t* ib, const float* messages,
                           float* out, int32_t* argmax, int32_t* degree, int N, int C, int K, long long nnz, hipStream_t st) {
    const ListLaunch g = list_launch(N, K, ((uint32_t)C + kMsgFeatures - 1u) / kMsgFeatures);
#define FSLIC_MSG(MODE) (transposed ? k_message_reduce<MODE, true> : k_message_reduce<MODE, false>)
    const auto kernel = reduce == kMsgMean ? FSLIC_MSG(kMsgMean) : reduce == kMsgMax ? FSLIC_MSG(kMsgMax) : reduce == kMsgMin ? FSLIC_MSG(kMsgMin) : FSLIC_MSG(kMsgSum);
#undef FSLIC_MSG
    launch(kernel, g.grid, dim3(256), 0, st, offsets, ia, ib, messages, out, argmax, degree, C, (uint32_t)K, g.R, (int)nnz, g.groups, g.items);
}

}  // namespace fslic
