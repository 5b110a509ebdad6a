// attend.h -- attention over neighbour lists: the per-entry dot product of two feature arrays, the softmax over each row's entries and
// the neighbour sum with one weight per head, which are each other's gradients (attend.hip, attendapi.cpp;
// fast_slic_amd/attention.py states the rules).  Internal to the library.
//
// Lists, transposed lists, features, the rule of what is trusted and the tile with its LDS window are lists.h's.  Hd heads, D = C / Hd
// channels a head, head h owns the channels h D .. h D + D - 1.  A per-entry array is float [Hd][nnz], the entries innermost.
//
// Launch shapes.
//   dot      one thread per (head, entry), the entries innermost, grid-stride; the channels of the head in ascending order.
//   softmax  an item is a tile x 4 heads: wave w owns head 4 * group + w and keeps the window of its head's scores.  A lane writes its
//            results into the window, or to global memory for what lies beyond it, and the wave stores the window's part of the tile
//            coalesced.
//   apply    an item is a tile x 4 waves x 8 channels; a wave's eight channels never straddle a head.  Plain shape: an item is 32
//            channels of one head and the block shares the head's weight window.  With D < 32 that shape would leave waves of every
//            block idle, and in the packed shape the four waves take consecutive eight-channel chunks of the (head, chunk) sequence
//            instead, each with the weight window of its own head: with D = 8 they serve four heads (attend_pack; DESIGN.md has the
//            comparison).  graph_aggregate's weighted sum is the plain shape at one head, whatever its C.
#pragma once
#include "lists.h"

namespace fslic {

constexpr int kAttendHeads = 4;            // heads of a softmax item: one per wave of the block
// The item shape head_aggregate takes for heads of D channels (true: packed).  -DFSLIC_ATTEND_PACK=0 / =1 (make VAR=.. DEFS=..) builds a
// library with one shape throughout, for the comparison of scripts/attention_bench.py.
inline bool attend_pack(int D) {
#ifdef FSLIC_ATTEND_PACK
    return FSLIC_ATTEND_PACK != 0;
#else
    return D < 32;
#endif
}

// out[h][p] = the left fold from +0.0 over c = h D .. h D + D - 1 of a[n][c][i] * b[n][c][indices[p]], (n, i) = rows[p]; +0.0 where
// rows[p] is outside [0, N * K) or indices[p] outside [0, K).  One launch; nnz > 0.
void launch_attend_dot(const int32_t* rows, const int32_t* indices, const float* a, const float* b, float* out, int N, int C, int K, long long nnz,
                       int heads, hipStream_t st);
// grad == nullptr: out[h][p] = crf_expf(s - m) / Z over the valid entries of p's row, s = in[h][p] (rule 2 of attention.py).
// grad != nullptr: out[h][p] = alpha * (g - t), alpha = in[h][p], g = grad[h][p], t the row's fold of alpha * g.  +0.0 for every entry
// that is not valid, those outside every row included.  One launch; nnz > 0.
void launch_attend_softmax(const long long* offsets, const int32_t* indices, const float* in, const float* grad, float* out, int N, int K,
                           long long nnz, int heads, hipStream_t st);
// dst[n][c][i] = the left fold over the valid entries p of row (n, i) of weight[h(c)][p] * src[n][c][indices[p]] (ia = indices, ib =
// nullptr), or over the transposed lists (transposed: ia = t_entries, ib = t_rows) of weight[h(c)][p] * src[n][c][row(p)].  pack: the
// item shape; the bits do not depend on it.  One launch.
void launch_attend_apply(bool transposed, bool pack, const long long* offsets, const int32_t* ia, const int32_t* ib, const float* weight,
                         const float* src, float* dst, int N, int C, int K, long long nnz, int heads, hipStream_t st);

}  // namespace fslic
