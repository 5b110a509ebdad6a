// message.h -- messages over neighbour lists: the gather of node features to the entries and the reduction of a per-entry array to
// the nodes, which are each other's gradients (message.hip, messageapi.cpp; fast_slic_amd/messages.py states the rules).  Internal
// to the library.
//
// Lists, transposed lists, features, the rule of what is trusted and the tile with its LDS window are lists.h's.  A per-entry array is
// float [F][nnz], the entries innermost (attend.h's [Hd][nnz]); the node side of a reduce is float [N][F][K].
//
// Launch shapes.
//   gather   one thread per (feature, entry), the entries innermost, grid-stride (attend.h's dot): rows[p] and indices[p] are read
//            coalesced, the store is coalesced, a channel's K floats stay in cache.
//   reduce   an item is a tile x 4 features (attend.h's softmax): wave w owns feature 4 * group + w and keeps the window of its
//            feature's messages, gathered through the staged entries in the transposed form.
#pragma once
#include "lists.h"

namespace fslic {

enum MessageEnd { kMsgTarget = 0, kMsgSource = 1 };
enum MessageReduce { kMsgSum = 0, kMsgMean = 1, kMsgMax = 2, kMsgMin = 3 };

constexpr int kMsgFeatures = 4;            // features of a reduce item: one per wave of the block

// out[c][p] = values[n][c][node], (n, i) = rows[p], node = i (kMsgTarget) or indices[p] (kMsgSource); +0.0 where rows[p] is outside
// [0, N * K) or indices[p] outside [0, K).  scale_degree (int32 [N * K]) != nullptr: the value divided by (float)scale_degree[n * K +
// node].  argmax (int32 [N][C][K]) != nullptr: +0.0 unless argmax[n][c][node] == p.  One launch; nnz > 0.
void launch_message_gather(int end, const int32_t* rows, const int32_t* indices, const float* values, const int32_t* scale_degree,
                           const int32_t* argmax, float* out, int N, int C, int K, long long nnz, hipStream_t st);
// out[n][c][i] = the fold by `reduce` over the valid entries of row (n, i) of messages[c][p] (ia = indices, ib = nullptr), or over the
// transposed lists (transposed: offsets = t_offsets, ia = t_entries, ib = t_rows) of messages[c][t_entries[q]].  argmax int32
// [N][C][K] (kMsgMax, kMsgMin): the entry p the extremum was first met at, -1 for none; degree int32 [N * K] (kMsgMean): the terms of
// each fold.  One launch, also for nnz == 0 (zeros).
void launch_message_reduce(int reduce, bool transposed, const long long* offsets, const int32_t* ia, const int32_t* ib, const float* messages,
                           float* out, int32_t* argmax, int32_t* degree, int N, int C, int K, long long nnz, hipStream_t st);

}  // namespace fslic
