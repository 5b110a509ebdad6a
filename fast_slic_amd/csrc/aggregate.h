// aggregate.h -- aggregation of node features over neighbour lists and its gradients (aggregate.hip, aggregateapi.cpp;
// fast_slic_amd/propagate.py states the rules).  Internal to the library.
//
// Lists, transposed lists, features, the rule of what is trusted and the tile with its LDS window are lists.h's; weight is float [nnz]
// or nullptr.  Launch shape of the list kernels: an item is a tile x 32 channels; wave w owns the channels 32 * group + 8 w .. + 7,
// eight accumulators a lane.
#pragma once
#include "lists.h"

namespace fslic {

enum AggregateReduce { kAggSum = 0, kAggMean = 1, kAggMax = 2 };

// out[n][c][i] by rule 1, 2 or 3 of propagate.py; argmax int32 [N][C][K] (kAggMax), degree int32 [N * K] (kAggMean: the valid entries
// of each row).  weight only with kAggSum: attend.h's apply with one head.  One launch.
void launch_aggregate_forward(int reduce, const long long* offsets, const int32_t* indices, const float* weight, const float* values, float* out,
                              int32_t* argmax, int32_t* degree, int N, int C, int K, long long nnz, hipStream_t st);
// grad_values[n][c][j] by rule 4 over the transposed lists.  One launch.
void launch_aggregate_backward_values(int reduce, const long long* t_offsets, const int32_t* t_entries, const int32_t* t_rows, const float* weight,
                                      const int32_t* argmax, const int32_t* degree, const float* grad_out, float* grad_values, int N, int C, int K,
                                      long long nnz, hipStream_t st);
// grad_weight[p] = the fold over c of grad_out[n][c][i] * values[n][c][indices[p]], (n, i) = rows[p]: attend.h's dot with one head.  One launch.
void launch_aggregate_backward_weight(const int32_t* rows, const int32_t* indices, const float* values, const float* grad_out, float* grad_weight,
                                      int N, int C, int K, long long nnz, hipStream_t st);

}  // namespace fslic
