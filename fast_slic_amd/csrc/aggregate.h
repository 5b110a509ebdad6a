// aggregate.h -- aggregation of node features over neighbour lists and its gradients (aggregate.hip, aggregateapi.cpp;
// fast_slic_amd/propagate.py states the rules).  Internal to the library.
//
// Lists: one CSR over the R = N * K rows (frame, node): offsets int64 [R + 1], indices int32 [nnz] (node numbers inside the frame),
// weight float [nnz] or nullptr.  Transposed lists (crf_torch.transpose_batch_csr): t_offsets int64 [R + 1] over the targets,
// t_entries int32 [nnz] the entry p and t_rows int32 [nnz] the row of p, per transposed position.  Features float [N][C][K].
// Nothing a kernel reads from device memory becomes an address before it is checked: row bounds are clamped into [0, nnz] and an end
// before its start is an empty row; an index outside [0, K), an entry outside [0, nnz) and a row outside the target's frame
// contribute nothing.
//
// Launch shape of the two list kernels: a block of 256 threads takes an item = 64 consecutive rows x 32 channels; lane l of every
// wave owns row 64 * tile + l, wave w the channels 32 * group + 8 w .. + 7, eight accumulators a lane.  The block first copies the
// first kAggStage entries behind the tile's first row into LDS (coalesced), and a lane walking its row takes an entry from there
// when it lies in that window and from global memory otherwise: a hub row longer than the window is walked in full, in order.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fslic {

enum AggregateReduce { kAggSum = 0, kAggMean = 1, kAggMax = 2 };

constexpr int kAggRows = 64;               // rows of an item: one wavefront of lanes
constexpr int kAggWaveChannels = 8;        // channels a lane accumulates at once
constexpr int kAggBlockChannels = 32;      // channels of an item: 4 waves x 8
constexpr int kAggStage = 1024;            // entries of the LDS window: 16 a row, a SLIC map has about 6

// the clamped bound of a row: offsets are not trusted (aggregate.hip, attend.hip)
__device__ __forceinline__ int row_bound(const long long* __restrict__ offsets, uint32_t r, int nnz) {
    const long long o = offsets[r];
    return o < 0 ? 0 : o > (long long)nnz ? nnz : (int)o;
}

// out[n][c][i] by rule 1, 2 or 3 of propagate.py; argmax int32 [N][C][K] (kAggMax), degree int32 [N * K] (kAggMean: the valid entries
// of each row).  weight only with kAggSum.  One launch.
void launch_aggregate_forward(int reduce, const long long* offsets, const int32_t* indices, const float* weight, const float* values, float* out,
                              int32_t* argmax, int32_t* degree, int N, int C, int K, long long nnz, hipStream_t st);
// grad_values[n][c][j] by rule 4 over the transposed lists.  One launch.
void launch_aggregate_backward_values(int reduce, const long long* t_offsets, const int32_t* t_entries, const int32_t* t_rows, const float* weight,
                                      const int32_t* argmax, const int32_t* degree, const float* grad_out, float* grad_values, int N, int C, int K,
                                      long long nnz, hipStream_t st);
// grad_weight[p] = the fold over c of values[n][c][indices[p]] * grad_out[n][c][i], (n, i) = rows[p]; one thread an entry.  One launch.
void launch_aggregate_backward_weight(const int32_t* rows, const int32_t* indices, const float* values, const float* grad_out, float* grad_weight,
                                      int N, int C, int K, long long nnz, hipStream_t st);

}  // namespace fslic
