// region.h -- the features of merged regions (region.hip, regionapi.cpp; fast_slic_amd/regions.py states the rules): the exact sums
// of node values over the groups of a mapping, and the weights of a graph's edges from the regions' means.  Internal to the library.
//
// Nodes and graphs as merge.h: N frames of K nodes, E edges, edge_index int64 [2][E], offsets int64 [N + 1].  Everything a kernel
// reads from device memory is checked before it becomes an index: a mapping word outside [0, K2) adds nothing, an edge with a node
// outside [0, K) has the weight +inf, and the frame of an edge is merge.h's search.
//
// Workspace of region_sums: acc[N][C][kPoolLimbs][K2] int64, the fixed-point accumulator of fixsum.h, one per (frame, channel, group).
// The caller clears it, and the output counts, before the launch.
#pragma once
#include "merge.h"
#include "pool.h"

namespace fslic {

enum RegionMode { kRegionMean = 0, kRegionWard = 1 };

inline size_t region_sums_workspace_bytes(int N, int C, int K2) { return (size_t)N * (size_t)C * (size_t)K2 * 8 * kPoolLimbs; }

// sums[n][c][g] = the exact sum (fixsum.h) of values[n][c][v] over the nodes v with mapping[n][v] == g, for g in [0, K2);
// counts_out[n][g] likewise from counts (both int32: kLabelI32, or int64: kLabelI64; nullptr: no counts).  Two launches.
void launch_region_sums(const float* values, const int32_t* mapping, const void* counts, int counts_type, float* sums, void* counts_out,
                        void* workspace, int N, int C, int K, int K2, hipStream_t st);
// weight[e] by the rule of regions.py from sums float [N][C][K] and counts [N][K] (kLabelI32 / kLabelI64).  One launch.
void launch_region_edge_weights(const long long* edge_index, const long long* offsets, const float* sums, const void* counts, int counts_type,
                                int mode, float* weight, int N, int C, int K, long long E, hipStream_t st);

}  // namespace fslic
