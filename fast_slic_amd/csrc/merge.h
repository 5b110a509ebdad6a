// merge.h -- merging superpixels on the region adjacency graph (merge.hip, mergeapi.cpp; fast_slic_amd/merge.py states the rules).
// Internal to the library.
//
// A graph has N frames of K nodes and E edges: edge_index int64 [2][E] (row 0: a, row 1: b), offsets int64 [N + 1]; the edges of
// frame f are [offsets[f], offsets[f + 1]), and the position of an edge is its index minus offsets[f].  N * K < 2^31 and E < 2^31.
// Everything a kernel reads from device memory is checked before it becomes an index: a node outside [0, K) takes its edge out of
// every pass, and the frame of an edge is the result of a search over offsets[1 .. N], clamped to [0, N - 1] whatever they hold.
//
// Workspace of best_edges: uint64 [N][K], per node the smallest key (weight bits << 32 | position) of its eligible edges.
// Workspace of components, every part 16-byte aligned:
//   parent : uint32 [N][K]   a node of v's group with a number <= v, kMergeAbsent for an absent node; after k_merge_flatten the leader
//   rank   : uint32 [N][K]   at a leader: the number of its group
//   sums   : uint32 [N][ceil(K / 256)]   leaders per chunk of 256 nodes, then (k_merge_scan) those of the frame's chunks before it
#pragma once
#include "pairtable.h"

namespace fslic {

constexpr int kMergeChunk = 256;                     // nodes of one block of the rank passes
constexpr uint32_t kMergeAbsent = 0xFFFFFFFFu;       // the parent word of a node that is in no group

// (kernels of merge.hip and region.hip) The frame of edge e: how many of offsets[1 .. N] are <= e
// (torch.searchsorted(offsets[1:], e, right=True)), at most N - 1.
static __device__ __forceinline__ int frame_of(const long long* __restrict__ offsets, int N, long long e) {
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid + 1] <= e) lo = mid + 1;
        else hi = mid;
    }
    return min(lo, N - 1);
}

inline size_t merge_align(size_t b) { return (b + 15) & ~(size_t)15; }
inline size_t merge_chunks_per_frame(int K) { return ((size_t)K + kMergeChunk - 1) / kMergeChunk; }
inline size_t merge_best_workspace_bytes(int N, int K) { return (size_t)N * (size_t)K * 8; }
inline size_t merge_components_workspace_bytes(int N, int K) {
    return 2 * merge_align((size_t)N * (size_t)K * 4) + merge_align((size_t)N * merge_chunks_per_frame(K) * 4);
}

// join[e] = 1 where e is the best edge of one of its two nodes, 0 elsewhere.  `all`: every edge is eligible, else those with
// weight < threshold.  The caller has set every byte of the workspace to 0xFF.
void launch_merge_best_edges(const long long* edge_index, const long long* offsets, const float* weight, bool all, double threshold,
                             uint8_t* join, void* workspace, int N, int K, long long E, hipStream_t st);
// members: int32 (kLabelI32) or int64 (kLabelI64) [N][K], or nullptr: every node is present.  mapping int32 [N][K], counts int32 [N].
void launch_merge_components(const long long* edge_index, const long long* offsets, const uint8_t* join, const void* members,
                             int members_type, int32_t* mapping, int32_t* counts, void* workspace, int N, int K, long long E, hipStream_t st);
// out[p] = mapping[frame of p][labels[p]], -1 where the label is outside [0, K); P pixels per frame, N * P < 2^31
void launch_merge_labels(const void* labels, int label_type, const int32_t* mapping, int32_t* out, int N, long long P, int K, hipStream_t st);
// Adds every edge's boundary and contrast row to the pair (min, max) of its nodes' images under `mapping` in the pair table of
// pairtable.h (keys and key_bias as rag.h); contrast int64 [E][C] or nullptr (then C == 0).
void launch_merge_contract(const long long* edge_index, const long long* offsets, const int32_t* boundary, const long long* contrast,
                           const int32_t* mapping, void* workspace, int N, int C, int K, int K2, long long E, uint32_t capacity, hipStream_t st);

}  // namespace fslic
