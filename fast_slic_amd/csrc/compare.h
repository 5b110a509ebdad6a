// compare.h -- two label maps of one shape against each other (compare.hip, compareapi.cpp): the overlap table and the boundary
// match.  Internal to the library.
//
// Workspace of one fslic_hip_overlap_accumulate call (offsets from its start, every part 8-byte aligned):
//   header : RagHeader (rag.h): uint32 overflow flag, uint32 unused, uint64 cursor of compact, then uint32 distinct pairs of
//            frame n [N]; padded to 16 bytes
//   keys   : uint32 [N][capacity]  -- (a << 16 | b) + 1 of the label pair (a < K, b < M, K and M <= 65534: at most 0xFFFDFFFE);
//                                     0 = empty slot, which the pair (0, 0) therefore never is
//   count  : uint32 [N][capacity]  -- the pixels of that pair
// The boundary match needs no workspace: its three counters per frame are the result.
#pragma once
#include "rag.h"

namespace fslic {

constexpr uint32_t kOverlapMinCapacity = 64u;        // capacities are powers of two in [kOverlapMinCapacity, kOverlapMaxCapacity]
constexpr uint32_t kOverlapMaxCapacity = 1u << 31;
constexpr int kMatchMaxTolerance = 15;               // a tile of 32 rows and its halo of 15 on either side: one row per lane

inline size_t overlap_workspace_bytes(int N, uint32_t capacity) { return rag_header_bytes(N) + (size_t)N * (size_t)capacity * 8; }

// labels, other: N x H x W of the given PoolLabel types (pool.h)
void launch_overlap_accumulate(const void* labels, int label_type, const void* other, int other_type, void* workspace,
                               int N, int H, int W, int K, int M, uint32_t capacity, hipStream_t st);
void launch_overlap_compact(void* workspace, int N, uint32_t capacity, unsigned long long* keys, int32_t* count,
                            unsigned long long max_pairs, hipStream_t st);
// out: uint64 [N][3] = (hits, boundary pixels of other, boundary pixels of labels), cleared by the caller
void launch_boundary_match(const void* labels, int label_type, const void* other, int other_type, unsigned long long* out,
                           int N, int H, int W, int tolerance, hipStream_t st);

}  // namespace fslic
