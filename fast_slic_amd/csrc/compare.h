// compare.h -- two label maps of one shape against each other (compare.hip, compareapi.cpp): the overlap table and the boundary
// match.  Internal to the library.
//
// The overlap's workspace is the label pair table of pairtable.h with C = 0:
//   keys   : (a << 16 | b) + 1 of the label pair (a < K, b < M, K and M <= 65534: at most 0xFFFDFFFE), which the pair (0, 0) needs
//            to be no empty slot: key_bias 1 in the compact pass
//   counts : the pixels of that pair
// The boundary match needs no workspace: its three counters per frame are the result.
#pragma once
#include "pairtable.h"

namespace fslic {

constexpr int kMatchMaxTolerance = 15;               // a tile of 32 rows and its halo of 15 on either side: one row per lane

// labels, other: N x H x W of the given LabelTypes (labels.h)
void launch_overlap_accumulate(const void* labels, int label_type, const void* other, int other_type, void* workspace,
                               int N, int H, int W, int K, int M, uint32_t capacity, hipStream_t st);
// out: uint64 [N][3] = (hits, boundary pixels of other, boundary pixels of labels), cleared by the caller
void launch_boundary_match(const void* labels, int label_type, const void* other, int other_type, unsigned long long* out,
                           int N, int H, int W, int tolerance, hipStream_t st);

}  // namespace fslic
