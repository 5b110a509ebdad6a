// rag.h -- the region adjacency graph of a label map (rag.hip, ragapi.cpp).  Internal to the library.
//
// Its workspace is the label pair table of pairtable.h:
//   keys   : lo << 16 | hi of the unordered label pair (lo < hi < K <= 65534, so never 0): key_bias 0 in the compact pass
//   counts : the boundary, the neighbouring pixel pairs of that label pair
//   sums   : the contrast, per channel the sum of |difference| over those pixel pairs (C = 0: no image, no sums)
#pragma once
#include "pairtable.h"

namespace fslic {

// labels: N x H x W of the given LabelType (labels.h); image: N x H x W x C uint8 or nullptr (then C == 0)
void launch_rag_accumulate(const void* labels, int label_type, const uint8_t* image, void* workspace,
                           int N, int C, int H, int W, int K, int connectivity, uint32_t capacity, hipStream_t st);

}  // namespace fslic
