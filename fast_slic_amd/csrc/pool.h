// pool.h -- superpixel pooling / unpooling of float feature planes (pool.hip, poolapi.cpp).  Internal to the library.
//
// Workspace of one fslic_hip_pool call (offsets from its start, every part 8-byte aligned):
//   sum / mean : acc[N][C][kPoolLimbs][K] int64 -- the exact fixed-point sum of every (n, c, k), one 32-bit limb per word
//   max        : key[N][C][K] uint64             -- (order-preserving bits of x) << 32 | (0xFFFFFFFF - flat pixel index)
//   then       : counts[N][K] uint32
#pragma once
#include "labels.h"
#include <cstddef>

namespace fslic {

constexpr int kPoolLimbs = 7;          // 7 x 32 bits: the fixed point spans 2^-96 .. 2^128
constexpr int kPoolLsb = -96;          // weight of bit 0 of limb 0

enum PoolReduce { kPoolSum = 0, kPoolMean = 1, kPoolMax = 2 };

inline size_t pool_acc_bytes(int N, int C, int K, int reduce) {
    const size_t cells = (size_t)N * (size_t)C * (size_t)K;
    return reduce == kPoolMax ? cells * 8 : cells * 8 * kPoolLimbs;
}
inline size_t pool_workspace_bytes(int N, int C, int K, int reduce) {
    return pool_acc_bytes(N, C, K, reduce) + (((size_t)N * (size_t)K * 4 + 7) & ~(size_t)7);
}

// labels: N x H x W of the given LabelType (labels.h); label values outside [0, K) are skipped everywhere
void launch_pool_tiles(const float* feat, const void* labels, int label_type, int reduce, void* workspace,
                       int N, int C, int H, int W, int K, hipStream_t st);
void launch_pool_finalize(const void* workspace, int reduce, float* values, int32_t* counts, int32_t* argmax,
                          int N, int C, int K, hipStream_t st);
void launch_unpool(const float* values, const void* labels, int label_type, const int32_t* argmax, float fill, float* out,
                   int N, int C, int H, int W, int K, hipStream_t st);

}  // namespace fslic
