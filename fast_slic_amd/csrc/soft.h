// soft.h -- soft superpixel assignment on float feature planes over a regular seed grid (soft.hip, softapi.cpp).  Internal to the library.
//
// Geometry: a frame of H x W pixels and a grid of gh x gw cells (1 <= gh <= H, 1 <= gw <= W, K = gh * gw <= 65534).  Pixel (y, x) lies
// in cell (cy, cx) = ((y * gh) / H, (x * gw) / W), integer arithmetic; cell c of an axis of L pixels and g cells starts at pixel
// ceil(c * L / g), so every cell holds a pixel.  Slot j = 3 (dy + 1) + (dx + 1), dy, dx in {-1, 0, 1}, of a pixel names cell
// (cy + dy, cx + dx), superpixel k = (cy + dy) * gw + (cx + dx); a slot outside the grid is invalid: its Q is +0.0 and it is never read.
//   features : float [N][C][H][W]      centres, values, sums : float [N][C][K]      Q, gd : float [N][9][H][W]      weights : float [N][K]
// Arithmetic: soft.hip is compiled with the Makefile's default contraction (hipcc's -ffp-contract=fast: a * b + c becomes one fma);
// nothing in it is compared bit for bit with another implementation, only with itself.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "launch.h"

namespace fslic {

constexpr int kSoftChunk = 16;         // channels of one k_soft_pool item (one accumulator register each)
constexpr int kSoftStage = 4096;       // pixels of a window staged in LDS at a time (weight and pixel offset: 32 KB)
constexpr int kSoftMaxK = 65534;
// Launch rule.  Every kernel runs one 256-thread block per item (a pixel kernel: N * ceil(H W / 256) blocks; k_soft_pool: N * K *
// ceil(C / kSoftChunk)), and the entries admit both counts up to 2^31 - 1.  The HIP runtime supports no launch of 2^32 or more threads
// in a grid dimension, that is 2^24 blocks of 256, and it does not refuse one: measured on the MI355X, a grid of b >= 2^24 blocks
// returns hipSuccess and runs b mod 2^24 of them, so the rest of the output stays unwritten.  The launches of soft.hip therefore go
// out in slices of at most kSoftMaxBlocks blocks, in order on the stream, each with the flat index of its first block as the kernel's
// last argument: a block computes what it would in one launch, bit for bit, and below 2^24 blocks there is one launch as before.
constexpr unsigned long long kSoftMaxBlocks = kMaxLaunchBlocks;        // 2^32 - 256 threads: the largest launch the runtime supports (launch.h)

// d_j = sum_c (F[c][p] - S[c][k_j])^2 in ascending c; Q_j = exp(-(d_j - min d)) / sum over the valid slots
void launch_soft_assign(const float* feat, const float* centres, float* q, int N, int C, int H, int W, int gh, int gw, hipStream_t st);
// gd_j = -Q_j (gQ_j - sum_i gQ_i Q_i), gF[c][p] = 2 sum_j gd_j (F[c][p] - S[c][k_j])
void launch_soft_assign_bwd(const float* feat, const float* centres, const float* q, const float* gq, float* gd, float* gfeat,
                            int N, int C, int H, int W, int gh, int gw, hipStream_t st);
// sums[c][k] = sum over the 3 x 3 cell window of k of Q_{j_k(p)}(p) * F[c][p] (with centres: * (F[c][p] - S[c][k])); weights (optional)
// the same sum of Q alone
void launch_soft_pool(const float* feat, const float* q, const float* centres, float* sums, float* weights,
                      int N, int C, int H, int W, int gh, int gw, hipStream_t st);
// out[c][p] = sum over the valid slots of Q_j(p) * V[c][k_j]
void launch_soft_unpool(const float* values, const float* q, float* out, int N, int C, int H, int W, int gh, int gw, hipStream_t st);
// out_j(p) = sum_c A[c][p] * B[c][k_j] (+ bias[k_j]), 0 on an invalid slot
void launch_soft_dot(const float* a, const float* b, const float* bias, float* out, int N, int C, int H, int W, int gh, int gw, hipStream_t st);

// blocks of k_soft_pool: one per (frame, superpixel, chunk of channels)
inline unsigned long long soft_pool_items(int N, int C, int K) {
    return (unsigned long long)N * (unsigned long long)K * (unsigned long long)((C + kSoftChunk - 1) / kSoftChunk);
}

}  // namespace fslic
