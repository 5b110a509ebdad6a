// pixel.h -- pixels over neighbour lists: every pixel sees S slots, its own superpixel and the first S - 1 entries of that node's row,
// and the per-slot dot product, softmax, mix and scatter over them, which are each other's gradients (pixel.hip, pixelapi.cpp;
// fast_slic_amd/pixels.py states the rules).  Internal to the library.
//
// Label map as in pool.h (N x H x W of a LabelType, a value outside [0, K) is no label), lists as in lists.h (one CSR over the
// R = N * K rows, offsets int64 [R + 1], indices int32 [nnz]).  Pixel features float [N][C][H][W], node features float [N][C][K], a
// per-slot array float [N][Hd][S][H][W]; Hd heads, D = C / Hd channels a head, head h owns the channels h D .. h D + D - 1.
// The slots of a pixel of label i < K in frame f: slot 0 is node i; slot s >= 1 is entry p = lo + s - 1 of row f K + i, [lo, hi) the
// row's bounds clamped into [0, nnz], and it is empty unless p < hi and 0 <= indices[p] < K.  A pixel without a label has empty slots
// only.  Nothing a kernel reads from device memory becomes an address before it is checked (lists.h's rule).  No kernel keeps
// the S nodes of a pixel: a slot's node is read again where it is needed (label-coherent reads, served by the caches).
//
// Launch shapes.
//   dot      one thread per pixel, x innermost, grid-stride; per head four slots at a time: one load of `a` serves four gathers from
//            `b`, the channels of the head in ascending order; the per-slot planes are stored coalesced.
//   mix      one thread per pixel; per head four channels at a time: one load of the weight serves four gathers from the values,
//            the slots in ascending order.
//   softmax  one thread per (pixel, head); a 32-bit mask of the non-empty slots, then the walks of attend.hip's softmax over the S
//            planes of the head.
//   scatter  pool.hip's tile kernel: one wavefront per (frame, tile of 16 x 64 pixels, chunk of channels); the tile's distinct
//            labels once; per slot, head and channel the 16 products of a lane, per label a column sum in row order and the
//            wavefront's tree, and one fix_add (fixsum.h) from one lane to the node the slot names for that label; then a pass of
//            fix_to_float.  The accumulator is int64 [N][C][kPoolLimbs][K], zeroed on the stream by the entry.
#pragma once
#include "pool.h"
#include <cstdint>

namespace fslic {

constexpr int kPixelMaxSlots = 32;         // the softmax keeps a pixel's non-empty slots in one 32-bit mask

// what every launch takes: the sizes, the label map and the lists
struct PixelGeom {
    int N, C, H, W, K, S, heads;
    long long nnz;
    int label_type;
    const void* labels;
    const long long* offsets;
    const int32_t* indices;
};

inline size_t pixel_scatter_workspace_bytes(int N, int C, int K) { return pool_acc_bytes(N, C, K, kPoolSum); }

// out[n][h][s][y][x] = the left fold from +0.0 over c = h D .. h D + D - 1 of a[n][c][y][x] * b[n][c][j], j the slot's node; +0.0 for
// an empty slot.  One launch.
void launch_pixel_dot(const PixelGeom& g, const float* a, const float* b, float* out, hipStream_t st);
// grad == nullptr: out = crf_expf(s - m) / Z over the non-empty slots of each (pixel, head), s = in (rule 2 of pixels.py).
// grad != nullptr: out = alpha * (g - t), alpha = in, t the fold of alpha * g over the non-empty slots.  +0.0 for every empty slot.
// g.C is not read.  One launch.
void launch_pixel_softmax(const PixelGeom& g, const float* in, const float* grad, float* out, hipStream_t st);
// out[n][c][y][x] = the left fold over the non-empty slots, ascending, of weight[n][h(c)][s][y][x] * values[n][c][j].  One launch.
void launch_pixel_mix(const PixelGeom& g, const float* values, const float* weight, float* out, hipStream_t st);
// out[n][c][j] = the exact sum, rounded once, of the tile partials of weight * x whose slot names node j (rule 4 of pixels.py);
// `acc` is the zeroed accumulator.  Two launches.
void launch_pixel_scatter(const PixelGeom& g, const float* x, const float* weight, void* acc, float* out, hipStream_t st);

}  // namespace fslic
