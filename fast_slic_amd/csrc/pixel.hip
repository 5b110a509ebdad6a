// pixel.hip -- pixels over neighbour lists, gfx950 (fast_slic_amd/pixels.py states the rules; layout, slots, checks and the launch
// shapes are pixel.h's).
//   k_pixel_dot             : one thread per pixel; per head four slots at a time, the channels of the head in ascending order.
//   k_pixel_mix             : one thread per pixel; per head four channels at a time, the slots in ascending order.
//   k_pixel_softmax<false>  : one thread per (pixel, head).  Three walks of the S planes: the maximum; e = crf_expf(s - m) into the
//                             place of the result and the fold Z of e; e / Z.
//   k_pixel_softmax<true>   : the same item; t = the fold of alpha * g, then alpha * (g - t).
//   k_pixel_scatter_tiles   : k_pool_tiles' item and label analysis (pool.hip); per 64 listed labels and slot the node of every
//                             label once, a slot that no listed label fills is skipped; per channel the lane's 16 products, per label
//                             the column sum in row order and the DPP tree, lane d keeps the partial of label d, one fix_add each.
//   k_pixel_scatter_finalize: accumulator -> out [N][C][K], one rounding.
// This file is compiled with -ffp-contract=off: every product, sum, difference and quotient is one IEEE float operation rounded on its
// own, and the division is HIP's correctly rounded one (crf_expf writes its fused operations out, as in attend.hip).  The only
// atomics are fix_add's 64-bit integer adds: no float atomics, and no kernel waits for another block.
#include "device_common.h"
#include "pixel.h"
#include "lists.h"   // row_bound
#include "crf.h"         // crf_expf
#include "fixsum.h"      // fix_add, fix_to_float
#include <algorithm>
#include <type_traits>

namespace fslic {

namespace {

constexpr int kPixRows = 16;               // rows of a scatter tile: pool.hip's kPoolRows
constexpr int kPixMaxList = 64 * kPixRows;

// The node of slot s < S of a pixel of label i (K: no label) whose row has the clamped bounds [lo, hi): K for an empty slot.
// lo <= nnz < 2^31 and s <= 31: the entry number does not wrap as an unsigned.
static __device__ __forceinline__ uint32_t slot_node(uint32_t i, int s, int lo, int hi, const int32_t* __restrict__ indices, uint32_t K) {
    if (i >= K) return K;
    if (s == 0) return i;
    const uint32_t p = (uint32_t)lo + (uint32_t)(s - 1);
    if (p >= (uint32_t)hi) return K;                                 // hi >= 0; an end before its start is an empty row
    const uint32_t j = (uint32_t)indices[p];
    return j < K ? j : K;
}

// the clamped bounds of the row of label i < K in frame f; an empty row for a pixel without a label
static __device__ __forceinline__ void row_of(const long long* __restrict__ offsets, uint32_t f, uint32_t i, uint32_t K, int nnz, int& lo, int& hi) {
    lo = hi = 0;
    if (i < K) {
        lo = row_bound(offsets, f * K + i, nnz);
        hi = row_bound(offsets, f * K + i + 1u, nnz);
    }
}

template <class L>
__global__ __launch_bounds__(256) void k_pixel_dot(const L* __restrict__ labels, const long long* __restrict__ offsets,
                                                   const int32_t* __restrict__ indices, const float* __restrict__ a, const float* __restrict__ b,
                                                   float* __restrict__ out, int C, int D, int heads, int S, uint32_t HW, uint32_t K, int nnz,
                                                   uint32_t total) {
    // total = N * H * W < 2^31, and a round of the grid is at most 2^21 threads: q does not wrap
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
        const uint32_t f = q / HW, p = q - f * HW;
        const uint32_t i = canon(labels[q], K);
        int lo, hi;
        row_of(offsets, f, i, K, nnz, lo, hi);
        const float* __restrict__ af = a + (size_t)f * (size_t)C * HW + p;
        const float* __restrict__ bf = b + (size_t)f * (size_t)C * K;
        float* __restrict__ of = out + (size_t)f * (size_t)heads * (size_t)S * HW + p;
        for (int h = 0; h < heads; ++h) {
            const float* __restrict__ ah = af + (size_t)h * (size_t)D * HW;
            const float* __restrict__ bh = bf + (size_t)h * (size_t)D * K;
            for (int s0 = 0; s0 < S; s0 += 4) {
                uint32_t j[4];
                float acc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    j[u] = s0 + u < S ? slot_node(i, s0 + u, lo, hi, indices, K) : K;
                    acc[u] = 0.0f;
                }
                if (j[0] < K || j[1] < K || j[2] < K || j[3] < K) {
                    for (int c = 0; c < D; ++c) {
                        const float av = ah[(size_t)c * HW];
                        const float* __restrict__ bc = bh + (size_t)c * K;
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (j[u] < K) acc[u] = acc[u] + av * bc[j[u]];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (s0 + u < S) of[((size_t)h * (size_t)S + (size_t)(s0 + u)) * HW] = acc[u];
            }
        }
    }
}

template <class L>
__global__ __launch_bounds__(256) void k_pixel_mix(const L* __restrict__ labels, const long long* __restrict__ offsets,
                                                   const int32_t* __restrict__ indices, const float* __restrict__ values,
                                                   const float* __restrict__ weight, float* __restrict__ out, int C, int D, int heads, int S,
                                                   uint32_t HW, uint32_t K, int nnz, uint32_t total) {
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
        const uint32_t f = q / HW, p = q - f * HW;
        const uint32_t i = canon(labels[q], K);
        int lo, hi;
        row_of(offsets, f, i, K, nnz, lo, hi);
        const float* __restrict__ vf = values + (size_t)f * (size_t)C * K;
        const float* __restrict__ wf = weight + (size_t)f * (size_t)heads * (size_t)S * HW + p;
        float* __restrict__ of = out + (size_t)f * (size_t)C * HW + p;
        for (int h = 0; h < heads; ++h) {
            const float* __restrict__ wh = wf + (size_t)h * (size_t)S * HW;
            const int cend = (h + 1) * D;
            for (int c0 = h * D; c0 < cend; c0 += 4) {
                float acc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = 0.0f;
                for (int s = 0; s < S; ++s) {
                    const uint32_t j = slot_node(i, s, lo, hi, indices, K);
                    if (j >= K) continue;
                    const float w = wh[(size_t)s * HW];
                    const float* __restrict__ vc = vf + (size_t)c0 * K + j;
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (c0 + u < cend) acc[u] = acc[u] + w * vc[(size_t)u * K];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (c0 + u < cend) of[(size_t)(c0 + u) * HW] = acc[u];
            }
        }
    }
}

// `out` is read back by the thread that wrote it (the forward's third walk): it is not __restrict__
template <bool BACK, class L>
__global__ __launch_bounds__(256) void k_pixel_softmax(const L* __restrict__ labels, const long long* __restrict__ offsets,
                                                       const int32_t* __restrict__ indices, const float* __restrict__ in,
                                                       const float* __restrict__ grad, float* out, uint32_t heads, int S, uint32_t HW, uint32_t K,
                                                       int nnz, uint32_t total) {
    // total = N * heads * H * W < 2^31
    const uint32_t per = heads * HW;                                                   // <= total
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
        const uint32_t f = q / per, r = q - f * per, h = r / HW, p = r - h * HW;
        const uint32_t i = canon(labels[(size_t)f * HW + p], K);
        int lo, hi;
        row_of(offsets, f, i, K, nnz, lo, hi);
        uint32_t full = 0u;                                                            // bit s: slot s is not empty
        for (int s = 0; s < S; ++s) full |= (slot_node(i, s, lo, hi, indices, K) < K ? 1u : 0u) << s;
        const size_t base = ((size_t)f * heads + h) * (size_t)S * HW + p;
        const float* __restrict__ ip = in + base;
        float* op = out + base;
        if (!BACK) {
            float m = -INFINITY;
            for (int s = 0; s < S; ++s) {
                if (!((full >> s) & 1u)) continue;
                const float v = ip[(size_t)s * HW];
                m = v > m ? v : m;
            }
            float Z = 0.0f;
            for (int s = 0; s < S; ++s) {
                float e = 0.0f;
                if ((full >> s) & 1u) {
                    e = crf_expf(ip[(size_t)s * HW] - m);
                    Z = Z + e;
                }
                op[(size_t)s * HW] = e;
            }
            for (int s = 0; s < S; ++s)
                if ((full >> s) & 1u) op[(size_t)s * HW] = op[(size_t)s * HW] / Z;     // this thread's own store of the walk before
        } else {
            const float* __restrict__ gp = grad + base;
            float t = 0.0f;
            for (int s = 0; s < S; ++s)
                if ((full >> s) & 1u) t = t + ip[(size_t)s * HW] * gp[(size_t)s * HW];
            for (int s = 0; s < S; ++s) {
                float v = 0.0f;
                if ((full >> s) & 1u) v = ip[(size_t)s * HW] * (gp[(size_t)s * HW] - t);
                op[(size_t)s * HW] = v;
            }
        }
    }
}

// pool.hip's k_pool_tiles with a weight and S destinations a label.  The label analysis is the same: the distinct labels in order of
// first appearance, each with the rows that hold it, in LDS.  Then per 64 listed labels, lane d < dn owning label d of them: per slot
// the node of the lane's label (K where the slot is empty); per channel of the chunk the lane's products w * x of its 16 pixels (the
// weight plane of a slot and head is loaded once and serves the head's channels of the chunk); per label the sum of the lane's pixels
// of that label in row order (from -0.0, adding -0.0 for the others: exactly the sum of the label's products) and the DPP tree.
template <class L>
__global__ __launch_bounds__(256) void k_pixel_scatter_tiles(const float* __restrict__ x, const float* __restrict__ weight, const L* __restrict__ labels,
                                                             const long long* __restrict__ offsets, const int32_t* __restrict__ indices,
                                                             unsigned long long* __restrict__ acc, int N, int C, int D, int heads, int S, int H, int W,
                                                             uint32_t K, int nnz, int nchunk, int cchunk) {
    __shared__ uint32_t s_list[4][kPixMaxList];            // per wavefront: label << 16 | rows holding it
    const int lane = LANE();
    const uint32_t wave = rfl(threadIdx.x >> 6);
    uint32_t* lst = s_list[wave];
    const unsigned long long ntx = (unsigned long long)((W + 63) / 64), nty = (unsigned long long)((H + kPixRows - 1) / kPixRows);
    const unsigned long long per = ntx * nty, nitems = per * (unsigned long long)N * (unsigned long long)nchunk;
    const unsigned long long nwaves = (unsigned long long)gridDim.x * 4ull;
    const size_t HW = (size_t)H * (size_t)W;
    for (unsigned long long it = (unsigned long long)blockIdx.x * 4ull + wave; it < nitems; it += nwaves) {
        const unsigned long long t = it / (unsigned long long)nchunk;            // the chunks of one tile are neighbours (shared label reads)
        const int chunk = (int)(it - t * (unsigned long long)nchunk);
        const int c0 = chunk * cchunk, c1 = min(C, c0 + cchunk);
        const int n = (int)(t / per);
        const unsigned long long tt = t - (unsigned long long)n * per;
        const int ty = (int)(tt / ntx), tx = (int)(tt - (unsigned long long)ty * ntx);
        const int px = tx * 64 + lane, y0 = ty * kPixRows;
        const bool okx = px < W;
        const int nrows = min(kPixRows, H - y0);                      // (a row offset below stays inside the frame: < H * W < 2^31)
        const size_t p0 = (size_t)y0 * W + (size_t)min(px, W - 1);    // this lane's pixel of row 0 (flat index in the frame)
        const L* __restrict__ lb = labels + (size_t)n * HW + p0;
        uint32_t lab[kPixRows];                                       // K: no label (outside [0, K), past the image)
#pragma unroll
        for (int r = 0; r < kPixRows; ++r) {                          // rows past the image re-read the last one
            const uint32_t v = canon(lb[(uint32_t)min(r, nrows - 1) * (uint32_t)W], K);
            lab[r] = (okx && r < nrows) ? v : K;
        }
        uint32_t pend = 0;                                            // bit r: row r not yet listed
#pragma unroll
        for (int r = 0; r < kPixRows; ++r) pend |= (lab[r] < K ? 1u : 0u) << r;
        wave_lds_sync();                                              // every lane has read the previous tile's list
        int nlab = 0;
        for (;;) {
            const unsigned long long any = ballot(pend != 0u);
            if (!any) break;
            uint32_t first = K;
#pragma unroll
            for (int r = kPixRows - 1; r >= 0; --r) first = ((pend >> r) & 1u) ? lab[r] : first;
            const uint32_t cur = (uint32_t)__builtin_amdgcn_readlane((int)first, (int)__builtin_ctzll(any));
            uint32_t mine = 0, rows = 0;
#pragma unroll
            for (int r = 0; r < kPixRows; ++r) {
                const bool m = lab[r] == cur;
                mine |= (m ? 1u : 0u) << r;
                rows |= (ballot(m) != 0ull ? 1u : 0u) << r;
            }
            pend &= ~mine;
            if (lane == 0) lst[nlab] = (cur << 16) | rows;            // nlab < 1024: a tile has at most that many pixels
            ++nlab;
        }
        wave_lds_sync();
        if (nlab == 0) continue;
        const float* __restrict__ xb = x + ((size_t)n * (size_t)C) * HW + p0;
        const float* __restrict__ wb = weight + ((size_t)n * (size_t)heads * (size_t)S) * HW + p0;
        for (int d0 = 0; d0 < nlab; d0 += 64) {
            const int dn = min(64, nlab - d0);
            const uint32_t ent = lst[d0 + min(lane, dn - 1)];
            const uint32_t k = ent >> 16;                             // < K: listed labels passed canon()
            int lo, hi;
            row_of(offsets, (uint32_t)n, k, K, nnz, lo, hi);
            for (int s = 0; s < S; ++s) {
                const uint32_t node = lane < dn ? slot_node(k, s, lo, hi, indices, K) : K;
                const unsigned long long filled = ballot(node < K);  // bit d: label d has this slot
                if (!filled) continue;
                int hprev = -1;
                float wv[kPixRows];
                for (int c = c0; c < c1; ++c) {
                    const int h = c / D;
                    if (h != hprev) {                                 // (the same in every lane)
                        const float* __restrict__ wp = wb + ((size_t)h * (size_t)S + (size_t)s) * HW;
#pragma unroll
                        for (int r = 0; r < kPixRows; ++r) wv[r] = wp[(uint32_t)min(r, nrows - 1) * (uint32_t)W];
                        hprev = h;
                    }
                    const float* __restrict__ xp = xb + (size_t)c * HW;
                    float prod[kPixRows];
#pragma unroll
                    for (int r = 0; r < kPixRows; ++r) prod[r] = wv[r] * xp[(uint32_t)min(r, nrows - 1) * (uint32_t)W];
                    float part = -0.0f;
                    for (int dd = 0; dd < dn; ++dd) {
                        if (!((filled >> dd) & 1ull)) continue;       // (the same in every lane)
                        const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)ent, dd);
                        const uint32_t cur = e >> 16, rows = e & 0xFFFFu;
                        float v = -0.0f;
#pragma unroll
                        for (int r = 0; r < kPixRows; ++r)
                            if ((rows >> r) & 1u) v += lab[r] == cur ? prod[r] : -0.0f;
                        const float sum = wave_reduce_add<float>(v);
                        part = lane == dd ? sum : part;
                    }
                    // node < K: checked, and the accumulator of (n, c) has K cells a limb
                    if (node < K) fix_add(acc + ((size_t)n * C + c) * (size_t)kPoolLimbs * K + node, (size_t)K, part);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_pixel_scatter_finalize(const unsigned long long* __restrict__ acc, float* __restrict__ out, uint32_t K,
                                                                uint32_t total) {
    // total = N * C * K < 2^31
    for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < total; q += gridDim.x * 256u) {
        const uint32_t nc = q / K, k = q - nc * K;
        out[q] = fix_to_float(acc + (size_t)nc * (size_t)kPoolLimbs * K + k, (size_t)K);
    }
}

// the items of the scatter: pool.hip's rule (about kItems items, chunks of at least kMinChunk channels)
constexpr unsigned long long kPixItems = 256ull * 28ull * 4ull;
constexpr int kPixMinChunk = 4;

}  // namespace

void launch_pixel_dot(const PixelGeom& g, const float* a, const float* b, float* out, hipStream_t st) {
    const unsigned long long HW = (unsigned long long)g.H * (unsigned long long)g.W, total = HW * (unsigned long long)g.N;
    const dim3 grid((unsigned)tile_grid(total, 256)), block(256);
    with_label_type(g.labels, g.label_type, [&](auto* lab) {
        launch(k_pixel_dot<std::remove_cv_t<std::remove_pointer_t<decltype(lab)>>>, grid, block, 0, st, lab, g.offsets, g.indices, a, b, out, g.C,
               g.C / g.heads, g.heads, g.S, (uint32_t)HW, (uint32_t)g.K, (int)g.nnz, (uint32_t)total);
    });
}

void launch_pixel_mix(const PixelGeom& g, const float* values, const float* weight, float* out, hipStream_t st) {
    const unsigned long long HW = (unsigned long long)g.H * (unsigned long long)g.W, total = HW * (unsigned long long)g.N;
    const dim3 grid((unsigned)tile_grid(total, 256)), block(256);
    with_label_type(g.labels, g.label_type, [&](auto* lab) {
        launch(k_pixel_mix<std::remove_cv_t<std::remove_pointer_t<decltype(lab)>>>, grid, block, 0, st, lab, g.offsets, g.indices, values, weight, out,
               g.C, g.C / g.heads, g.heads, g.S, (uint32_t)HW, (uint32_t)g.K, (int)g.nnz, (uint32_t)total);
    });
}

void launch_pixel_softmax(const PixelGeom& g, const float* in, const float* grad, float* out, hipStream_t st) {
    const unsigned long long HW = (unsigned long long)g.H * (unsigned long long)g.W;
    const unsigned long long total = HW * (unsigned long long)g.N * (unsigned long long)g.heads;
    const dim3 grid((unsigned)tile_grid(total, 256)), block(256);
    with_label_type(g.labels, g.label_type, [&](auto* lab) {
        using L = std::remove_cv_t<std::remove_pointer_t<decltype(lab)>>;
        if (grad)
            launch(k_pixel_softmax<true, L>, grid, block, 0, st, lab, g.offsets, g.indices, in, grad, out, (uint32_t)g.heads, g.S, (uint32_t)HW,
                   (uint32_t)g.K, (int)g.nnz, (uint32_t)total);
        else
            launch(k_pixel_softmax<false, L>, grid, block, 0, st, lab, g.offsets, g.indices, in, grad, out, (uint32_t)g.heads, g.S, (uint32_t)HW,
                   (uint32_t)g.K, (int)g.nnz, (uint32_t)total);
    });
}

void launch_pixel_scatter(const PixelGeom& g, const float* x, const float* weight, void* workspace, float* out, hipStream_t st) {
    const unsigned long long tiles =
        (unsigned long long)g.N * (unsigned long long)((g.W + 63) / 64) * (unsigned long long)((g.H + kPixRows - 1) / kPixRows);
    const unsigned long long most = (unsigned long long)(g.C + kPixMinChunk - 1) / kPixMinChunk;
    const int want = (int)std::min<unsigned long long>(most, std::max<unsigned long long>(1ull, (kPixItems + tiles - 1) / tiles));
    const int cchunk = (g.C + want - 1) / want, nchunk = (g.C + cchunk - 1) / cchunk;
    const unsigned long long items = tiles * (unsigned long long)nchunk;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(workspace);
    with_label_type(g.labels, g.label_type, [&](auto* lab) {
        launch(k_pixel_scatter_tiles<std::remove_cv_t<std::remove_pointer_t<decltype(lab)>>>, dim3((unsigned)tile_grid(items, 4)), dim3(256), 0, st, x,
               weight, lab, g.offsets, g.indices, acc, g.N, g.C, g.C / g.heads, g.heads, g.S, g.H, g.W, (uint32_t)g.K, (int)g.nnz, nchunk, cchunk);
    });
    const unsigned long long total = (unsigned long long)g.N * (unsigned long long)g.C * (unsigned long long)g.K;
    launch(k_pixel_scatter_finalize, dim3((unsigned)tile_grid(total, 256)), dim3(256), 0, st, acc, out, (uint32_t)g.K, (uint32_t)total);
}

}  // namespace fslic
