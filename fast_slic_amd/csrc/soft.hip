// soft.hip -- soft superpixel assignment of float feature planes over a regular seed grid, gfx950 (fast_slic_amd/soft.py; soft.h has
// the geometry).
//   k_soft_assign     : one thread per pixel: per channel one coalesced feature load and nine gathers from the frame's [C][K] centre
//                       table (read-only, neighbouring pixels share their nine centres: served by the caches); nine Q planes out
//   k_soft_assign_bwd : one thread per pixel: gd from Q and gQ, then per channel gF = 2 sum_j gd_j (F - S_j)
//   k_soft_pool       : one block per (frame, superpixel k, chunk of kSoftChunk channels): the block walks the pixels of k's 3 x 3 cell
//                       window row by row in pieces of kSoftStage pixels; a piece's weights Q_{j_k(p)}(p) and pixel offsets are staged
//                       in LDS once and every channel of the chunk is then summed over them.  With centres it sums w (F - S[k]).
//   k_soft_unpool     : one thread per pixel: out[c][p] = sum_j Q_j(p) V[c][k_j]
//   k_soft_dot        : one thread per pixel: out_j(p) = sum_c A[c][p] B[c][k_j] (+ bias[k_j])
// Determinism: no atomics.  A pixel kernel's sums run in ascending slot or channel order inside one thread.  In k_soft_pool, element e
// of the window (row-major in the window's rectangle, which depends on H, W, gh, gw and k alone) always belongs to thread
// (e % kSoftStage) % 256, a thread adds its elements in ascending e, a wavefront's 64 sums meet in wave_reduce_add's fixed tree and
// the four wavefronts in (w0 + w1) + (w2 + w3).  A channel's sum never meets another channel's, so neither the other channels nor the
// chunk a channel falls into can change a bit.  Every gather index is checked against the grid before use.
#include "device_common.h"
#include "soft.h"

namespace fslic {

// wide: (y * gh) or (x * gw) can pass 2^32 (H * W < 2^31 does not bound H * gh), so the cell needs a 64-bit division
struct SoftGrid { uint32_t H, W, gh, gw, wide; };

static SoftGrid soft_grid(int H, int W, int gh, int gw) {
    SoftGrid g;
    g.H = (uint32_t)H; g.W = (uint32_t)W; g.gh = (uint32_t)gh; g.gw = (uint32_t)gw;
    g.wide = ((unsigned long long)H * gh > 0xFFFFFFFFull || (unsigned long long)W * gw > 0xFFFFFFFFull) ? 1u : 0u;
    return g;
}

// cell of pixel v on an axis of L pixels and g cells
static __device__ __forceinline__ uint32_t cell_of(uint32_t v, uint32_t g, uint32_t L, uint32_t wide) {
    return wide ? (uint32_t)(((unsigned long long)v * g) / L) : (v * g) / L;
}
// first pixel of cell c (c == g: L)
static __device__ __forceinline__ uint32_t cell_start(uint32_t c, uint32_t g, uint32_t L) {
    return (uint32_t)(((unsigned long long)c * L + g - 1u) / g);
}

// the nine slots of pixel p: k[j] is a checked index (0 where the slot is invalid), bit j of the result says whether slot j is valid
static __device__ __forceinline__ uint32_t soft_slots(const SoftGrid& g, uint32_t p, uint32_t (&k)[9]) {
    const uint32_t y = p / g.W, x = p - y * g.W;
    const int cy = (int)cell_of(y, g.gh, g.H, g.wide), cx = (int)cell_of(x, g.gw, g.W, g.wide);
    uint32_t ok = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int ny = cy + j / 3 - 1, nx = cx + j % 3 - 1;
        const bool in = ny >= 0 && ny < (int)g.gh && nx >= 0 && nx < (int)g.gw;
        k[j] = in ? (uint32_t)ny * g.gw + (uint32_t)nx : 0u;
        ok |= in ? 1u << j : 0u;
    }
    return ok;
}

// `first`: the flat block index of the launch's block 0 (launch_sliced)
#define SOFT_PIXEL()                                                           \
    const uint32_t blk = first + blockIdx.x, n = blk / bpf, p = (blk - n * bpf) * 256u + threadIdx.x; \
    if (p >= HW) return;                                                       \
    uint32_t k[9];                                                             \
    const uint32_t ok = soft_slots(g, p, k)

__global__ __launch_bounds__(256) void k_soft_assign(const float* __restrict__ feat, const float* __restrict__ cen, float* __restrict__ q,
                                                     SoftGrid g, int C, uint32_t HW, uint32_t K, uint32_t bpf, uint32_t first) {
    SOFT_PIXEL();
    const float* __restrict__ f = feat + (size_t)n * C * HW + p;
    const float* __restrict__ s = cen + (size_t)n * C * K;
    float d[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) d[j] = 0.0f;
    for (int c = 0; c < C; ++c, f += HW, s += K) {
        const float v = *f;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const float t = v - s[k[j]];
            d[j] += t * t;
        }
    }
    float m = d[4];                                    // slot 4, the pixel's own cell, is always valid
#pragma unroll
    for (int j = 0; j < 9; ++j) if ((ok >> j) & 1u) m = fminf(m, d[j]);
    float e[9], sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        e[j] = 0.0f;
        if ((ok >> j) & 1u) { e[j] = expf(-(d[j] - m)); sum += e[j]; }
    }
    float* __restrict__ o = q + (size_t)n * 9u * HW + p;
#pragma unroll
    for (int j = 0; j < 9; ++j) st_stream(o + (size_t)j * HW, ((ok >> j) & 1u) ? e[j] / sum : 0.0f);
}

__global__ __launch_bounds__(256) void k_soft_assign_bwd(const float* __restrict__ feat, const float* __restrict__ cen,
                                                         const float* __restrict__ q, const float* __restrict__ gq, float* __restrict__ gd,
                                                         float* __restrict__ gfeat, SoftGrid g, int C, uint32_t HW, uint32_t K, uint32_t bpf,
                                                         uint32_t first) {
    SOFT_PIXEL();
    const size_t qoff = (size_t)n * 9u * HW + p;
    float qq[9], gg[9], dot = 0.0f;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        qq[j] = 0.0f; gg[j] = 0.0f;
        if ((ok >> j) & 1u) { qq[j] = q[qoff + (size_t)j * HW]; gg[j] = gq[qoff + (size_t)j * HW]; dot += gg[j] * qq[j]; }
    }
    float w[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        w[j] = ((ok >> j) & 1u) ? -qq[j] * (gg[j] - dot) : 0.0f;
        st_stream(gd + qoff + (size_t)j * HW, w[j]);
    }
    const float* __restrict__ f = feat + (size_t)n * C * HW + p;
    const float* __restrict__ s = cen + (size_t)n * C * K;
    float* __restrict__ o = gfeat + (size_t)n * C * HW + p;
    for (int c = 0; c < C; ++c, f += HW, s += K, o += HW) {
        const float v = *f;
        float a = 0.0f;
#pragma unroll
        for (int j = 0; j < 9; ++j) if ((ok >> j) & 1u) a += w[j] * (v - s[k[j]]);
        __builtin_nontemporal_store(2.0f * a, o);
    }
}

__global__ __launch_bounds__(256) void k_soft_unpool(const float* __restrict__ values, const float* __restrict__ q, float* __restrict__ out,
                                                     SoftGrid g, int C, uint32_t HW, uint32_t K, uint32_t bpf, uint32_t first) {
    SOFT_PIXEL();
    const size_t qoff = (size_t)n * 9u * HW + p;
    float qq[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) qq[j] = ((ok >> j) & 1u) ? q[qoff + (size_t)j * HW] : 0.0f;
    const float* __restrict__ v = values + (size_t)n * C * K;
    float* __restrict__ o = out + (size_t)n * C * HW + p;
    for (int c = 0; c < C; ++c, v += K, o += HW) {
        float a = 0.0f;
#pragma unroll
        for (int j = 0; j < 9; ++j) if ((ok >> j) & 1u) a += qq[j] * v[k[j]];
        __builtin_nontemporal_store(a, o);
    }
}

__global__ __launch_bounds__(256) void k_soft_dot(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ bias,
                                                  float* __restrict__ out, SoftGrid g, int C, uint32_t HW, uint32_t K, uint32_t bpf,
                                                  uint32_t first) {
    SOFT_PIXEL();
    const float* __restrict__ f = a + (size_t)n * C * HW + p;
    const float* __restrict__ t = b + (size_t)n * C * K;
    float acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = 0.0f;
    for (int c = 0; c < C; ++c, f += HW, t += K) {
        const float v = *f;
#pragma unroll
        for (int j = 0; j < 9; ++j) acc[j] += v * t[k[j]];
    }
    float* __restrict__ o = out + (size_t)n * 9u * HW + p;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        float r = 0.0f;
        if ((ok >> j) & 1u) r = bias ? acc[j] + bias[(size_t)n * K + k[j]] : acc[j];
        st_stream(o + (size_t)j * HW, r);
    }
}

// One staged piece of a window: a thread takes its elements in ascending order and, per element, every channel of the chunk -- the
// chunk's loads of one pixel are in flight together (a channel-by-channel walk waits for one gather per step: measured 3.37 ms against
// 0.61 ms at 8 x 1280x720, C = 20), and a channel's sum still adds its elements in the same order.
template <bool kCentred, bool kFull>
static __device__ __forceinline__ void soft_pool_piece(const float* s_w, const uint32_t* s_p, uint32_t cnt, uint32_t tid,
                                                       const float* __restrict__ fn, uint32_t HW, const float (&sc)[kSoftChunk], int nc,
                                                       float (&acc)[kSoftChunk], float& wacc) {
#pragma unroll 2
    for (uint32_t i = tid; i < cnt; i += 256u) {
        const float w = s_w[i];
        const float* __restrict__ f = fn + s_p[i];
        float v[kSoftChunk];
#pragma unroll
        for (int c = 0; c < kSoftChunk; ++c) v[c] = (kFull || c < nc) ? f[(size_t)c * HW] : 0.0f;
#pragma unroll
        for (int c = 0; c < kSoftChunk; ++c)
            if (kFull || c < nc) acc[c] += kCentred ? w * (v[c] - sc[c]) : w * v[c];
        wacc += w;
    }
}

template <bool kCentred>
__global__ __launch_bounds__(256) void k_soft_pool(const float* __restrict__ feat, const float* __restrict__ q, const float* __restrict__ cen,
                                                   float* __restrict__ sums, float* __restrict__ weights, SoftGrid g, int C, uint32_t HW,
                                                   uint32_t K, uint32_t nchunk, uint32_t first) {
    __shared__ float s_w[kSoftStage];
    __shared__ uint32_t s_p[kSoftStage];
    __shared__ float s_part[4][kSoftChunk + 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t item = first + blockIdx.x, chunk = item % nchunk, nk = item / nchunk, k = nk % K, n = nk / K;
    const uint32_t cy = k / g.gw, cx = k - cy * g.gw;
    // the window: the cells (cy - 1 .. cy + 1) x (cx - 1 .. cx + 1) inside the grid, as a pixel rectangle; yb1, yb2 (xb1, xb2) are
    // the first rows (columns) of k's own cell and of the cell behind it
    const uint32_t ry0 = cell_start(cy > 0u ? cy - 1u : 0u, g.gh, g.H), ry1 = cell_start(min(cy + 2u, g.gh), g.gh, g.H);
    const uint32_t rx0 = cell_start(cx > 0u ? cx - 1u : 0u, g.gw, g.W), rx1 = cell_start(min(cx + 2u, g.gw), g.gw, g.W);
    const uint32_t yb1 = cell_start(cy, g.gh, g.H), yb2 = cell_start(cy + 1u, g.gh, g.H);
    const uint32_t xb1 = cell_start(cx, g.gw, g.W), xb2 = cell_start(cx + 1u, g.gw, g.W);
    const uint32_t wx = rx1 - rx0, total = (ry1 - ry0) * wx;              // <= H * W < 2^31
    const int c0 = (int)chunk * kSoftChunk, nc = min(kSoftChunk, C - c0);
    const float* __restrict__ qn = q + (size_t)n * 9u * HW;
    const float* __restrict__ fn = feat + ((size_t)n * C + c0) * HW;
    float acc[kSoftChunk], sc[kSoftChunk], wacc = 0.0f;
#pragma unroll
    for (int c = 0; c < kSoftChunk; ++c) {
        acc[c] = 0.0f;
        sc[c] = kCentred && c < nc ? cen[((size_t)n * C + c0 + c) * K + k] : 0.0f;
    }
    for (uint32_t base = 0; base < total; base += kSoftStage) {
        const uint32_t cnt = min((uint32_t)kSoftStage, total - base);
        __syncthreads();                                                   // the previous piece has been summed
        for (uint32_t i = tid; i < cnt; i += 256u) {
            const uint32_t e = base + i, r = e / wx, y = ry0 + r, x = rx0 + (e - r * wx);
            // the slot of pixel (y, x) that names k: dy = cy - (the pixel's cell row), dx likewise
            const uint32_t jy = y < yb1 ? 2u : y < yb2 ? 1u : 0u, jx = x < xb1 ? 2u : x < xb2 ? 1u : 0u;
            const uint32_t p = y * g.W + x;
            s_p[i] = p;
            s_w[i] = qn[(size_t)(3u * jy + jx) * HW + p];
        }
        __syncthreads();
        if (nc == kSoftChunk) soft_pool_piece<kCentred, true>(s_w, s_p, cnt, tid, fn, HW, sc, nc, acc, wacc);
        else soft_pool_piece<kCentred, false>(s_w, s_p, cnt, tid, fn, HW, sc, nc, acc, wacc);
    }
    const uint32_t wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < kSoftChunk; ++c) {
        const float v = wave_reduce_add(acc[c]);
        if (LANE() == 0) s_part[wave][c] = v;
    }
    {
        const float v = wave_reduce_add(wacc);
        if (LANE() == 0) s_part[wave][kSoftChunk] = v;
    }
    __syncthreads();
    if ((int)tid < nc) sums[((size_t)n * C + c0 + tid) * K + k] = (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]);
    if (tid == (uint32_t)kSoftChunk && chunk == 0u && weights)
        weights[(size_t)n * K + k] = (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]);
}

// ---- launches (the entries of softapi.cpp have checked every argument: N * ceil(H W / 256) and the pool items are below 2^31) ----
// One block per item, issued through launch_sliced (launch.h; soft.h has the rule and why): a kernel's last argument is the flat index of
// its slice's first block, so every block computes exactly what it would in a single launch.

#define SOFT_PIXEL_GRID()                                                  \
    const uint32_t HW = (uint32_t)H * (uint32_t)W, bpf = (HW + 255u) / 256u; \
    const unsigned long long blocks = (unsigned long long)bpf * (unsigned long long)N; \
    const SoftGrid g = soft_grid(H, W, gh, gw);                            \
    const uint32_t K = (uint32_t)gh * (uint32_t)gw

void launch_soft_assign(const float* feat, const float* centres, float* q, int N, int C, int H, int W, int gh, int gw, hipStream_t st) {
    SOFT_PIXEL_GRID();
    launch_sliced(k_soft_assign, blocks, st, feat, centres, q, g, C, HW, K, bpf);
}

void launch_soft_assign_bwd(const float* feat, const float* centres, const float* q, const float* gq, float* gd, float* gfeat,
                            int N, int C, int H, int W, int gh, int gw, hipStream_t st) {
    SOFT_PIXEL_GRID();
    launch_sliced(k_soft_assign_bwd, blocks, st, feat, centres, q, gq, gd, gfeat, g, C, HW, K, bpf);
}

void launch_soft_unpool(const float* values, const float* q, float* out, int N, int C, int H, int W, int gh, int gw, hipStream_t st) {
    SOFT_PIXEL_GRID();
    launch_sliced(k_soft_unpool, blocks, st, values, q, out, g, C, HW, K, bpf);
}

void launch_soft_dot(const float* a, const float* b, const float* bias, float* out, int N, int C, int H, int W, int gh, int gw, hipStream_t st) {
    SOFT_PIXEL_GRID();
    launch_sliced(k_soft_dot, blocks, st, a, b, bias, out, g, C, HW, K, bpf);
}

void launch_soft_pool(const float* feat, const float* q, const float* centres, float* sums, float* weights,
                      int N, int C, int H, int W, int gh, int gw, hipStream_t st) {
    const uint32_t HW = (uint32_t)H * (uint32_t)W, K = (uint32_t)gh * (uint32_t)gw, nchunk = (uint32_t)((C + kSoftChunk - 1) / kSoftChunk);
    const unsigned long long items = soft_pool_items(N, C, (int)K);
    const SoftGrid g = soft_grid(H, W, gh, gw);
    if (centres) launch_sliced(k_soft_pool<true>, items, st, feat, q, centres, sums, weights, g, C, HW, K, nchunk);
    else launch_sliced(k_soft_pool<false>, items, st, feat, q, centres, sums, weights, g, C, HW, K, nchunk);
}

}  // namespace fslic
