// connect.hip -- connectivity on label tensors, gfx950 (fast_slic_amd/connect.py): the 4-connected components of equal labels,
// numbered by their first pixel in raster order, and the merge of the components below a minimum area.  Layout of the scratch:
// connect.h.  One call is eight launches on the caller's stream; a launch only reads what an earlier launch completed, except for
// the words named below, which move one way (a parent only ever becomes a smaller pixel of the same component, a link only ever
// becomes an earlier link of its chain or the final label), so that a reader is right with the old value and with the new one.
//   k_connect_tiles   : per tile of 64 columns x 16 rows one block.  The labels are read once, coalesced at their own width, into
//                       LDS; the horizontal runs of a row are one ballot; the vertical unions (one per pair of touching runs) are
//                       CAS on a union-find in LDS whose root is the smallest index; the pixels of every run go to the tile root
//                       as ONE LDS add.  Out: parent = the tile component's first pixel, area = its pixels there and 0 elsewhere.
//   k_connect_seams   : one thread per pixel pair across a tile edge; the unions are CAS on `parent` in global memory (a root is
//                       only ever given a smaller parent, so the root of a component is its leader whatever the order).
//   k_connect_flatten : parent = leader for every pixel; every tile component adds its area to its leader's: one integer atomic per
//                       tile and component (a constant map: one per tile, not one per pixel).
//   k_connect_count, k_connect_scan, k_connect_apply : the rank of the numbered leaders (components: all; enforce: area >= min_size)
//                       as a prefix sum in three launches: per chunk of 1024 pixels the count, per frame the scan of the counts,
//                       per chunk the ranks.  apply leaves at every leader its label, or (enforce, rule 4) the leader to take it from.
//   k_connect_chain   : rule 4 by pointer jumping in place: a leader replaces its link by what it finds there until that is a label.
//                       A link names a smaller index than its owner, so every walk ends; what others have resolved or shortened is used.
//   k_connect_output  : out = the label at the pixel's leader.
// No kernel waits for another block.  All integer work: the result is the same bits from run to run.
#include "device_common.h"
#include "labels.h"
#include "connect.h"

namespace fslic {

static_assert(kConnectTileRows == 16 && kConnectChunk == 1024, "256 threads: four rows of a tile and four pixels of a chunk each");

// ld_now of device_common.h for a word in LDS
static __device__ __forceinline__ uint32_t lds_now(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

static __device__ __forceinline__ uint32_t lds_find(const uint32_t* par, uint32_t a) {
    for (uint32_t q; (q = lds_now(par + a)) != a;) a = q;
    return a;
}
static __device__ __forceinline__ uint32_t find(const uint32_t* par, uint32_t a) {
    for (uint32_t q; (q = ld_now(par + a)) != a;) a = q;
    return a;
}
// Joins the sets of a and b: the larger of the two roots gets the smaller as its parent, by CAS on the root's own word.  A CAS that
// fails returns the parent another thread gave that root, and the walk goes on from there: every round ends or moves to a smaller index.
template <bool kLds>
static __device__ __forceinline__ void unite(uint32_t* par, uint32_t a, uint32_t b) {
    for (;;) {
        a = kLds ? lds_find(par, a) : find(par, a);
        b = kLds ? lds_find(par, b) : find(par, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicCAS(par + a, a, b);
        if (old == a) return;
        a = old;
    }
}

template <class L>
__global__ __launch_bounds__(256) void k_connect_tiles(const L* __restrict__ labels, uint32_t* __restrict__ parent, uint32_t* __restrict__ area,
                                                       int N, int H, int W) {
    __shared__ L s_lab[kConnectTileRows * 64];
    __shared__ uint32_t s_par[kConnectTileRows * 64];
    __shared__ uint32_t s_cnt[kConnectTileRows * 64];
    const int lane = LANE();
    const int wave = (int)rfl(threadIdx.x >> 6);
    const unsigned long long ntx = ((unsigned long long)W + 63ull) / 64ull, nty = (unsigned long long)((H + kConnectTileRows - 1) / kConnectTileRows);
    const unsigned long long per = ntx * nty, ntiles = per * (unsigned long long)N;
    const size_t HW = (size_t)H * (size_t)W;
    const unsigned long long upto = (2ull << lane) - 1ull;                 // the lanes up to this one (lane 63: all)
    for (unsigned long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const unsigned long long n = t / per, tt = t - n * per;
        const unsigned long long ty = tt / ntx, tx = tt - ty * ntx;
        const long long x = (long long)tx * 64 + lane;
        const int y0 = (int)ty * kConnectTileRows;
        const bool okx = x < (long long)W;
        const size_t base = (size_t)n * HW;
        L v[4];
        bool ok[4], same_left[4];
        uint32_t len[4];                                                   // at the first pixel of a run: its pixels
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = wave * 4 + k;
            ok[k] = okx && y0 + r < H;
            v[k] = ok[k] ? labels[base + (size_t)(y0 + r) * (size_t)W + (size_t)x] : L(0);
            s_lab[r * 64 + lane] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                      // a row is one wavefront's: its runs are one ballot
            const int i = (wave * 4 + k) * 64 + lane;
            same_left[k] = ok[k] && lane > 0 && s_lab[i - 1] == v[k];      // (a pixel left of a pixel of the image is one)
            const unsigned long long starts = ballot(!same_left[k]);      // lane 0 always starts a run; a lane outside the image is its own
            const int first = 63 - __builtin_clzll(starts & upto);
            const unsigned long long later = starts & ~upto;
            const int end = later ? __builtin_ctzll(later) : 64;
            len[k] = ok[k] && first == lane ? (uint32_t)(end - lane) : 0u;
            s_par[i] = (uint32_t)(i - lane + first);
            s_cnt[i] = len[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                      // one union per pair of runs that touch: at the pair's first column
            const int r = wave * 4 + k, i = r * 64 + lane;
            if (r > 0 && ok[k] && s_lab[i - 64] == v[k]) {
                const bool seen = same_left[k] && s_lab[i - 65] == v[k];   // the column to the left joins the same two runs
                if (!seen) unite<true>(s_par, (uint32_t)i, (uint32_t)(i - 64));
            }
        }
        __syncthreads();
        uint32_t root[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = (wave * 4 + k) * 64 + lane;
            root[k] = lds_find(s_par, (uint32_t)i);
            if (len[k] && root[k] != (uint32_t)i) atomicAdd(&s_cnt[root[k]], len[k]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = wave * 4 + k, i = r * 64 + lane;
            if (ok[k]) {
                const size_t p = (size_t)(y0 + r) * (size_t)W + (size_t)x;
                const size_t lead = (size_t)(y0 + (int)(root[k] >> 6)) * (size_t)W + (size_t)tx * 64 + (size_t)(root[k] & 63u);
                parent[base + p] = (uint32_t)lead;
                area[base + p] = root[k] == (uint32_t)i ? s_cnt[i] : 0u;
            }
        }
        __syncthreads();
    }
}

// Per frame (nty - 1) W pixel pairs across the horizontal tile edges, then (ntx - 1) H across the vertical ones.  A pair whose
// neighbouring pair INSIDE the same two tiles joins the same two runs is left to that pair (never across a tile corner: there the
// neighbouring pair may itself be left out).
template <class L>
__global__ __launch_bounds__(256) void k_connect_seams(const L* __restrict__ labels, uint32_t* parent, int N, int H, int W) {
    const unsigned long long ntx = ((unsigned long long)W + 63ull) / 64ull, nty = (unsigned long long)((H + kConnectTileRows - 1) / kConnectTileRows);
    const unsigned long long nh = (nty - 1ull) * (unsigned long long)W, per = nh + (ntx - 1ull) * (unsigned long long)H;
    const unsigned long long total = per * (unsigned long long)N;
    const size_t HW = (size_t)H * (size_t)W;
    for (unsigned long long id = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; id < total; id += (unsigned long long)gridDim.x * 256ull) {
        const unsigned long long n = id / per, e = id - n * per;
        const L* __restrict__ lab = labels + (size_t)n * HW;
        uint32_t* par = parent + (size_t)n * HW;
        size_t p, q;
        bool seen;
        if (e < nh) {
            const unsigned long long s = e / (unsigned long long)W, x = e - s * (unsigned long long)W;
            p = (size_t)(s + 1ull) * kConnectTileRows * (size_t)W + (size_t)x;
            q = p - (size_t)W;
            if (lab[p] != lab[q]) continue;
            seen = (x & 63ull) != 0ull && lab[p - 1] == lab[p] && lab[q - 1] == lab[p];
        } else {
            const unsigned long long f = e - nh, s = f / (unsigned long long)H, y = f - s * (unsigned long long)H;
            p = (size_t)y * (size_t)W + (size_t)(s + 1ull) * 64;
            q = p - 1;
            if (lab[p] != lab[q]) continue;
            seen = (y % kConnectTileRows) != 0ull && lab[p - (size_t)W] == lab[p] && lab[q - (size_t)W] == lab[p];
        }
        if (!seen) unite<false>(par, (uint32_t)p, (uint32_t)q);
    }
}

// The pixel kernels: a block takes chunks of 1024 pixels of one frame, thread t the pixels b * 1024 + k * 256 + t, k = 0 .. 3.
struct Chunk {
    size_t base;           // of the frame, in pixels
    uint32_t first;        // the chunk's first pixel in the frame
};
static __device__ __forceinline__ Chunk chunk_of(unsigned long long c, unsigned long long nb, size_t HW) {
    const unsigned long long n = c / nb;
    return Chunk{(size_t)n * HW, (uint32_t)((c - n * nb) * kConnectChunk)};
}

__global__ __launch_bounds__(256) void k_connect_flatten(uint32_t* parent, uint32_t* area, size_t HW, unsigned long long nb, unsigned long long chunks) {
    for (unsigned long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const Chunk ch = chunk_of(c, nb, HW);
        uint32_t* par = parent + ch.base;
        uint32_t a[4], lead[4], cnt[4];
        bool walk[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                      // (the loads of the four pixels are in flight together, here and in every round)
            const size_t p = (size_t)ch.first + (size_t)k * 256 + threadIdx.x;
            walk[k] = p < HW;
            a[k] = walk[k] ? ld_now(par + p) : 0u;
            cnt[k] = walk[k] ? area[ch.base + p] : 0u;                     // (only a leader's word is added to, and a leader adds nothing)
            lead[k] = a[k];
        }
        for (bool more = true; more;) {
            more = false;
            uint32_t q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = walk[k] ? ld_now(par + lead[k]) : lead[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                walk[k] = q[k] != lead[k];
                lead[k] = q[k];
                more |= walk[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t p = (size_t)ch.first + (size_t)k * 256 + threadIdx.x;
            if (p >= HW) continue;
            if (lead[k] != a[k]) st_now(par + p, lead[k]);
            if (cnt[k] && lead[k] != (uint32_t)p) atomicAdd(area + ch.base + lead[k], cnt[k]);
        }
    }
}

// is p a leader, and one that gets a number of its own?
struct Pixel { bool leader, numbered; };
static __device__ __forceinline__ Pixel classify(const uint32_t* par, const uint32_t* area, size_t p, size_t HW, uint32_t min_size) {
    Pixel r{false, false};
    if (p < HW) {
        const uint32_t a = par[p], c = area[p];
        r.leader = a == (uint32_t)p;
        r.numbered = r.leader && c >= min_size;
    }
    return r;
}

__global__ __launch_bounds__(256) void k_connect_count(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ area, uint32_t* __restrict__ sums,
                                                       size_t HW, unsigned long long nb, unsigned long long chunks, uint32_t min_size) {
    __shared__ uint32_t s_w[4];
    const int lane = LANE();
    const uint32_t wave = rfl(threadIdx.x >> 6);
    for (unsigned long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const Chunk ch = chunk_of(c, nb, HW);
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            cnt += (uint32_t)__popcll(ballot(classify(parent + ch.base, area + ch.base, (size_t)ch.first + (size_t)k * 256 + threadIdx.x, HW, min_size).numbered));
        if (lane == 0) s_w[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) sums[c] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}

// per frame one block: sums[n][b] becomes the numbered leaders of the chunks before b, counts[n] their total (at least `floor`)
__global__ __launch_bounds__(256) void k_connect_scan(uint32_t* __restrict__ sums, int32_t* __restrict__ counts, int N, unsigned long long nb, uint32_t floor) {
    __shared__ uint32_t s_w[4];
    const int lane = LANE();
    const uint32_t wave = rfl(threadIdx.x >> 6);
    for (unsigned long long n = blockIdx.x; n < (unsigned long long)N; n += gridDim.x) {
        uint32_t* s = sums + (size_t)n * (size_t)nb;
        uint32_t carry = 0;
        for (unsigned long long i0 = 0; i0 < nb; i0 += 256ull) {
            const unsigned long long i = i0 + threadIdx.x;
            const uint32_t v = i < nb ? s[i] : 0u;
            uint32_t incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t u = (uint32_t)__shfl_up((int)incl, (unsigned)d, 64);
                if (lane >= d) incl += u;
            }
            if (lane == 63) s_w[wave] = incl;
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) {
                before += w < wave ? s_w[w] : 0u;
                total += s_w[w];
            }
            if (i < nb) s[i] = carry + before + incl - v;
            carry += total;
            __syncthreads();
        }
        if (threadIdx.x == 0) counts[n] = (int32_t)(carry < floor ? floor : carry);
    }
}

__global__ __launch_bounds__(256) void k_connect_apply(const uint32_t* __restrict__ parent, uint32_t* area, const uint32_t* __restrict__ sums,
                                                       size_t HW, int W, unsigned long long nb, unsigned long long chunks, uint32_t min_size) {
    __shared__ uint32_t s_w[4][4];
    const int lane = LANE();
    const uint32_t wave = rfl(threadIdx.x >> 6);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (unsigned long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const Chunk ch = chunk_of(c, nb, HW);
        const uint32_t* par = parent + ch.base;
        uint32_t* sub = area + ch.base;
        Pixel px[4];
        uint32_t pre[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[k] = classify(par, sub, (size_t)ch.first + (size_t)k * 256 + threadIdx.x, HW, min_size);
            const unsigned long long m = ballot(px[k].numbered);
            pre[k] = (uint32_t)__popcll(m & below);
            if (lane == 0) s_w[k][wave] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        uint32_t rank = sums[c], word[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t p = (size_t)ch.first + (size_t)k * 256 + threadIdx.x;
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) {
                if (w == wave) word[k] = rank + pre[k];
                rank += s_w[k][w];
            }
            // rules 3 and 4: label 0, or that of the pixel left of (above) the leader
            if (px[k].leader && !px[k].numbered) word[k] = p == 0 ? 0u : kConnectLink | par[(uint32_t)p % (uint32_t)W ? p - 1 : p - (size_t)W];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (px[k].leader) sub[(size_t)ch.first + (size_t)k * 256 + threadIdx.x] = word[k];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_connect_chain(const uint32_t* __restrict__ parent, uint32_t* area, size_t HW, unsigned long long nb, unsigned long long chunks) {
    for (unsigned long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const Chunk ch = chunk_of(c, nb, HW);
        uint32_t* sub = area + ch.base;
        uint32_t v[4];
        bool more = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                      // (the four pixels of a thread walk together: their loads are in flight at once)
            const size_t p = (size_t)ch.first + (size_t)k * 256 + threadIdx.x;
            v[k] = p < HW && parent[ch.base + p] == (uint32_t)p ? ld_now(sub + p) : 0u;
            more |= (v[k] & kConnectLink) != 0u;
        }
        while (more) {                                                     // a link names a leader below p: its word is its label, or a link further down
            more = false;
            uint32_t q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = v[k] & kConnectLink ? ld_now(sub + (v[k] & ~kConnectLink)) : v[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (v[k] & kConnectLink) st_now(sub + (size_t)ch.first + (size_t)k * 256 + threadIdx.x, q[k]);
                v[k] = q[k];
                more |= (v[k] & kConnectLink) != 0u;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_connect_output(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ area, int32_t* __restrict__ out,
                                                        size_t HW, unsigned long long nb, unsigned long long chunks) {
    for (unsigned long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const Chunk ch = chunk_of(c, nb, HW);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t p = (size_t)ch.first + (size_t)k * 256 + threadIdx.x;
            if (p < HW) out[ch.base + p] = (int32_t)area[ch.base + parent[ch.base + p]];
        }
    }
}

// ---- launches ---------------------------------------------------------------------------------
// Every kernel strides over its items with at most tile_grid's 8192 blocks (launch.h).
void launch_connect(const void* labels, int label_type, int32_t* out, int32_t* counts, void* workspace, int N, int H, int W,
                    bool enforce, uint32_t min_size, hipStream_t st) {
    const size_t HW = (size_t)H * (size_t)W, P = (size_t)N * HW;
    const unsigned long long nb = (HW + kConnectChunk - 1) / kConnectChunk, chunks = nb * (unsigned long long)N;
    char* ws = reinterpret_cast<char*>(workspace);
    uint32_t* parent = reinterpret_cast<uint32_t*>(ws);
    uint32_t* area = reinterpret_cast<uint32_t*>(ws + connect_align(P * 4));
    uint32_t* sums = reinterpret_cast<uint32_t*>(ws + 2 * connect_align(P * 4));
    const unsigned long long ntx = ((unsigned long long)W + 63ull) / 64ull, nty = (unsigned long long)((H + kConnectTileRows - 1) / kConnectTileRows);
    const unsigned long long seams = ((nty - 1ull) * (unsigned long long)W + (ntx - 1ull) * (unsigned long long)H) * (unsigned long long)N;
    const dim3 block(256), pixels = tile_grid_dim(chunks, 1);
    if (!enforce) min_size = 0;
    with_label_type(labels, label_type, [&](auto* la) {
        using L = std::decay_t<decltype(*la)>;
        launch(k_connect_tiles<L>, tile_grid_dim(ntx * nty * (unsigned long long)N, 1), block, 0, st, la, parent, area, N, H, W);
        if (seams) launch(k_connect_seams<L>, tile_grid_dim(seams, 256), block, 0, st, la, parent, N, H, W);
    });
    launch(k_connect_flatten, pixels, block, 0, st, parent, area, HW, nb, chunks);
    launch(k_connect_count, pixels, block, 0, st, parent, area, sums, HW, nb, chunks, min_size);
    launch(k_connect_scan, tile_grid_dim((unsigned long long)N, 1), block, 0, st, sums, counts, N, nb, enforce ? 1u : 0u);
    launch(k_connect_apply, pixels, block, 0, st, parent, area, sums, HW, W, nb, chunks, min_size);
    if (enforce) launch(k_connect_chain, pixels, block, 0, st, parent, area, HW, nb, chunks);
    launch(k_connect_output, pixels, block, 0, st, parent, area, out, HW, nb, chunks);
}

}  // namespace fslic
