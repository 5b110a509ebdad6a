// compare.hip -- two label maps of one shape against each other, gfx950 (fast_slic_amd/compare.py).
//   k_overlap_tiles   : the overlap (contingency) table: every pair (a, b) = (labels[p], other[p]) with its number of pixels.  Per
//                       (frame, tile of 64 columns x 16 rows) one wavefront, as k_rag_tiles (rag.hip) without its halo and its LDS
//                       planes: the 16 rows of both maps are loaded to registers, row by row the wavefront merges the lanes' keys
//                       ((a << 16 | b) + 1) with one ballot per distinct key, whose popcount is the key's count.  The tile's
//                       distinct keys live one per lane; at the end of the tile every such lane issues ONE update of the frame's
//                       open-addressing table.  Keys past the 64th of a tile (noise maps) go to the table as they are met.
//                       The table and its compact pass: pairtable.h, pairtable.hip.
//   k_boundary_match  : boundary pixels of `other` that have a boundary pixel of `labels` within Chebyshev distance `tolerance`,
//                       and the boundary pixels of either map.  Per (frame, tile of 64 columns x 32 rows) one wavefront.  A row of
//                       boundary bits is one 64-bit ballot: the tile's columns and, for the halo of `tolerance` columns on either
//                       side, a second ballot; dilation along x is shifts and ORs of that (64 + 2 tolerance)-bit word in scalar
//                       registers.  Lane j keeps the dilated word of row y0 - tolerance + j (32 + 2 x 15 rows fit the 64 lanes),
//                       dilation along y is an OR over 2 tolerance + 1 lanes.  One block is four neighbouring tiles of one
//                       frame: its counts meet in LDS and go out as one 64-bit atomic per counter.
// All integer work: neither the order in which tiles arrive nor the capacity of the table can change a bit of the result.
#include "device_common.h"
#include "labels.h"
#include "compare.h"

namespace fslic {

constexpr int kOverlapRows = 16;                 // rows of an overlap tile
constexpr int kMatchRows = 32;                   // rows of a boundary match tile
static_assert(kMatchRows + 2 * kMatchMaxTolerance <= 64, "one lane per row of a tile and its halo");

template <class LA, class LB>
__global__ __launch_bounds__(256) void k_overlap_tiles(const LA* __restrict__ labels, const LB* __restrict__ other, PairHeader* __restrict__ hdr,
                                                       uint32_t* __restrict__ tkey, uint32_t* __restrict__ tcnt,
                                                       int N, int H, int W, uint32_t K, uint32_t M, uint32_t cap_mask) {
    const int lane = LANE();
    const uint32_t wave = rfl(threadIdx.x >> 6);
    const unsigned long long ntx = ((unsigned long long)W + 63ull) / 64ull, nty = (unsigned long long)((H + kOverlapRows - 1) / kOverlapRows);
    const unsigned long long per = ntx * nty, ntiles = per * (unsigned long long)N;
    const unsigned long long nwaves = (unsigned long long)gridDim.x * 4ull;
    const size_t HW = (size_t)H * (size_t)W;
    for (unsigned long long t = (unsigned long long)blockIdx.x * 4ull + wave; t < ntiles; t += nwaves) {
        if (pair_pass_lost(hdr)) return;
        const int n = (int)(t / per);
        const unsigned long long tt = t - (unsigned long long)n * per;
        const unsigned long long ty = tt / ntx, tx = tt - ty * ntx;
        const long long x = (long long)tx * 64 + lane;
        const int y0 = (int)ty * kOverlapRows;
        const bool okx = x < (long long)W;
        const int nrows = min(kOverlapRows, H - y0);
        const LA* __restrict__ la = labels + (size_t)n * HW;
        const LB* __restrict__ lb = other + (size_t)n * HW;
        const size_t cx = (size_t)min(x, (long long)W - 1);
        LA va[kOverlapRows];
        LB vb[kOverlapRows];
#pragma unroll
        for (int r = 0; r < kOverlapRows; ++r) {                           // rows past the image re-read the last one
            const size_t p = (size_t)min(y0 + r, H - 1) * (size_t)W + cx;
            va[r] = la[p];
            vb[r] = lb[p];
        }
        uint32_t key[kOverlapRows];                                        // 0: the pixel takes no part
#pragma unroll
        for (int r = 0; r < kOverlapRows; ++r) {
            const uint32_t a = canon(va[r], K), b = canon(vb[r], M);
            key[r] = (okx && r < nrows && a < K && b < M) ? ((a << 16) | b) + 1u : 0u;
        }
        // lane d: the tile's d-th distinct key and its pixels
        uint32_t ent = 0, ecnt = 0;
        int D = 0;
#pragma unroll
        for (int r = 0; r < kOverlapRows; ++r) {                           // (a run-time index would send key[] to scratch memory)
            if (r >= nrows) continue;
            const uint32_t k = key[r];
            bool pend = k != 0u;
            for (;;) {
                const unsigned long long any = ballot(pend);
                if (!any) break;
                const uint32_t cur = (uint32_t)__builtin_amdgcn_readlane((int)k, (int)__builtin_ctzll(any));
                const bool m = k == cur;
                const uint32_t cnt = (uint32_t)__popcll(ballot(m));
                pend = pend && !m;
                const unsigned long long hit = ballot(ent == cur);
                const int idx = hit ? (int)__builtin_ctzll(hit) : D;
                if (idx < 64) {
                    if (!hit) ++D;
                    if (lane == idx) {
                        ent = cur;
                        ecnt += cnt;
                    }
                } else if (lane == 0) {                                    // the lanes are taken: this row's share goes out at once
                    pair_table_add<false>(hdr, tkey, tcnt, nullptr, n, cap_mask, cur, cnt);
                }
            }
        }
        if (lane < D) pair_table_add<false>(hdr, tkey, tcnt, nullptr, n, cap_mask, ent, ecnt);
    }
}

// ---- boundary match ---------------------------------------------------------------------------
// Is (y, x) a boundary pixel of the map: its value differs from its right or its lower neighbour's, where the image has one.
// 0 <= y < H; any x (false outside [0, W)).  Values are compared as stored.
template <class T>
static __device__ __forceinline__ bool boundary_bit(const T* __restrict__ map, int y, long long x, int H, int W) {
    bool b = false;
    if (x >= 0 && x < (long long)W) {
        const size_t p = (size_t)y * (size_t)W + (size_t)x;
        const T c = map[p];
        if (x + 1 < (long long)W) b = map[p + 1] != c;
        if (y + 1 < H) b |= map[p + (size_t)W] != c;
    }
    return b;
}

// the value of lane + delta (a lane past the 63rd keeps its own)
static __device__ __forceinline__ unsigned long long lane_down(unsigned long long v, int delta) {
    const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, (unsigned)delta, 64);
    const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), (unsigned)delta, 64);
    return ((unsigned long long)hi << 32) | lo;
}

template <class LA, class LB>
__global__ __launch_bounds__(256) void k_boundary_match(const LA* __restrict__ labels, const LB* __restrict__ other,
                                                        unsigned long long* __restrict__ out, int N, int H, int W, int tol) {
    __shared__ uint32_t s_part[4][3];
    const int lane = LANE();
    const uint32_t wave = rfl(threadIdx.x >> 6);
    const unsigned long long ntx = ((unsigned long long)W + 63ull) / 64ull, nty = (unsigned long long)((H + kMatchRows - 1) / kMatchRows);
    const unsigned long long per = ntx * nty, gpf = (per + 3ull) / 4ull;    // a block's round: four neighbouring tiles of one frame
    const unsigned long long ngroups = gpf * (unsigned long long)N;
    const size_t HW = (size_t)H * (size_t)W;
    const int win = 2 * tol + 1;
    for (unsigned long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int n = (int)(g / gpf);
        const unsigned long long tt = (g - (unsigned long long)n * gpf) * 4ull + wave;
        uint32_t hits = 0, nother = 0, nlabels = 0;
        if (tt < per) {                                                    // (the same for every lane of the wavefront)
            const unsigned long long ty = tt / ntx, tx = tt - ty * ntx;
            const long long x0 = (long long)tx * 64, x = x0 + lane;
            const int y0 = (int)ty * kMatchRows;
            const int nr = min(kMatchRows, H - y0);
            const LA* __restrict__ la = labels + (size_t)n * HW;
            const LB* __restrict__ lb = other + (size_t)n * HW;
            const long long hx = lane < tol ? x0 - tol + lane : x0 + 64 + (lane - tol);      // lanes below 2 tol: the halo columns
            unsigned long long mine_l = 0, mine_o = 0;                     // lane j: row y0 - tol + j of labels (dilated along x), row y0 + j of other
            for (int j = 0; j < nr + 2 * tol; ++j) {
                const int y = y0 - tol + j;
                unsigned long long word = 0;
                if (y >= 0 && y < H) {
                    const unsigned long long mw = ballot(boundary_bit(la, y, x, H, W));
                    if (j >= tol && j < tol + nr) nlabels += (uint32_t)__popcll(mw);
                    word = mw;
                    if (tol > 0) {
                        const unsigned long long hw = ballot(lane < 2 * tol && boundary_bit(la, y, hx, H, W));
                        // bits 0 .. 63 + 2 tol: columns x0 - tol .. x0 + 63 + tol
                        unsigned long long lo = (hw & ((1ull << tol) - 1ull)) | (mw << tol);
                        unsigned long long hi = (mw >> (64 - tol)) | ((hw >> tol) << tol);
                        // bit i |= bits i + 1 .. i + 2 tol, by doubling: every shift is in [1, 30]
                        int cover = 1;
                        while (2 * cover <= win) {
                            lo |= (lo >> cover) | (hi << (64 - cover));
                            hi |= hi >> cover;
                            cover *= 2;
                        }
                        if (win > cover) {
                            const int s = win - cover;
                            lo |= (lo >> s) | (hi << (64 - s));
                        }
                        word = lo;
                    }
                }
                if (lane == j) mine_l = word;
                if (j < nr) {
                    const unsigned long long ow = ballot(boundary_bit(lb, y0 + j, x, H, W));
                    nother += (uint32_t)__popcll(ow);
                    if (lane == j) mine_o = ow;
                }
            }
            // lane j: the OR of lanes j .. j + 2 tol, rows y0 + j - tol .. y0 + j + tol
            int cover = 1;
            while (2 * cover <= win) {
                mine_l |= lane_down(mine_l, cover);
                cover *= 2;
            }
            if (win > cover) mine_l |= lane_down(mine_l, win - cover);
            hits = wave_reduce_add<uint32_t>(lane < nr ? (uint32_t)__popcll(mine_o & mine_l) : 0u);      // at most 64 x 32 a tile
        }
        if (lane == 0) {
            s_part[wave][0] = hits;
            s_part[wave][1] = nother;
            s_part[wave][2] = nlabels;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            const uint32_t sum = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
            if (sum) atomicAdd(&out[(size_t)n * 3 + threadIdx.x], (unsigned long long)sum);
        }
        __syncthreads();
    }
}

// ---- launches ---------------------------------------------------------------------------------
static inline unsigned long long compare_tiles(int N, int H, int W, int rows) {
    return (unsigned long long)N * (((unsigned long long)W + 63ull) / 64ull) * (unsigned long long)((H + rows - 1) / rows);
}

// (the two maps as their label types: with_label_type of labels.h, nested)
void launch_overlap_accumulate(const void* labels, int label_type, const void* other, int other_type, void* workspace,
                               int N, int H, int W, int K, int M, uint32_t capacity, hipStream_t st) {
    const PairTables t = pair_tables(workspace, N, capacity);
    const dim3 grid(tile_grid(compare_tiles(N, H, W, kOverlapRows), 4)), block(256);
    with_label_type(labels, label_type, [&](auto* la) {
        with_label_type(other, other_type, [&](auto* lb) {
            launch(k_overlap_tiles<std::decay_t<decltype(*la)>, std::decay_t<decltype(*lb)>>, grid, block, 0, st, la, lb, t.hdr, t.key, t.cnt,
                   N, H, W, (uint32_t)K, (uint32_t)M, capacity - 1u);
        });
    });
}

void launch_boundary_match(const void* labels, int label_type, const void* other, int other_type, unsigned long long* out,
                           int N, int H, int W, int tolerance, hipStream_t st) {
    const dim3 grid(tile_grid(compare_tiles(N, H, W, kMatchRows) + 3ull * (unsigned long long)N, 4)), block(256);
    with_label_type(labels, label_type, [&](auto* la) {
        with_label_type(other, other_type, [&](auto* lb) {
            launch(k_boundary_match<std::decay_t<decltype(*la)>, std::decay_t<decltype(*lb)>>, grid, block, 0, st, la, lb, out, N, H, W, tolerance);
        });
    });
}

}  // namespace fslic
