// rag.hip -- the region adjacency graph of a label map, gfx950 (fast_slic_amd/rag.py): every unordered pair of labels that touch,
// with the number of neighbouring pixel pairs across their boundary and, per image channel, the sum of |difference| over those pairs.
//   k_rag_tiles   : per (frame, tile of 64 columns x 16 rows) one wavefront.  The tile and a one-pixel halo (right, below, left for the
//                   down-left neighbour) go to LDS once; pixel p owns the pairs {p, right}, {p, down} and, 8-connectivity, {p, down-right},
//                   {p, down-left}, so a pair that straddles a tile seam belongs to the tile of p alone.  Row by row the wavefront merges
//                   the lanes' pair keys (lo << 16 | hi): one ballot per distinct key for the count, one DPP reduction per two channels for
//                   the contrast.  The tile's distinct keys live one per lane (lane d: key d, its count, its C sums); at the end of the
//                   tile every such lane issues ONE update of the frame's open-addressing table.  Keys past the 64th of a tile (noise
//                   maps) are sent to the table as they are met, one update per (row, key).
// The table and its compact pass: pairtable.h, pairtable.hip.
// All integer work: counts are 32-bit integer adds, contrast sums 64-bit integer adds, so neither the order in which tiles arrive nor
// the capacity of the table can change a bit of the result.  Labels are checked against K before they form a key.
#include "device_common.h"
#include "labels.h"
#include "rag.h"

namespace fslic {

constexpr int kRagRows = 16;                 // rows of a tile
constexpr int kRagPitch = 66;                // 64 columns and one halo column on either side

// the C bytes of one pixel in one word (channel c in bits 8c .. 8c + 7)
static __device__ __forceinline__ uint32_t load_pixel(const uint8_t* __restrict__ p, int C, bool word) {
    if (word) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = p[0];
    if (C > 1) v |= (uint32_t)p[1] << 8;
    if (C > 2) v |= (uint32_t)p[2] << 16;
    if (C > 3) v |= (uint32_t)p[3] << 24;
    return v;
}
// |a - b| of the bytes at bit `lo` into the low half, of the bytes at bit `lo + 8` into the high half
static __device__ __forceinline__ uint32_t absdiff2(uint32_t a, uint32_t b, int lo) {
    const int d0 = (int)((a >> lo) & 255u) - (int)((b >> lo) & 255u);
    const int d1 = (int)((a >> (lo + 8)) & 255u) - (int)((b >> (lo + 8)) & 255u);
    return (uint32_t)abs(d0) | ((uint32_t)abs(d1) << 16);
}

template <class L, bool kImg, bool k8>
__global__ __launch_bounds__(256) void k_rag_tiles(const L* __restrict__ labels, const uint8_t* __restrict__ image, PairHeader* __restrict__ hdr,
                                                   uint32_t* __restrict__ tkey, uint32_t* __restrict__ tcnt, unsigned long long* __restrict__ tsum,
                                                   int N, int C, int H, int W, uint32_t K, uint32_t cap_mask, bool word) {
    __shared__ uint32_t s_lab[4][kRagRows + 1][kRagPitch];                 // K: no label (outside [0, K), past the image)
    __shared__ uint32_t s_pix[kImg ? 4 : 1][kImg ? kRagRows + 1 : 1][kRagPitch];
    constexpr int kDirs = k8 ? 4 : 2;
    const int lane = LANE();
    const uint32_t wave = rfl(threadIdx.x >> 6);
    uint32_t (*sl)[kRagPitch] = s_lab[wave];
    uint32_t (*sp)[kRagPitch] = s_pix[kImg ? wave : 0];
    const unsigned long long ntx = (unsigned long long)((W + 63) / 64), nty = (unsigned long long)((H + kRagRows - 1) / kRagRows);
    const unsigned long long per = ntx * nty, ntiles = per * (unsigned long long)N;
    const unsigned long long nwaves = (unsigned long long)gridDim.x * 4ull;
    const size_t HW = (size_t)H * (size_t)W;
    for (unsigned long long t = (unsigned long long)blockIdx.x * 4ull + wave; t < ntiles; t += nwaves) {
        if (pair_pass_lost(hdr)) return;
        const int n = (int)(t / per);
        const unsigned long long tt = t - (unsigned long long)n * per;
        const int ty = (int)(tt / ntx), tx = (int)(tt - (unsigned long long)ty * ntx);
        const int x = tx * 64 + lane, y0 = ty * kRagRows;
        const bool okx = x < W;
        const int nrows = min(kRagRows, H - y0);
        const L* __restrict__ lb = labels + (size_t)n * HW;
        const uint8_t* __restrict__ ib = kImg ? image + (size_t)n * HW * (size_t)C : nullptr;
        wave_lds_sync();                                                   // every lane has read the previous tile
        {
            const size_t cx = (size_t)min(x, W - 1);
            uint32_t lv[kRagRows + 1], pv[kRagRows + 1];
#pragma unroll
            for (int r = 0; r <= kRagRows; ++r) {                          // rows past the image re-read the last one
                const size_t p = (size_t)min(y0 + r, H - 1) * W + cx;
                lv[r] = canon(lb[p], K);
                if (kImg) pv[r] = load_pixel(ib + p * (size_t)C, C, word);
            }
#pragma unroll
            for (int r = 0; r <= kRagRows; ++r) {
                sl[r][lane + 1] = (okx && y0 + r < H) ? lv[r] : K;
                if (kImg) sp[r][lane + 1] = pv[r];
            }
        }
        if (lane == 0 || lane == 63) {                                     // the halo columns: x0 - 1 (down-left pairs) and x0 + 64
            const int hx = lane == 0 ? x - 1 : x + 1;
            const bool okh = hx >= 0 && hx < W;
            const size_t cx = (size_t)min(max(hx, 0), W - 1);
            const int col = lane == 0 ? 0 : kRagPitch - 1;
            uint32_t lv[kRagRows + 1], pv[kRagRows + 1];
#pragma unroll
            for (int r = 0; r <= kRagRows; ++r) {
                const size_t p = (size_t)min(y0 + r, H - 1) * W + cx;
                lv[r] = canon(lb[p], K);
                if (kImg) pv[r] = load_pixel(ib + p * (size_t)C, C, word);
            }
#pragma unroll
            for (int r = 0; r <= kRagRows; ++r) {
                sl[r][col] = (okh && y0 + r < H) ? lv[r] : K;
                if (kImg) sp[r][col] = pv[r];
            }
        }
        wave_lds_sync();
        // lane d: the tile's d-th distinct key, its pixel pairs and its channel sums
        uint32_t ent = 0, ecnt = 0, esum[kPairMaxChannels] = {0, 0, 0, 0};
        int D = 0;
        for (int r = 0; r < nrows; ++r) {
            const uint32_t a = sl[r][lane + 1];
            uint32_t nb[4], key[4];                                        // the first kDirs in use
            nb[0] = sl[r][lane + 2];                                       // right
            nb[1] = sl[r + 1][lane + 1];                                   // down
            if (k8) {
                nb[2] = sl[r + 1][lane + 2];                               // down-right
                nb[3] = sl[r + 1][lane];                                   // down-left
            }
            uint32_t pend = 0;
#pragma unroll
            for (int s = 0; s < kDirs; ++s) {
                const bool on = a < K && nb[s] < K && a != nb[s];
                key[s] = on ? (min(a, nb[s]) << 16) | max(a, nb[s]) : 0u;
                pend |= (on ? 1u : 0u) << s;
            }
            if (ballot(pend != 0u) == 0ull) continue;
            uint32_t d01[4], d23[4];
            if (kImg) {
                const uint32_t pa = sp[r][lane + 1];
                uint32_t pn[4];
                pn[0] = sp[r][lane + 2];
                pn[1] = sp[r + 1][lane + 1];
                if (k8) {
                    pn[2] = sp[r + 1][lane + 2];
                    pn[3] = sp[r + 1][lane];
                }
#pragma unroll
                for (int s = 0; s < kDirs; ++s) {
                    d01[s] = absdiff2(pa, pn[s], 0);
                    d23[s] = absdiff2(pa, pn[s], 16);
                }
            }
            for (;;) {
                const unsigned long long any = ballot(pend != 0u);
                if (!any) break;
                uint32_t first = key[kDirs - 1];
#pragma unroll
                for (int s = kDirs - 2; s >= 0; --s) first = ((pend >> s) & 1u) ? key[s] : first;
                const uint32_t cur = (uint32_t)__builtin_amdgcn_readlane((int)first, (int)__builtin_ctzll(any));
                uint32_t cnt = 0, v01 = 0, v23 = 0;                        // per lane at most 4 x 255 a half: 64 lanes stay below 2^16
#pragma unroll
                for (int s = 0; s < kDirs; ++s) {
                    const bool m = key[s] == cur;
                    cnt += (uint32_t)__popcll(ballot(m));
                    if (kImg) {
                        v01 += m ? d01[s] : 0u;
                        v23 += m ? d23[s] : 0u;
                    }
                    pend &= ~((m ? 1u : 0u) << s);
                }
                uint32_t add[kPairMaxChannels] = {0, 0, 0, 0};
                if (kImg) {
                    const uint32_t r01 = wave_reduce_add<uint32_t>(v01);
                    add[0] = r01 & 0xFFFFu;
                    add[1] = r01 >> 16;
                    if (C > 2) {
                        const uint32_t r23 = wave_reduce_add<uint32_t>(v23);
                        add[2] = r23 & 0xFFFFu;
                        add[3] = r23 >> 16;
                    }
                }
                const unsigned long long hit = ballot(ent == cur);
                const int idx = hit ? (int)__builtin_ctzll(hit) : D;
                if (idx < 64) {
                    if (!hit) ++D;
                    if (lane == idx) {
                        ent = cur;
                        ecnt += cnt;
#pragma unroll
                        for (int c = 0; c < kPairMaxChannels; ++c) esum[c] += add[c];
                    }
                } else if (lane == 0) {                                    // the lanes are taken: this row's share goes out at once
                    pair_table_add<true>(hdr, tkey, tcnt, tsum, n, cap_mask, cur, cnt, C, add);
                }
            }
        }
        if (lane < D) pair_table_add<true>(hdr, tkey, tcnt, tsum, n, cap_mask, ent, ecnt, C, esum);
    }
}

// ---- launches ---------------------------------------------------------------------------------
template <class L>
static void rag_tiles_as(const L* lab, const uint8_t* image, void* ws, int N, int C, int H, int W, int K, int connectivity,
                         uint32_t capacity, hipStream_t st) {
    const unsigned long long tiles = (unsigned long long)N * (unsigned long long)((W + 63) / 64) * (unsigned long long)((H + kRagRows - 1) / kRagRows);
    const PairTables t = pair_tables(ws, N, capacity);
    const dim3 grid(tile_grid(tiles, 4)), block(256);
    const bool word = C == 4 && (reinterpret_cast<uintptr_t>(image) & 3u) == 0u;      // a pixel is one aligned 32-bit word
    const uint32_t mask = capacity - 1u;
#define FSLIC_RAG_LAUNCH(IMG, EIGHT) \
    launch(k_rag_tiles<L, IMG, EIGHT>, grid, block, 0, st, lab, image, t.hdr, t.key, t.cnt, t.sum, N, C, H, W, (uint32_t)K, mask, word)
    if (image) {
        if (connectivity == 8) FSLIC_RAG_LAUNCH(true, true);
        else FSLIC_RAG_LAUNCH(true, false);
    } else {
        if (connectivity == 8) FSLIC_RAG_LAUNCH(false, true);
        else FSLIC_RAG_LAUNCH(false, false);
    }
#undef FSLIC_RAG_LAUNCH
}
void launch_rag_accumulate(const void* labels, int label_type, const uint8_t* image, void* workspace,
                           int N, int C, int H, int W, int K, int connectivity, uint32_t capacity, hipStream_t st) {
    with_label_type(labels, label_type, [&](auto* lab) { rag_tiles_as(lab, image, workspace, N, C, H, W, K, connectivity, capacity, st); });
}

}  // namespace fslic
