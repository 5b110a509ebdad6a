// pool.hip -- superpixel pooling of float feature planes over a label map and its inverse broadcast, gfx950 (fast_slic_amd/pool.py).
//   k_pool_tiles     : per (frame, tile of 64 columns x 16 rows, chunk of channels) one wavefront: the tile's distinct labels once,
//                      then every channel plane of the chunk; one f32 partial (sum) or one 64-bit key (max) per (tile, label, channel), added into the
//                      workspace with integer atomics, and the pixel count per (tile, label)
//   k_pool_finalize  : workspace -> values [N][C][K] (sum, mean or max), counts [N][K], argmax [N][C][K]
//   k_unpool         : out[n][c][p] = values[n][c][labels[n][p]] (fill where the label is not in [0, K)); with an argmax table the
//                      value only reaches the pixel the table names (the max backward)
// Determinism: a partial is a fixed-order sum (rows of a column in order, then the wavefront's DPP tree) of the tile's pixels of one
// label; partials are combined EXACTLY in a fixed-point accumulator of kPoolLimbs int64 words (one 32-bit limb each, bit 0 of limb 0
// weighs 2^kPoolLsb), so the order in which tiles arrive cannot change a bit; k_pool_finalize rounds once to f32.  Max keys are
// combined with a 64-bit integer atomicMax.  No float atomics anywhere.  Labels are checked against K before any use as an index.
#include "device_common.h"
#include "pool.h"
#include "fixsum.h"      // fix_add, fix_to_float: the accumulator, shared with region.hip
#include <algorithm>

namespace fslic {

constexpr int kPoolRows = 16;          // rows of a tile (one label per lane and row held in registers)
constexpr int kPoolMaxList = 64 * kPoolRows;

// float -> uint32 whose unsigned order is the float order (-0.0 below +0.0), and back
static __device__ __forceinline__ uint32_t ordered_bits(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static __device__ __forceinline__ float from_ordered(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

static __device__ __forceinline__ unsigned long long wave_reduce_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// One wavefront per (frame, tile, channel chunk).  Label analysis once per item: the distinct labels in order of first appearance (column-major
// scan of the lanes' first pending rows), each with the rows that hold it, in LDS; the pixel count per label goes out at once.
// Then, per channel plane: 16 rows of 256 B, and per distinct label one partial -- every lane sums its column's pixels of that
// label in row order (starting from -0.0 and adding -0.0 for the others, so that the value is exactly the sum of the label's
// pixels), the DPP tree adds the 64 lanes in a fixed order.  Lane d keeps the partial of label d; one flush per 64 labels.
template <class L, bool kMax>
__global__ __launch_bounds__(256) void k_pool_tiles(const float* __restrict__ feat, const L* __restrict__ labels,
                                                    unsigned long long* __restrict__ acc, uint32_t* __restrict__ counts,
                                                    int N, int C, int H, int W, uint32_t K, int nchunk, int cchunk) {
    __shared__ uint32_t s_list[4][kPoolMaxList];           // per wavefront: label << 16 | rows holding it
    const int lane = LANE();
    const uint32_t wave = rfl(threadIdx.x >> 6);
    uint32_t* lst = s_list[wave];
    const unsigned long long ntx = (unsigned long long)((W + 63) / 64), nty = (unsigned long long)((H + kPoolRows - 1) / kPoolRows);
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
        const int x = tx * 64 + lane, y0 = ty * kPoolRows;
        const bool okx = x < W;
        const int nrows = min(kPoolRows, H - y0);
        const size_t p0 = (size_t)y0 * W + (size_t)min(x, W - 1);     // this lane's pixel of row 0 (flat index in the frame)
        const L* __restrict__ lb = labels + (size_t)n * HW + p0;
        uint32_t lab[kPoolRows];                                      // K: no label (outside [0, K), past the image)
#pragma unroll
        for (int r = 0; r < kPoolRows; ++r) {                         // rows past the image re-read the last one
            const uint32_t v = canon(lb[(size_t)min(r, nrows - 1) * W], K);
            lab[r] = (okx && r < nrows) ? v : K;
        }
        uint32_t pend = 0;                                            // bit r: row r not yet listed
#pragma unroll
        for (int r = 0; r < kPoolRows; ++r) pend |= (lab[r] < K ? 1u : 0u) << r;
        wave_lds_sync();                                              // every lane has read the previous tile's list
        int D = 0;
        for (;;) {
            const unsigned long long any = ballot(pend != 0u);
            if (!any) break;
            uint32_t first = K;
#pragma unroll
            for (int r = kPoolRows - 1; r >= 0; --r) first = ((pend >> r) & 1u) ? lab[r] : first;
            const uint32_t cur = (uint32_t)__builtin_amdgcn_readlane((int)first, (int)__builtin_ctzll(any));
            uint32_t mine = 0, rows = 0;
#pragma unroll
            for (int r = 0; r < kPoolRows; ++r) {
                const bool m = lab[r] == cur;
                mine |= (m ? 1u : 0u) << r;
                rows |= (ballot(m) != 0ull ? 1u : 0u) << r;
            }
            pend &= ~mine;
            const uint32_t cnt = wave_reduce_add<uint32_t>((uint32_t)__popc(mine));
            if (lane == 0) {
                lst[D] = (cur << 16) | rows;
                if (chunk == 0) atomicAdd(&counts[(size_t)n * K + cur], cnt);
            }
            ++D;
        }
        wave_lds_sync();
        if (D == 0) continue;
        const float* __restrict__ fb = feat + ((size_t)n * (size_t)C + (size_t)c0) * HW + p0;
        for (int c = c0; c < c1; ++c, fb += HW) {
            float xv[kPoolRows];
#pragma unroll
            for (int r = 0; r < kPoolRows; ++r) xv[r] = __builtin_nontemporal_load(fb + (size_t)min(r, nrows - 1) * W);
            unsigned long long* __restrict__ a = acc + ((size_t)n * C + c) * (size_t)(kMax ? 1 : kPoolLimbs) * K;
            for (int d0 = 0; d0 < D; d0 += 64) {
                const int dn = min(64, D - d0);
                const uint32_t ent = lst[d0 + min(lane, dn - 1)];
                float part = -0.0f;
                unsigned long long best = 0ull;
                for (int dd = 0; dd < dn; ++dd) {
                    const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)ent, dd);
                    const uint32_t cur = e >> 16, rows = e & 0xFFFFu;
                    if (kMax) {
                        unsigned long long bk = 0ull;                 // (value, lowest flat index) of this lane's pixels of `cur`
#pragma unroll
                        for (int r = 0; r < kPoolRows; ++r) {
                            if ((rows >> r) & 1u) {
                                const unsigned long long key = ((unsigned long long)ordered_bits(xv[r]) << 32) |
                                                               (unsigned long long)(0xFFFFFFFFu - (uint32_t)(p0 + (size_t)r * W));
                                bk = (lab[r] == cur && key > bk) ? key : bk;
                            }
                        }
                        bk = wave_reduce_max_u64(bk);
                        best = lane == dd ? bk : best;
                    } else {
                        float v = -0.0f;
#pragma unroll
                        for (int r = 0; r < kPoolRows; ++r)
                            if ((rows >> r) & 1u) v += lab[r] == cur ? xv[r] : -0.0f;
                        const float s = wave_reduce_add<float>(v);
                        part = lane == dd ? s : part;
                    }
                }
                if (lane < dn) {
                    const uint32_t k = ent >> 16;                     // < K: listed labels passed canon()
                    if (kMax) atomicMax(a + k, best);                 // best != 0: the label has a pixel in this tile
                    else fix_add(a + k, (size_t)K, part);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_pool_finalize(const unsigned long long* __restrict__ acc, const uint32_t* __restrict__ counts,
                                                       int reduce, float* __restrict__ values, int32_t* __restrict__ cnt_out,
                                                       int32_t* __restrict__ argmax, int C, uint32_t K, unsigned long long total) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    const unsigned long long CK = (unsigned long long)C * K;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < total; i += stride) {
        const unsigned long long n = i / CK, ck = i - n * CK, c = ck / K, k = ck - c * K;
        const uint32_t cnt = counts[n * K + k];
        if (cnt_out && c == 0) cnt_out[n * K + k] = (int32_t)cnt;
        if (reduce == kPoolMax) {
            const unsigned long long key = acc[i];
            values[i] = key ? from_ordered((uint32_t)(key >> 32)) : 0.0f;
            if (argmax) argmax[i] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
        } else {
            float f = fix_to_float(acc + (n * C + c) * (unsigned long long)kPoolLimbs * K + k, (size_t)K);
            if (reduce == kPoolMean) f = cnt ? f / (float)cnt : 0.0f;
            values[i] = f;
        }
    }
}

// One thread per 4 consecutive pixels of a frame; the labels are read once, then every channel: 4 gathers from the frame's [C][K]
// table (label-coherent: served by the caches) and one 16-byte store (kVec: H * W % 4 == 0 and an aligned output).
typedef float pool_f4 __attribute__((ext_vector_type(4)));
template <class L, bool kArg, bool kVec>
__global__ __launch_bounds__(256) void k_unpool(const float* __restrict__ values, const L* __restrict__ labels,
                                                const int32_t* __restrict__ argmax, float fill, float* __restrict__ out,
                                                int C, unsigned long long HW, uint32_t K, unsigned long long blocks_per_frame) {
    const unsigned long long n = blockIdx.x / blocks_per_frame, pb = blockIdx.x - n * blocks_per_frame;
    const unsigned long long p = (pb * 256ull + threadIdx.x) * 4ull;
    if (p >= HW) return;
    const L* __restrict__ lb = labels + n * HW;
    uint32_t lab[4], idx[4];
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lab[j] = p + j < HW ? canon(lb[p + j], K) : K;
        ok[j] = lab[j] < K;
        idx[j] = ok[j] ? lab[j] : 0u;                               // every gather reads a checked index
    }
    const float* __restrict__ vt = values + n * (unsigned long long)C * K;
    const int32_t* __restrict__ at = kArg ? argmax + n * (unsigned long long)C * K : nullptr;
    float* __restrict__ ob = out + n * (unsigned long long)C * HW + p;
    for (int c = 0; c < C; ++c, vt += K, ob += HW) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool take = ok[j];
            if (kArg) take = take && at[idx[j]] == (int32_t)(p + j);
            o[j] = take ? vt[idx[j]] : fill;
        }
        if (kArg) at += K;
        if (kVec) {
            const pool_f4 v = {o[0], o[1], o[2], o[3]};
            __builtin_nontemporal_store(v, reinterpret_cast<pool_f4*>(ob));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (p + j < HW) __builtin_nontemporal_store(o[j], ob + j);
        }
    }
}

// ---- launches ---------------------------------------------------------------------------------
// Work item = (tile, chunk of channels).  A wavefront walks its item's channels one after the other, so with few tiles (8 x 1280x720:
// 7 200) whole-C items leave the chip with one long round of waves and a tail; the channels are cut into chunks until there are about
// kPoolItems items (each chunk re-reads and re-analyses its tile's labels: 2 B/px per chunk, L2-served between neighbouring items).
// Measured on 8 x 1280x720, K=1600: C=21 269 -> 248 us, C=64 703 -> 560 us; one channel per chunk (C=3) lost (75 -> 94 us).
constexpr unsigned long long kPoolItems = 256ull * 28ull * 4ull;
constexpr int kPoolMinChunk = 4;
template <class L>
static void pool_tiles_as(const float* feat, const L* lab, int reduce, void* ws, int N, int C, int H, int W, int K, hipStream_t st) {
    const unsigned long long tiles = (unsigned long long)N * (unsigned long long)((W + 63) / 64) * (unsigned long long)((H + kPoolRows - 1) / kPoolRows);
    const unsigned long long most = (unsigned long long)(C + kPoolMinChunk - 1) / kPoolMinChunk;     // chunks of at least kPoolMinChunk channels
    const int want = (int)std::min<unsigned long long>(most, std::max<unsigned long long>(1ull, (kPoolItems + tiles - 1) / tiles));
    const int cchunk = (C + want - 1) / want, nchunk = (C + cchunk - 1) / cchunk;
    const unsigned long long items = tiles * (unsigned long long)nchunk;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(ws);
    uint32_t* counts = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + pool_acc_bytes(N, C, K, reduce));
    if (reduce == kPoolMax)
        launch(k_pool_tiles<L, true>, dim3(tile_grid(items, 4)), dim3(256), 0, st, feat, lab, acc, counts, N, C, H, W, (uint32_t)K, nchunk, cchunk);
    else
        launch(k_pool_tiles<L, false>, dim3(tile_grid(items, 4)), dim3(256), 0, st, feat, lab, acc, counts, N, C, H, W, (uint32_t)K, nchunk, cchunk);
}
void launch_pool_tiles(const float* feat, const void* labels, int label_type, int reduce, void* workspace,
                       int N, int C, int H, int W, int K, hipStream_t st) {
    with_label_type(labels, label_type, [&](auto* lab) { pool_tiles_as(feat, lab, reduce, workspace, N, C, H, W, K, st); });
}

void launch_pool_finalize(const void* workspace, int reduce, float* values, int32_t* counts, int32_t* argmax,
                          int N, int C, int K, hipStream_t st) {
    const unsigned long long total = (unsigned long long)N * (unsigned long long)C * (unsigned long long)K;
    const unsigned long long* acc = reinterpret_cast<const unsigned long long*>(workspace);
    const uint32_t* cnt = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(workspace) + pool_acc_bytes(N, C, K, reduce));
    launch(k_pool_finalize, dim3(tile_grid(total, 256)), dim3(256), 0, st, acc, cnt, reduce, values, counts, argmax, C, (uint32_t)K, total);
}

template <bool kArg, class L>
static void unpool_as(const float* values, const L* lab, const int32_t* argmax, float fill, float* out,
                      int N, int C, int H, int W, int K, hipStream_t st) {
    const unsigned long long HW = (unsigned long long)H * (unsigned long long)W, bpf = (HW + 1023ull) / 1024ull;
    const dim3 grid((unsigned)(bpf * (unsigned long long)N));
    if (HW % 4ull == 0ull && (reinterpret_cast<uintptr_t>(out) & 15u) == 0u)
        launch(k_unpool<L, kArg, true>, grid, dim3(256), 0, st, values, lab, argmax, fill, out, C, HW, (uint32_t)K, bpf);
    else
        launch(k_unpool<L, kArg, false>, grid, dim3(256), 0, st, values, lab, argmax, fill, out, C, HW, (uint32_t)K, bpf);
}
void launch_unpool(const float* values, const void* labels, int label_type, const int32_t* argmax, float fill, float* out,
                   int N, int C, int H, int W, int K, hipStream_t st) {
    with_label_type(labels, label_type, [&](auto* lab) {
        if (argmax) unpool_as<true>(values, lab, argmax, fill, out, N, C, H, W, K, st);
        else unpool_as<false>(values, lab, argmax, fill, out, N, C, H, W, K, st);
    });
}

}  // namespace fslic
