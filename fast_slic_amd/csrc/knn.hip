// knn.hip -- exact k nearest neighbours in feature space, gfx950 (fast_slic_amd/knn.py states the rule; the key, the launch shape and
// its forms are knn.h's).
//   k_knn<T, ROWS, DR> : a block of T threads takes items = (frame, group of ROWS consecutive query rows), grid-stride.  Thread t is row
//                        t % ROWS and slice t / ROWS.  DR > 0: the query's D <= DR channels in registers; the block stages tiles of
//                        candidates in LDS channel-major (an invalid candidate with NaN in channel 0: its distance is NaN and drops out
//                        with the others), and a thread folds the candidates of its slice, W neighbouring ones a step from one wide
//                        LDS read a channel.  DR == 0: both ends from global memory.  Then the merge of the slices' lists and the
//                        coalesced store.
// This file is compiled with -ffp-contract=off: the difference, the product and the sum of a channel are three IEEE float operations,
// each rounded on its own, in ascending channel order for every pair, whatever the tile.  No atomics, no workspace, no block waits for
// another; every store is a vector store and every output element is written exactly once.
#include "knn.h"
#include "launch.h"

namespace fslic {

namespace {

constexpr unsigned long long kKnnEmpty = ~0ull;

// `key` (below `worst`) into the ascending list of k keys at list[0], list[stride], ...; the last one falls out
__device__ __forceinline__ void knn_insert(unsigned long long* list, int stride, int k, unsigned long long key, unsigned long long& worst) {
    int p = k - 1;
    while (p > 0) {
        const unsigned long long prev = list[(p - 1) * stride];
        if (prev < key) break;
        list[p * stride] = prev;
        --p;
    }
    list[p * stride] = key;
    worst = list[(k - 1) * stride];
}

__device__ __forceinline__ void knn_offer(unsigned long long* list, int stride, int k, float d, uint32_t j, unsigned long long& worst) {
    if (d != d) return;                                                                // a NaN distance is no candidate
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)j;
    if (key < worst) knn_insert(list, stride, k, key, worst);
}

template <int T, int ROWS, int DR>
__global__ __launch_bounds__(T) void k_knn(const float* __restrict__ x, const float* __restrict__ y, const uint8_t* __restrict__ valid,
                                           int32_t* __restrict__ indices, float* __restrict__ dist, int D, uint32_t K, int k, int skip_self,
                                           uint32_t groups, unsigned long long items) {
    constexpr int S = T / ROWS;
    constexpr uint32_t W = DR > 8 ? 2u : 4u;                                           // candidates of a step in the register forms
    struct alignas(4 * W) Wide { float v[W]; };
    static_assert(S >= 2 && (S & (S - 1)) == 0 && 16 % S == 0 && ROWS % 16 == 0, "slices of a block");      // 4 S divides a tile
    extern __shared__ unsigned long long s_key[];                                      // [k][T] keys, then the tile, float [D][tile] (knn_lds_bytes)
    float* const s_y = reinterpret_cast<float*>(s_key + k * T);
    const uint32_t tid = threadIdx.x, r = tid % ROWS, s = tid / ROWS;
    const uint32_t tile = DR > 0 ? ((uint32_t)kKnnTileFloats / (uint32_t)D) & ~63u : 0u;      // candidates of a tile: >= 64, a multiple of 4 S
    unsigned long long* const list = s_key + tid;
    for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x) {      // (the same trips for every thread of a block)
        const uint32_t f = (uint32_t)(item / groups), i0 = (uint32_t)(item - (unsigned long long)f * groups) * (uint32_t)ROWS;      // i0 < K
        const uint32_t i = i0 + r;
        const size_t frame = (size_t)f * (size_t)D * K, node0 = (size_t)f * K;         // of channel 0, node 0; of node 0
        const bool active = i < K && (!valid || valid[node0 + i] != 0);
        __syncthreads();                                                               // the stores of the item before have read the lists
        for (int o = 0; o < k; ++o) list[o * T] = kKnnEmpty;
        unsigned long long worst = kKnnEmpty;
        if (DR > 0) {
            float q[DR > 0 ? DR : 1];
#pragma unroll
            for (int c = 0; c < DR; ++c) q[c] = active && c < D ? x[frame + (size_t)c * K + i] : 0.0f;
            for (uint32_t j0 = 0; j0 < K; j0 += tile) {
                const uint32_t cnt = K - j0 < tile ? K - j0 : tile;
                __syncthreads();                                                       // the folds of the tile before are over
                for (uint32_t c = tid >> 6; c < (uint32_t)D; c += T / 64)
                    for (uint32_t t = tid & 63u; t < cnt; t += 64u) {
                        const bool drop = c == 0u && valid && valid[node0 + j0 + t] == 0;
                        s_y[c * tile + t] = drop ? __builtin_nanf("") : y[frame + (size_t)c * K + j0 + t];
                    }
                __syncthreads();
                if (!active) continue;                                                 // (every thread meets the barriers above)
                // W neighbouring candidates a step: one wide LDS read a channel serves W folds (beyond cnt it reads what the tile held
                // before, inside the tile, and offers nothing).  W = 4 in the narrow form, 2 in the wide one, whose 64 channels leave
                // fewer registers
                for (uint32_t t = W * s; t < cnt; t += W * S) {
                    float acc[W];
#pragma unroll
                    for (uint32_t u = 0; u < W; ++u) acc[u] = 0.0f;
#pragma unroll
                    for (int c = 0; c < DR; ++c) {
                        if (c < D) {                                                   // (no early exit: the loop unrolls and q stays in registers)
                            const Wide yv = *reinterpret_cast<const Wide*>(s_y + c * tile + t);
#pragma unroll
                            for (uint32_t u = 0; u < W; ++u) {
                                const float d = q[c] - yv.v[u];
                                acc[u] = acc[u] + d * d;
                            }
                        }
                    }
#pragma unroll
                    for (uint32_t u = 0; u < W; ++u) {
                        const uint32_t j = j0 + t + u;
                        if (t + u < cnt && !(skip_self && j == i)) knn_offer(list, T, k, acc[u], j, worst);
                    }
                }
            }
        } else if (active) {
            const float* __restrict__ xp = x + frame + i;
            for (uint32_t j = s; j < K; j += S) {
                if ((skip_self && j == i) || (valid && valid[node0 + j] == 0)) continue;
                const float* __restrict__ yp = y + frame + j;
                float acc = 0.0f;
                for (int c = 0; c < D; ++c) {
                    const float d = xp[(size_t)c * K] - yp[(size_t)c * K];
                    acc = acc + d * d;
                }
                knn_offer(list, T, k, acc, j, worst);
            }
        }
        // the slices of a row, by key: slice s takes in what slice s + h kept, ascending, until one is no better than its own worst
        for (int h = S / 2; h >= 1; h >>= 1) {
            __syncthreads();
            if (s < (uint32_t)h) {
                const unsigned long long* theirs = s_key + tid + h * ROWS;
                for (int o = 0; o < k; ++o) {
                    const unsigned long long key = theirs[o * T];
                    if (key >= worst) break;
                    knn_insert(list, T, k, key, worst);
                }
            }
        }
        __syncthreads();
        const uint32_t rows = K - i0 < (uint32_t)ROWS ? K - i0 : (uint32_t)ROWS;
        const size_t out0 = (node0 + i0) * (size_t)k;                                  // of the group's first row
        for (uint32_t e = tid; e < rows * (uint32_t)k; e += T) {
            const uint32_t row = e / (uint32_t)k, o = e - row * (uint32_t)k;
            const unsigned long long key = s_key[o * T + row];                         // slice 0 of the row
            indices[out0 + e] = key == kKnnEmpty ? -1 : (int32_t)(uint32_t)key;
            dist[out0 + e] = key == kKnnEmpty ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
        }
    }
}

template <int T, int ROWS>
void launch_form(const float* x, const float* y, const uint8_t* valid, int32_t* indices, float* dist, int N, int D, int K, int k, bool skip_self,
                 hipStream_t st) {
    const uint32_t groups = ((uint32_t)K + ROWS - 1u) / ROWS;
    const unsigned long long items = (unsigned long long)N * groups;
    const dim3 grid((unsigned)tile_grid(items, 1)), block(T);
#define FSLIC_KNN(DR) launch(k_knn<T, ROWS, DR>, grid, block, knn_lds_bytes(k, T, DR > 0), st, x, y, valid, indices, dist, D, (uint32_t)K, k, (int)skip_self, groups, items)
    if (D <= 8) FSLIC_KNN(8);
    else if (D <= kKnnRegChannels) FSLIC_KNN(kKnnRegChannels);
    else FSLIC_KNN(0);
#undef FSLIC_KNN
}

}  // namespace

void launch_knn_graph(const float* points, const float* other, const uint8_t* valid, int32_t* indices, float* dist, int N, int D, int K, int k,
                      bool loop, hipStream_t st) {
    const float* y = other ? other : points;
    const bool skip_self = !other && !loop;
    const bool wide = knn_rows(N, K) == 64;
    if (knn_threads(k) == 256) {
        if (wide) launch_form<256, 64>(points, y, valid, indices, dist, N, D, K, k, skip_self, st);
        else launch_form<256, 16>(points, y, valid, indices, dist, N, D, K, k, skip_self, st);
    } else {
        if (wide) launch_form<128, 64>(points, y, valid, indices, dist, N, D, K, k, skip_self, st);
        else launch_form<128, 16>(points, y, valid, indices, dist, N, D, K, k, skip_self, st);
    }
}

}  // namespace fslic
