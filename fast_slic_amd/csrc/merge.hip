// merge.hip -- merging superpixels on the region adjacency graph, gfx950 (fast_slic_amd/merge.py): each node's best edge, the groups
// of a set of joined edges, the relabelled pixels, and the graph of the groups.  Layout of the scratch: merge.h.  A launch only reads
// what an earlier launch completed, except for the parent words of k_merge_hook and k_merge_flatten, which move one way (a parent
// only ever becomes a smaller node of the same group), so that a reader is right with the old value and with the new one.
//   k_merge_best<false> : one thread per edge; an eligible edge offers its key (weight bits << 32 | position) to the words of its two
//                         nodes with a 64-bit integer atomicMin: the smallest key wins whatever the order.
//   k_merge_best<true>  : join[e] = the key of e is the word of one of its nodes.
//   k_merge_init        : parent = the node itself, or kMergeAbsent for a node without members.
//   k_merge_hook        : one thread per joined edge; the union is a CAS on the larger root's own word (a root is only ever given a
//                         smaller parent, so the root of a group is its leader whatever the order).  A walk to the root moves every
//                         node it passes to its grandparent (atomicMin), so a path of 65534 nodes does not leave a chain of that
//                         length to every later walk.
//   k_merge_flatten     : parent = leader for every node, and the leaders of every chunk of 256 nodes counted.
//   k_merge_scan, k_merge_rank : the rank of the leaders as a prefix sum: per frame the scan of the chunk counts, per chunk the ranks.
//   k_merge_output      : mapping = the rank at the node's leader, -1 for an absent node.
//   k_merge_labels      : out = mapping[frame][label], four pixels a thread: one 8 / 16 / 2 x 16 byte load and one 16 byte store;
//                         the pixels before the first 16-byte boundary of `out` and the last few are single ones.
//   k_merge_contract    : one thread per edge; its boundary and its contrast row go to the pair of its nodes' groups in the label
//                         pair table (pairtable.h), which the graph's compact pass reads out.
// No kernel waits for another block.  All integer work: the result is the same bits from run to run.
#include "device_common.h"
#include "labels.h"
#include "merge.h"

namespace fslic {

static_assert(kMergeChunk == 256, "256 threads: one node of a chunk each");
static_assert((65534 + kMergeChunk - 1) / kMergeChunk <= 256, "k_merge_scan: the chunks of a frame are one block's");

// The edge kernels: one edge a thread and round, with at most the 2048 blocks of 256 threads the chip holds at once (8 a CU).
static inline dim3 edge_grid(long long E) { return dim3(min(tile_grid_dim((unsigned long long)E, 256).x, 2048u)); }

// ---- each node's best edge --------------------------------------------------------------------
template <bool kMark>
__global__ __launch_bounds__(256) void k_merge_best(const long long* __restrict__ ei, const long long* __restrict__ offsets, const float* __restrict__ weight,
                                                    unsigned long long* slot, uint8_t* __restrict__ join, int N, uint32_t K, long long E,
                                                    bool all, double threshold) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const float w = weight[e];
        const unsigned long long a = (unsigned long long)ei[e], b = (unsigned long long)ei[E + e];
        const bool ok = (all || (double)w < threshold) && a < K && b < K;
        if (!ok) {
            if (kMark) join[e] = 0;
            continue;
        }
        const int f = frame_of(offsets, N, e);
        // non-negative float bits order like the values; -0.0 is +0.0
        const unsigned long long key = ((unsigned long long)(w == 0.0f ? 0u : __float_as_uint(w)) << 32) | (unsigned long long)(uint32_t)(e - offsets[f]);
        unsigned long long* s = slot + (size_t)f * K;
        if (!kMark) {
            atomicMin(s + a, key);
            atomicMin(s + b, key);
        } else {
            join[e] = (s[a] == key || s[b] == key) ? 1 : 0;
        }
    }
}

void launch_merge_best_edges(const long long* edge_index, const long long* offsets, const float* weight, bool all, double threshold,
                             uint8_t* join, void* workspace, int N, int K, long long E, hipStream_t st) {
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(workspace);
    const dim3 grid = edge_grid(E), block(256);
    launch(k_merge_best<false>, grid, block, 0, st, edge_index, offsets, weight, slot, join, N, (uint32_t)K, E, all, threshold);
    launch(k_merge_best<true>, grid, block, 0, st, edge_index, offsets, weight, slot, join, N, (uint32_t)K, E, all, threshold);
}

// ---- the groups of the joined edges -----------------------------------------------------------
template <class M>
__global__ __launch_bounds__(256) void k_merge_init(const M* __restrict__ members, uint32_t* __restrict__ parent, uint32_t K, uint32_t total) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u)
        parent[i] = !members || members[i] > M(0) ? i % K : kMergeAbsent;
}

// The root of a's tree; every node on the way is moved to its grandparent.  A node that has a parent is never a root again, so the
// atomicMin never touches the word a union's CAS is waiting for.
static __device__ __forceinline__ uint32_t find_halving(uint32_t* par, uint32_t a) {
    uint32_t p = ld_now(par + a);
    while (p != a) {
        const uint32_t g = ld_now(par + p);
        if (g != p) atomicMin(par + a, g);
        a = p;
        p = g;
    }
    return a;
}
// Joins the sets of a and b: the larger of the two roots gets the smaller as its parent, by CAS on the root's own word.  A CAS that
// fails returns the parent another thread gave that root, and the walk goes on from there: every round ends or moves to a smaller index.
static __device__ __forceinline__ void unite(uint32_t* par, uint32_t a, uint32_t b) {
    for (;;) {
        a = find_halving(par, a);
        b = find_halving(par, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicCAS(par + a, a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(256) void k_merge_hook(const long long* __restrict__ ei, const long long* __restrict__ offsets, const uint8_t* __restrict__ join,
                                                    uint32_t* parent, int N, uint32_t K, long long E) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        if (!join[e]) continue;
        const unsigned long long a = (unsigned long long)ei[e], b = (unsigned long long)ei[E + e];
        if (a >= K || b >= K || a == b) continue;
        uint32_t* par = parent + (size_t)frame_of(offsets, N, e) * K;
        if (ld_now(par + a) == kMergeAbsent || ld_now(par + b) == kMergeAbsent) continue;      // (absent since k_merge_init, for good)
        unite(par, (uint32_t)a, (uint32_t)b);
    }
}

// The node kernels: a block takes chunks of 256 nodes of one frame, thread t the node c * 256 + t.
__global__ __launch_bounds__(256) void k_merge_flatten(uint32_t* parent, uint32_t* __restrict__ sums, uint32_t K, uint32_t nb, uint32_t chunks) {
    __shared__ uint32_t s_w[4];
    const int lane = LANE();
    const uint32_t wave = rfl(threadIdx.x >> 6);
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint32_t n = c / nb, v = (c - n * nb) * kMergeChunk + threadIdx.x;
        uint32_t* par = parent + (size_t)n * K;
        const uint32_t a = v < K ? ld_now(par + v) : kMergeAbsent;
        if (a != kMergeAbsent) {
            uint32_t lead = a;
            for (uint32_t q; (q = ld_now(par + lead)) != lead;) lead = q;
            if (lead != a) st_now(par + v, lead);
        }
        const uint32_t leaders = (uint32_t)__popcll(ballot(a == v));       // (v >= K: a is kMergeAbsent, never v)
        if (lane == 0) s_w[wave] = leaders;
        __syncthreads();
        if (threadIdx.x == 0) sums[c] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}

// per frame one block: sums[n][b] becomes the leaders of the chunks before b, counts[n] their total
__global__ __launch_bounds__(256) void k_merge_scan(uint32_t* __restrict__ sums, int32_t* __restrict__ counts, int N, uint32_t nb) {
    __shared__ uint32_t s_w[4];
    const int lane = LANE();
    const uint32_t wave = rfl(threadIdx.x >> 6);
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        uint32_t* s = sums + (size_t)n * nb;
        const uint32_t v = threadIdx.x < nb ? s[threadIdx.x] : 0u;
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
        if (threadIdx.x < nb) s[threadIdx.x] = before + incl - v;
        if (threadIdx.x == 0) counts[n] = (int32_t)total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_merge_rank(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ sums, uint32_t* __restrict__ rank,
                                                    uint32_t K, uint32_t nb, uint32_t chunks) {
    __shared__ uint32_t s_w[4];
    const int lane = LANE();
    const uint32_t wave = rfl(threadIdx.x >> 6);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint32_t n = c / nb, v = (c - n * nb) * kMergeChunk + threadIdx.x;
        const bool leader = v < K && parent[(size_t)n * K + v] == v;
        const unsigned long long m = ballot(leader);
        if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = sums[c];
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) before += w < wave ? s_w[w] : 0u;
        if (leader) rank[(size_t)n * K + v] = before + (uint32_t)__popcll(m & below);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_merge_output(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rank, int32_t* __restrict__ mapping,
                                                      uint32_t K, uint32_t total) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const uint32_t lead = parent[i];
        mapping[i] = lead == kMergeAbsent ? -1 : (int32_t)rank[i - i % K + lead];
    }
}

void launch_merge_components(const long long* edge_index, const long long* offsets, const uint8_t* join, const void* members,
                             int members_type, int32_t* mapping, int32_t* counts, void* workspace, int N, int K, long long E, hipStream_t st) {
    const uint32_t total = (uint32_t)N * (uint32_t)K, nb = (uint32_t)merge_chunks_per_frame(K), chunks = nb * (uint32_t)N;
    char* ws = reinterpret_cast<char*>(workspace);
    uint32_t* parent = reinterpret_cast<uint32_t*>(ws);
    uint32_t* rank = reinterpret_cast<uint32_t*>(ws + merge_align((size_t)total * 4));
    uint32_t* sums = reinterpret_cast<uint32_t*>(ws + 2 * merge_align((size_t)total * 4));
    const dim3 block(256), nodes = tile_grid_dim(total, 256), per_chunk = tile_grid_dim(chunks, 1);
    if (members_type == kLabelI64) launch(k_merge_init<int64_t>, nodes, block, 0, st, reinterpret_cast<const int64_t*>(members), parent, (uint32_t)K, total);
    else launch(k_merge_init<int32_t>, nodes, block, 0, st, reinterpret_cast<const int32_t*>(members), parent, (uint32_t)K, total);
    if (E > 0) launch(k_merge_hook, edge_grid(E), block, 0, st, edge_index, offsets, join, parent, N, (uint32_t)K, E);
    launch(k_merge_flatten, per_chunk, block, 0, st, parent, sums, (uint32_t)K, nb, chunks);
    launch(k_merge_scan, tile_grid_dim((unsigned long long)N, 1), block, 0, st, sums, counts, N, nb);
    launch(k_merge_rank, per_chunk, block, 0, st, parent, sums, rank, (uint32_t)K, nb, chunks);
    launch(k_merge_output, nodes, block, 0, st, parent, rank, mapping, (uint32_t)K, total);
}

// ---- the relabelled pixels --------------------------------------------------------------------
template <class L> struct Four;          // four labels as one load (int64: two loads of 16 bytes)
template <> struct Four<uint16_t> { typedef uint2 type; };
template <> struct Four<int32_t> { typedef uint4 type; };

template <class L>
static __device__ __forceinline__ int32_t merged_label(const L* __restrict__ labels, const int32_t* __restrict__ mapping, uint32_t i, uint32_t frame, uint32_t K) {
    const uint32_t l = canon(labels[i], K);
    return l < K ? mapping[(size_t)frame * K + l] : -1;
}

// head: the pixels before the first 16-byte boundary of `out`; groups: the fours that follow; the rest (fewer than four) are the tail.
// kVector: labels + head is aligned for one load of four labels (two of 16 bytes for int64).
template <class L, bool kVector>
__global__ __launch_bounds__(256) void k_merge_labels(const L* __restrict__ labels, const int32_t* __restrict__ mapping, int32_t* __restrict__ out,
                                                      uint32_t P, uint32_t K, uint32_t total, uint32_t head, uint32_t groups) {
    for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < groups; g += gridDim.x * 256u) {
        const uint32_t i = head + 4u * g;
        L v[4];
        if constexpr (kVector && sizeof(L) == 8) {
            const uint4 lo = *reinterpret_cast<const uint4*>(labels + i), hi = *reinterpret_cast<const uint4*>(labels + i + 2);
            __builtin_memcpy(&v[0], &lo, 16);
            __builtin_memcpy(&v[2], &hi, 16);
        } else if constexpr (kVector) {
            typedef typename Four<L>::type V;
            const V q = *reinterpret_cast<const V*>(labels + i);
            __builtin_memcpy(v, &q, sizeof(V));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = labels[i + k];
        }
        const uint32_t f0 = i / P, r0 = i - f0 * P;
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t f = r0 + (uint32_t)k < P ? f0 : (i + (uint32_t)k) / P;      // (a four across the end of a frame; P may be 1)
            const uint32_t l = canon(v[k], K);
            o[k] = l < K ? (uint32_t)mapping[(size_t)f * K + l] : 0xFFFFFFFFu;
        }
        st_stream(reinterpret_cast<uint4*>(out + i), make_uint4(o[0], o[1], o[2], o[3]));
    }
    if (blockIdx.x == 0) {
        const uint32_t tail0 = head + 4u * groups, ntail = total - tail0;
        if (threadIdx.x < head + ntail) {
            const uint32_t i = threadIdx.x < head ? threadIdx.x : tail0 + (threadIdx.x - head);
            out[i] = merged_label(labels, mapping, i, i / P, K);
        }
    }
}

void launch_merge_labels(const void* labels, int label_type, const int32_t* mapping, int32_t* out, int N, long long P, int K, hipStream_t st) {
    const uint32_t total = (uint32_t)((long long)N * P);
    uint32_t head = (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) / 4u;      // (out is an int32 pointer: 4-byte aligned)
    if (head > total) head = total;
    const uint32_t groups = (total - head) / 4u;
    const dim3 grid = tile_grid_dim(groups, 256), block(256);
    with_label_type(labels, label_type, [&](auto* la) {
        using L = std::decay_t<decltype(*la)>;
        const size_t align = sizeof(L) == 8 ? 16 : 4 * sizeof(L);
        if ((reinterpret_cast<uintptr_t>(la + head) & (align - 1)) == 0)
            launch(k_merge_labels<L, true>, grid, block, 0, st, la, mapping, out, (uint32_t)P, (uint32_t)K, total, head, groups);
        else
            launch(k_merge_labels<L, false>, grid, block, 0, st, la, mapping, out, (uint32_t)P, (uint32_t)K, total, head, groups);
    });
}

// ---- the graph of the groups ------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_merge_contract(const long long* __restrict__ ei, const long long* __restrict__ offsets, const int32_t* __restrict__ boundary,
                                                        const long long* __restrict__ contrast, const int32_t* __restrict__ mapping,
                                                        PairHeader* __restrict__ hdr, uint32_t* __restrict__ tkey, uint32_t* __restrict__ tcnt,
                                                        unsigned long long* __restrict__ tsum, int N, int C, uint32_t K, uint32_t K2, long long E,
                                                        uint32_t cap_mask) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        if (pair_pass_lost(hdr)) return;
        const unsigned long long a = (unsigned long long)ei[e], b = (unsigned long long)ei[E + e];
        if (a >= K || b >= K) continue;
        const int f = frame_of(offsets, N, e);
        const uint32_t ga = (uint32_t)mapping[(size_t)f * K + a], gb = (uint32_t)mapping[(size_t)f * K + b];      // (-1 is above any K2)
        if (ga >= K2 || gb >= K2 || ga == gb) continue;
        unsigned long long s[kPairMaxChannels] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < kPairMaxChannels; ++c)
            if (c < C) s[c] = (unsigned long long)contrast[(size_t)e * (size_t)C + c];
        pair_table_add<true>(hdr, tkey, tcnt, tsum, f, cap_mask, (min(ga, gb) << 16) | max(ga, gb), (uint32_t)boundary[e], C, s);
    }
}

void launch_merge_contract(const long long* edge_index, const long long* offsets, const int32_t* boundary, const long long* contrast,
                           const int32_t* mapping, void* workspace, int N, int C, int K, int K2, long long E, uint32_t capacity, hipStream_t st) {
    const PairTables t = pair_tables(workspace, N, capacity);
    launch(k_merge_contract, edge_grid(E), dim3(256), 0, st, edge_index, offsets, boundary, contrast, mapping,
           t.hdr, t.key, t.cnt, t.sum, N, C, (uint32_t)K, (uint32_t)K2, E, capacity - 1u);
}

}  // namespace fslic
