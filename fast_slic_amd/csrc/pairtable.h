// pairtable.h -- the per-frame open-addressing table keyed by a 32-bit label pair, which the region adjacency graph (rag.hip) and the
// overlap of two label maps (compare.hip) accumulate into, and its compact pass (pairtable.hip).  Internal to the library.
//
// Workspace of one accumulate call (offsets from its start, every part 8-byte aligned):
//   header : uint32 overflow flag, uint32 unused, uint64 cursor of compact, uint32 distinct pairs of frame n [N]; padded to 16 bytes
//   keys   : uint32 [N][capacity]     -- the pair's key, never 0 (rag.h, compare.h); 0 = empty slot
//   counts : uint32 [N][capacity]     -- what the pair counts
//   sums   : uint64 [N][capacity][C]  -- the graph's channel sums (C = 0, the overlap and the graph without an image: no such part)
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace fslic {

constexpr int kPairMaxChannels = 4;
constexpr uint32_t kPairMinCapacity = 64u;           // capacities are powers of two in [kPairMinCapacity, kPairMaxCapacity]
constexpr uint32_t kPairMaxCapacity = 1u << 31;
constexpr uint32_t kPairMaxProbe = 255u;             // (linear probing at a load of at most 1/2: runs of a few dozen slots are already rare)
constexpr size_t kPairHeaderFixed = 16;              // sizeof(PairHeader), what _pairtable.py reads the counts behind

struct PairHeader {
    uint32_t overflow;              // != 0: a frame's table got more than half full or a probe run exceeded its bound; the tables are partial
    uint32_t unused;
    unsigned long long cursor;      // rows written by compact
};                                  // then uint32 count[N]: distinct pairs stored per frame
static_assert(sizeof(PairHeader) == kPairHeaderFixed, "the header's layout is part of the ABI (include/fslic_hip.h)");
static __host__ __device__ inline uint32_t* pair_counts(PairHeader* hdr) { return reinterpret_cast<uint32_t*>(hdr + 1); }

inline size_t pair_header_bytes(int N) { return (kPairHeaderFixed + (size_t)N * 4 + 15) & ~(size_t)15; }
inline size_t pair_workspace_bytes(int N, int C, uint32_t capacity) {
    return pair_header_bytes(N) + (size_t)N * (size_t)capacity * (size_t)(8 + 8 * C);
}

struct PairTables {
    PairHeader* hdr;
    uint32_t *key, *cnt;
    unsigned long long* sum;        // (unused when C == 0)
};
inline PairTables pair_tables(void* ws, int N, uint32_t capacity) {
    char* p = reinterpret_cast<char*>(ws);
    const size_t slots = (size_t)N * (size_t)capacity;
    PairTables t;
    t.hdr = reinterpret_cast<PairHeader*>(p);
    t.key = reinterpret_cast<uint32_t*>(p + pair_header_bytes(N));
    t.cnt = t.key + slots;
    t.sum = reinterpret_cast<unsigned long long*>(t.cnt + slots);
    return t;
}

// The occupied slots of every frame's table, densely, in no particular order: keys[r] = frame << 32 | (key - key_bias), counts[r],
// and with `sums` (the graph's table; nullptr: not wanted) the C channel sums of every row.  The caller has cleared the cursor.
// `graph` names the kernel (k_pair_compact<true>: the graph's, <false>: the overlap's), so that a kernel trace tells them apart.
void launch_pair_compact(void* workspace, int N, int C, uint32_t capacity, uint32_t key_bias, bool graph, unsigned long long* keys,
                         int32_t* counts, unsigned long long* sums, unsigned long long max_rows, hipStream_t st);

static __device__ __forceinline__ uint32_t pair_hash(uint32_t v) {
    v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
    return v;
}

// Has the pass been lost (a table declared full)?  Read at the top of every tile: leave then.  A workgroup-scope load, which the
// caches may serve: every tile reads this one word, and at agent scope those reads queue up behind each other at the memory side
// (measured: 22 ns a tile, whatever the tile held).  A stale 0 only delays the leaving.
static __device__ __forceinline__ bool pair_pass_lost(PairHeader* hdr) {
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(&hdr->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != 0u;
}

// One update of frame n's table: finds or claims the slot of `key`, then adds the count and, with kSums, the C channel sums.  The
// table is declared full -- more than half of it taken, or a probe run longer than kPairMaxProbe -- by setting the header's flag;
// the update is then lost, and so is the whole pass (the caller starts over with a larger table).  S: the type of the addends of
// the sums, uint32_t (the graph's pixel tiles) or unsigned long long (merge.hip, whose addends are sums already).
template <bool kSums, class S = uint32_t>
static __device__ __forceinline__ void pair_table_add(PairHeader* __restrict__ hdr, uint32_t* __restrict__ tkey, uint32_t* __restrict__ tcnt,
                                                      unsigned long long* __restrict__ tsum, int n, uint32_t cap_mask, uint32_t key,
                                                      uint32_t cnt, int C = 0, const S* s = nullptr) {
    const size_t base = (size_t)n * ((size_t)cap_mask + 1);
    uint32_t h = pair_hash(key) & cap_mask;
    for (uint32_t probe = 0; probe <= min(cap_mask, kPairMaxProbe); ++probe) {
        uint32_t cur = __hip_atomic_load(&tkey[base + h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0u) {
            cur = atomicCAS(&tkey[base + h], 0u, key);
            if (cur == 0u) {
                if (atomicAdd(pair_counts(hdr) + n, 1u) > (cap_mask >> 1)) atomicExch(&hdr->overflow, 1u);     // more than capacity / 2 pairs
                cur = key;
            }
        }
        if (cur == key) {
            atomicAdd(&tcnt[base + h], cnt);
            if (kSums) {
#pragma unroll
                for (int c = 0; c < kPairMaxChannels; ++c)               // (a run-time index would send s[] to scratch memory)
                    if (c < C) atomicAdd(&tsum[(base + h) * (size_t)C + c], (unsigned long long)s[c]);
            }
            return;
        }
        h = (h + 1u) & cap_mask;
    }
    atomicExch(&hdr->overflow, 1u);
}

}  // namespace fslic
