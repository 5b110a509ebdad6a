// pairtable.hip -- the compact pass of the label pair table (pairtable.h), gfx950.
//   k_pair_compact : the occupied slots of every frame's table, densely, in no particular order.  A wavefront takes a chunk of 1024
//                    slots (16 a lane, in registers), counts the occupied ones by ballots and adds the cursor once per chunk.
#include "device_common.h"
#include "pairtable.h"

namespace fslic {

constexpr int kCompactRounds = 16;               // slots a lane of k_pair_compact looks at: one cursor add per 1024 slots

// kSums: the graph's table, whose rows carry C channel sums (C == 0 without an image); false: the overlap's, keys and counts alone.
template <bool kSums>
__global__ __launch_bounds__(256) void k_pair_compact(PairHeader* __restrict__ hdr, const uint32_t* __restrict__ tkey, const uint32_t* __restrict__ tcnt,
                                                      const unsigned long long* __restrict__ tsum, int C, uint32_t key_bias,
                                                      unsigned long long capacity, unsigned long long total,
                                                      unsigned long long* __restrict__ keys, int32_t* __restrict__ count,
                                                      unsigned long long* __restrict__ sums, unsigned long long max_rows) {
    const int lane = LANE();
    const unsigned long long nwaves = (unsigned long long)gridDim.x * 4ull, chunk = 64ull * kCompactRounds;
    const unsigned long long nchunks = (total + chunk - 1) / chunk;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (unsigned long long c = (unsigned long long)blockIdx.x * 4ull + (threadIdx.x >> 6); c < nchunks; c += nwaves) {
        uint32_t key[kCompactRounds];
        uint32_t before[kCompactRounds];                                   // occupied slots of the chunk in earlier rounds
        uint32_t sum = 0;
#pragma unroll
        for (int r = 0; r < kCompactRounds; ++r) {
            const unsigned long long i = c * chunk + (unsigned long long)r * 64ull + lane;
            key[r] = i < total ? tkey[i] : 0u;
        }
#pragma unroll
        for (int r = 0; r < kCompactRounds; ++r) {
            const unsigned long long taken = ballot(key[r] != 0u);
            before[r] = sum + (uint32_t)__popcll(taken & below);
            sum += (uint32_t)__popcll(taken);
        }
        if (sum == 0u) continue;
        // one add of the cursor per chunk: the adds of one word queue up behind each other
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&hdr->cursor, (unsigned long long)sum);
        base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
               (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
#pragma unroll
        for (int r = 0; r < kCompactRounds; ++r) {
            const unsigned long long i = c * chunk + (unsigned long long)r * 64ull + lane;
            const unsigned long long pos = base + before[r];
            if (key[r] != 0u && pos < max_rows) {
                keys[pos] = ((i / capacity) << 32) | (unsigned long long)(key[r] - key_bias);
                count[pos] = (int32_t)tcnt[i];
            }
        }
        // The rows' channel sums, in a loop of its own that reads the chunk's keys again (the caches have them) and counts the rows
        // again: inside the unrolled rounds above the copies kept 97 VGPRs alive, 4 waves a SIMD; so it is 67 and 7.
        if (kSums && sums) {
            uint32_t row = 0;
#pragma unroll 1
            for (int r = 0; r < kCompactRounds; ++r) {
                const unsigned long long i = c * chunk + (unsigned long long)r * 64ull + lane;
                const bool mine = i < total && tkey[i] != 0u;
                const unsigned long long taken = ballot(mine);
                const unsigned long long pos = base + row + (uint32_t)__popcll(taken & below);
                row += (uint32_t)__popcll(taken);
                if (mine && pos < max_rows)
                    for (int ch = 0; ch < C; ++ch) sums[pos * (unsigned long long)C + ch] = tsum[i * (unsigned long long)C + ch];
            }
        }
    }
}

void launch_pair_compact(void* workspace, int N, int C, uint32_t capacity, uint32_t key_bias, bool graph, unsigned long long* keys,
                         int32_t* counts, unsigned long long* sums, unsigned long long max_rows, hipStream_t st) {
    const PairTables t = pair_tables(workspace, N, capacity);
    const unsigned long long total = (unsigned long long)N * (unsigned long long)capacity;
    const dim3 grid(tile_grid(total, 4ull * 64ull * kCompactRounds)), block(256);
    if (graph) launch(k_pair_compact<true>, grid, block, 0, st, t.hdr, t.key, t.cnt, t.sum, C, key_bias, (unsigned long long)capacity, total, keys, counts, sums, max_rows);
    else launch(k_pair_compact<false>, grid, block, 0, st, t.hdr, t.key, t.cnt, t.sum, C, key_bias, (unsigned long long)capacity, total, keys, counts, sums, max_rows);
}

}  // namespace fslic
