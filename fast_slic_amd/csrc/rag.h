// rag.h -- the region adjacency graph of a label map (rag.hip, ragapi.cpp).  Internal to the library.
//
// Workspace of one fslic_hip_rag_accumulate call (offsets from its start, every part 8-byte aligned):
//   header   : uint32 overflow flag, uint32 unused, uint64 cursor of compact, uint32 distinct pairs of frame n [N]; padded to 16 bytes
//   keys     : uint32 [N][capacity]     -- lo << 16 | hi of the unordered label pair (lo < hi < K <= 65534, so never 0); 0 = empty slot
//   boundary : uint32 [N][capacity]     -- neighbouring pixel pairs of that label pair
//   contrast : uint64 [N][capacity][C]  -- per channel the sum of |difference| over those pixel pairs (C = 0: no image, no table)
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace fslic {

constexpr int kRagMaxChannels = 4;
constexpr uint32_t kRagMinCapacity = 64u;            // capacities are powers of two in [kRagMinCapacity, kRagMaxCapacity]
constexpr uint32_t kRagMaxCapacity = 1u << 31;
constexpr size_t kRagHeaderFixed = 16;               // sizeof(RagHeader), what rag.py reads the counts behind

struct RagHeader {
    uint32_t overflow;              // != 0: a frame's table got more than half full or a probe run exceeded its bound; the tables are partial
    uint32_t unused;
    unsigned long long cursor;      // rows written by compact
};                                  // then uint32 count[N]: distinct pairs stored per frame
static_assert(sizeof(RagHeader) == kRagHeaderFixed, "the header's layout is part of the ABI (include/fslic_hip.h)");
static __host__ __device__ inline uint32_t* rag_counts(RagHeader* hdr) { return reinterpret_cast<uint32_t*>(hdr + 1); }

inline size_t rag_header_bytes(int N) { return (kRagHeaderFixed + (size_t)N * 4 + 15) & ~(size_t)15; }
inline size_t rag_workspace_bytes(int N, int C, uint32_t capacity) {
    return rag_header_bytes(N) + (size_t)N * (size_t)capacity * (size_t)(8 + 8 * C);
}

// labels: N x H x W of the given PoolLabel type (pool.h); image: N x H x W x C uint8 or nullptr (then C == 0)
void launch_rag_accumulate(const void* labels, int label_type, const uint8_t* image, void* workspace,
                           int N, int C, int H, int W, int K, int connectivity, uint32_t capacity, hipStream_t st);
void launch_rag_compact(void* workspace, int N, int C, uint32_t capacity, unsigned long long* keys, int32_t* boundary,
                        unsigned long long* contrast, unsigned long long max_edges, hipStream_t st);

}  // namespace fslic
