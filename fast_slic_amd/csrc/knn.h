// knn.h -- exact k nearest neighbours of every node among the nodes of its frame, by squared Euclidean distance over the channels
// (knn.hip, knnapi.cpp; fast_slic_amd/knn.py states the rule).  Internal to the library.
//
// Points and candidates are float [N][D][K], the node innermost; valid is one byte per node [N][K] or nullptr; the result is int32 and
// float [N * K][k], row (f, i) first.  d(i, j) is the left fold from +0.0f over c of t = x[f][c][i] - y[f][c][j], acc = acc + t * t,
// three separately rounded operations a channel; a NaN distance and an invalid node are no candidates, an invalid node's row is all
// padding (-1, +inf), and the k smallest candidates in the order (d, j) are written ascending.
//
// The key.  d >= +0 and never -0, so the bits of d order as an unsigned integer and (bits(d) << 32) | j, compared as one 64-bit
// unsigned value, is the order (d, j).  No two candidates of a row share a key; the empty slot is all ones, above every key (a kept d
// is at most +inf = 0x7F800000).  The result is therefore the same whatever the split below: every partial list is the k smallest of
// its share and the merge is by key.
//
// Launch shape.  A block of T threads is ROWS query rows x S = T / ROWS slices: thread t serves row t % ROWS of the block's row
// group with the candidates W s .. W s + W - 1, + W S, + 2 W S, ... of every tile, s = t / ROWS, W = 4 or 2 neighbouring candidates
// a step (knn.hip).  Each thread keeps a sorted list of k keys in LDS (slot-major, so the lanes of a wave touch consecutive words)
// and its worst key in a register: a candidate is compared with that first, and the insertion behind it is the rare case.  The
// slices' lists are merged in log2(S) rounds of the same insertion, and the block writes its rows' k * ROWS results coalesced,
// padding included: every output element exactly once.
//   T     256 for k <= 16 and 128 above: k * T keys are at most 32 KB of LDS either way.
//   ROWS  64 (a wave is one slice: every LDS read of a candidate is a broadcast) where that fills the chip, 16 (a wave is four
//         slices, four neighbouring addresses a read) otherwise: knn_rows().  Staging costs one load per ROWS pair-channels.
//   form  D <= 8 and D <= 64: the query's channels in registers, a candidate tile of 16 KB in LDS, channel-major.  D > 64: both ends
//         from global memory through the caches, the candidate's address uniform within a slice; correct, not fast.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fslic {

constexpr int kKnnMaxK = 32;               // neighbours a row
constexpr int kKnnTileFloats = 4096;       // floats of a candidate tile
constexpr int kKnnRegChannels = 64;        // D up to which the query's channels live in registers

inline int knn_threads(int k) { return k <= 16 ? 256 : 128; }
// dynamic LDS of a block: its k * T keys and, in the register forms, the tile; at most 48 KB
inline unsigned knn_lds_bytes(int k, int threads, bool tile) { return (unsigned)(k * threads * 8 + (tile ? kKnnTileFloats * 4 : 0)); }
// Rows of a block's row group.  64 where the groups of 64 rows alone give every CU a block (256 CUs); 16 below that, where the
// candidates of a row are better spread over more slices than the chip left idle.  -DFSLIC_KNN_ROWS=16 / =64 (make VAR=.. DEFS=..)
// builds a library with one shape throughout, for the comparison of scripts/knn_bench.py.
inline int knn_rows(int N, int K) {
#ifdef FSLIC_KNN_ROWS
    return FSLIC_KNN_ROWS;
#else
    return (long long)N * ((K + 63) / 64) >= 256 ? 64 : 16;
#endif
}

// indices[(f K + i) k + o], dist[...]: the o-th nearest candidate of node i of frame f of `points` among the nodes of frame f of
// `other` (nullptr: of `points`, node i itself left out unless `loop`), -1 and +inf behind the last one.  One launch.
void launch_knn_graph(const float* points, const float* other, const uint8_t* valid, int32_t* indices, float* dist, int N, int D, int K, int k,
                      bool loop, hipStream_t st);

}  // namespace fslic
