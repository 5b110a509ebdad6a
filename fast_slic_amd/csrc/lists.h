// lists.h -- neighbour lists on the device: their layout, the rule of what is trusted, and the tile of 64 rows with its LDS window that
// the list kernels of aggregate.hip, attend.hip and message.hip walk (pixel.hip takes row_bound only).  Internal to the library.
//
// Lists: one CSR over the R = N * K rows (frame, node): offsets int64 [R + 1], indices int32 [nnz] (node numbers inside the frame).
// Transposed lists (crf_torch.transpose_batch_csr): t_offsets int64 [R + 1] over the targets, t_entries int32 [nnz] the entry p and
// t_rows int32 [nnz] the row of p, per transposed position.  Features float [N][C][K]; a per-entry array is float [heads][nnz].
// Nothing a kernel reads from device memory becomes an address before it is checked: row bounds are clamped into [0, nnz] and an end
// before its start is an empty row; an index outside [0, K), an entry outside [0, nnz) and a row outside the target's frame
// contribute nothing.
//
// The tile.  A block of 256 threads takes an item = (tile, group): 64 consecutive rows, lane l of every wave owns row 64 * tile + l,
// and the group says which channels, heads or features the block's four waves serve.  The block first copies the first kAggStage
// positions behind the tile's first row into LDS (coalesced), and a lane walking its row takes a position from there when it lies in
// that window and from global memory otherwise: a hub row longer than the window is walked in full, in order.  Direct form: a
// position is the entry itself and the window holds its index.  Transposed form: position q holds entry t_entries[q], and the window
// holds the row of that entry, or -1 where the entry or the row is out of range, and the entry where the kernel asks for it (KEEP_P).
// A window of floats per entry (weights, scores, messages) is copied coalesced in the direct form; in the transposed form it is
// gathered through the entries, 64 independent loads an instruction, not one dependent load a step of a walk: by the block in the pass
// that stages the positions where the block shares one window, by each wave after a barrier where every wave has its own.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "launch.h"

namespace fslic {

constexpr int kAggRows = 64;               // rows of a tile: one wavefront of lanes
constexpr int kAggStage = 1024;            // positions of the LDS window: 16 a row, a SLIC map has about 6
constexpr int kAggWaveChannels = 8;        // channels a lane accumulates at once, where the group says channels (aggregate.h, attend.h's apply)
constexpr int kAggBlockChannels = 32;      // channels of such an item: 4 waves x 8

// the clamped bound of a row: offsets are not trusted
__device__ __forceinline__ int row_bound(const long long* __restrict__ offsets, uint32_t r, int nnz) {
    const long long o = offsets[r];
    return o < 0 ? 0 : o > (long long)nnz ? nnz : (int)o;
}

// LDS arrays are handed over with their address space, so that a read "from the window, else from global memory" stays two loads (a
// ds_read and a global_load) and is not merged into one flat load of a selected address.
typedef __attribute__((address_space(3))) int LdsInt;
typedef __attribute__((address_space(3))) float LdsFloat;

struct ListTile {
    uint32_t tile, group, row0;            // item = tile * groups + group; row0 = 64 * tile < R
    int lo, staged;                        // the window: positions lo .. lo + staged - 1
};
__device__ __forceinline__ ListTile list_tile(unsigned long long item, uint32_t groups, const long long* __restrict__ offsets, int nnz) {
    ListTile T;
    T.tile = (uint32_t)(item / groups), T.group = (uint32_t)(item - (unsigned long long)T.tile * groups);
    T.row0 = T.tile * (uint32_t)kAggRows;
    T.lo = row_bound(offsets, T.row0, nnz);
    T.staged = nnz - T.lo < kAggStage ? nnz - T.lo : kAggStage;
    return T;
}

// What of the window belongs to the tile's own rows (a kernel that writes per entry stores that part): rows row0 .. rows_end - 1 hold
// the positions lo .. hi - 1, the first `own` of them in the window.
struct ListTileOwn {
    uint32_t rows_end;
    int hi, own;
};
__device__ __forceinline__ ListTileOwn list_tile_own(const ListTile& T, const long long* __restrict__ offsets, uint32_t R, int nnz) {
    ListTileOwn o;
    o.rows_end = R - T.row0 < (uint32_t)kAggRows ? R : T.row0 + (uint32_t)kAggRows;
    o.hi = row_bound(offsets, o.rows_end, nnz);
    o.own = o.hi <= T.lo ? 0 : o.hi - T.lo < T.staged ? o.hi - T.lo : T.staged;
    return o;
}

// A lane's row r < R: its positions [begin, end), frame f, node i, and base = f * K, the row of the frame's node 0.
struct ListRow {
    int begin, end;
    uint32_t f, i, base;
};
__device__ __forceinline__ ListRow list_row(const long long* __restrict__ offsets, uint32_t r, uint32_t K, int nnz) {
    ListRow row;
    row.begin = row_bound(offsets, r, nnz), row.end = row_bound(offsets, r + 1u, nnz);
    if (row.end < row.begin) row.end = row.begin;
    row.f = r / K, row.base = row.f * K, row.i = r - row.base;
    return row;
}

// One position pos in [0, nnz).  Direct (ia = indices): node = the index, p = pos.  Transposed (ia = t_entries, ib = t_rows): p =
// the entry and node = its row over (frame, node), or both -1 unless p lies in [0, nnz) and the row in [0, R): either says alone
// whether the position counts, so what is gathered through p reads p only.
struct ListEntry {
    int node, p;
};
template <bool BACK>
__device__ __forceinline__ ListEntry list_entry(int pos, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib, uint32_t R, int nnz) {
    if (!BACK) return {ia[pos], pos};
    const int p = ia[pos], r = ib[pos];
    const bool ok = (uint32_t)p < (uint32_t)nnz && (uint32_t)r < R;
    return {ok ? r : -1, ok ? p : -1};
}

// The block copies the window's positions into s_node [kAggStage] and, with KEEP_P (transposed form only), s_p [kAggStage].  With
// WITH_F it copies the block's window of a per-entry float array `src` [nnz] into s_f [kAggStage] in the same pass, the transposed
// form through the entry it has just read (+0.0 where the node is -1): the loads of a position are in flight together.  Thread x
// writes the places x, x + 256, ..; barriers are the caller's.
template <bool BACK, bool KEEP_P, bool WITH_F = false>
__device__ __forceinline__ void list_stage(const ListTile& T, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib, uint32_t R, int nnz,
                                           LdsInt* s_node, LdsInt* s_p, const float* __restrict__ src = nullptr, LdsFloat* s_f = nullptr) {
    for (int t = threadIdx.x; t < T.staged; t += 256) {
        const ListEntry e = list_entry<BACK>(T.lo + t, ia, ib, R, nnz);
        s_node[t] = e.node;
        if (KEEP_P) s_p[t] = e.p;
        if (WITH_F) s_f[t] = !BACK || e.p >= 0 ? src[(size_t)e.p] : 0.0f;
    }
}

// A wave's own window of a per-entry float array `src` [nnz] into s_f [kAggStage] (every wave of the block another array).  Transposed
// form: gathered through the staged entries, behind the barrier that follows list_stage<true, true>; +0.0 where the entry is -1.
template <bool BACK>
__device__ __forceinline__ void list_stage_floats(const ListTile& T, const float* __restrict__ src, const LdsInt* s_p, LdsFloat* s_f, uint32_t lane) {
    for (int t = (int)lane; t < T.staged; t += 64) s_f[t] = !BACK ? src[(size_t)(T.lo + t)] : s_p[t] >= 0 ? src[(size_t)s_p[t]] : 0.0f;
}

// One step of the walk of a row: a kernel visits the positions pos = row.begin .. row.end - 1 in ascending order and asks here what
// each one is.  win: the position lies in the window, at place t.  p: the entry (the transposed form without KEEP_P does not know it:
// -1).  j: the node inside the frame, the neighbour's in the direct form, the entry's row's in the transposed form.  valid: j < K,
// which in the transposed form says that p is an entry and its row lies in the target's frame; a kernel that writes per entry writes
// +0.0 for the others, every other kernel skips them.
struct ListPos {
    bool win, valid;
    uint32_t t, j;
    int p;
};
template <bool BACK, bool KEEP_P>
__device__ __forceinline__ ListPos list_at(const ListTile& T, const ListRow& row, int pos, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib,
                                          uint32_t K, uint32_t R, int nnz, const LdsInt* s_node, const LdsInt* s_p) {
    ListPos o;
    o.t = (uint32_t)(pos - T.lo);                      // a row that garbage offsets put in front of the window wraps beyond it: t is unsigned
    o.win = o.t < (uint32_t)T.staged;
    ListEntry e;
    if (o.win) e = {s_node[o.t], KEEP_P ? s_p[o.t] : pos};
    else e = list_entry<BACK>(pos, ia, ib, R, nnz);
    o.j = (uint32_t)e.node - (BACK ? row.base : 0u);
    o.p = BACK && !KEEP_P ? -1 : e.p;
    o.valid = o.j < K;
    return o;
}

// The launch of a tile kernel over N * K rows and `groups` groups a tile: grid-stride over the items.
struct ListLaunch {
    uint32_t R, groups;
    unsigned long long items;
    dim3 grid;
};
static inline ListLaunch list_launch(int N, int K, uint32_t groups) {
    ListLaunch g;
    g.R = (uint32_t)N * (uint32_t)K, g.groups = groups;
    g.items = (unsigned long long)((g.R + kAggRows - 1u) / kAggRows) * groups;
    g.grid = dim3((unsigned)tile_grid(g.items, 1));
    return g;
}

}  // namespace fslic
