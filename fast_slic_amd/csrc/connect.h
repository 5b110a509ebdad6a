// connect.h -- connectivity on label tensors: components and the min-size merge (connect.hip, connectapi.cpp;
// fast_slic_amd/connect.py states the five rules).  Internal to the library.
//
// A frame has H x W pixels, p = y * W + x its raster index (N * H * W < 2^31, so every index and every count is a uint32 below 2^31).
// Workspace of one call: 8 bytes per pixel plus 4 bytes per chunk of 1024 pixels, every part 16-byte aligned:
//   parent : uint32 [N][H W]   a pixel of p's component with a raster index <= p; after k_connect_flatten the component's leader
//   area   : uint32 [N][H W]   k_connect_tiles: at the first pixel of a tile's component its pixels in the tile, 0 elsewhere;
//                              k_connect_flatten: at a leader the component's pixels; k_connect_apply overwrites the leaders' words
//                              with the label (the component number), or with kConnectLink | the leader the label comes from (rule 4)
//   sums   : uint32 [N][ceil(H W / 1024)]   numbered leaders per chunk, then (k_connect_scan) those of the frame's chunks before it
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace fslic {

constexpr int kConnectTileRows = 16;             // a tile: 64 columns x 16 rows, one 256-thread block
constexpr int kConnectChunk = 1024;              // pixels of one block of the rank passes
constexpr uint32_t kConnectLink = 0x80000000u;   // an area word that names a leader instead of a label

inline size_t connect_align(size_t b) { return (b + 15) & ~(size_t)15; }
inline size_t connect_chunks(int N, int H, int W) {
    return (size_t)N * (((size_t)H * (size_t)W + kConnectChunk - 1) / kConnectChunk);
}
inline size_t connect_workspace_bytes(int N, int H, int W) {
    const size_t P = (size_t)N * (size_t)H * (size_t)W;
    return 2 * connect_align(P * 4) + connect_align(connect_chunks(N, H, W) * 4);
}

// labels: N x H x W of the given LabelType (labels.h), compared for equality only.  enforce == false: out = the component number of
// every pixel, counts[n] = the components of frame n.  enforce == true: out = the labels of rules 2 to 4 with `min_size` (at most
// H W + 1), counts[n] = the kept components, 1 when there are none.  Every launch goes to `st`; nothing waits on the host.
void launch_connect(const void* labels, int label_type, int32_t* out, int32_t* counts, void* workspace, int N, int H, int W,
                    bool enforce, uint32_t min_size, hipStream_t st);

}  // namespace fslic
