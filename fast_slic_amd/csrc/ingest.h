// ingest.h -- frames of any torch layout into the engine's form (ingest.hip, ingestapi.cpp; Python: fast_slic_amd/frames.py).  Internal
// to the library.
//
// Source: N frames of 3 channels of H x W elements of one type (uint8, float16, bfloat16, float32), element (n, c, y, x) at
// src + n * strides[0] + c * strides[1] + y * strides[2] + x * strides[3], strides in ELEMENTS and of any value (0 included: a gray
// plane expanded to three channels).  Output: frame n is uint8 [H][W][3] interleaved at out + n * pitch, pitch >= 3 H W and a multiple
// of 16; the bytes [3 H W, pitch) of every frame are written as 0 and nothing outside [out, out + N * pitch) is touched.
// Arithmetic of a float source, per element, in float32 (float16 and bfloat16 widen exactly first): v = x * scale, one rounding;
// NaN -> 0; clamp to [0, 255]; round to nearest, ties to even.  One multiplication and no addition: there is nothing to contract, so
// numpy float32 gives the same bytes (tests/frames_ref.py).  A uint8 source is copied and `scale` ignored.
//
// Launch rule.  A thread owns 4 consecutive pixels of a frame's flat index, i.e. the 12 output bytes [12 t, 12 t + 12), and stores them
// as up to three dwords (those that begin below pitch); a frame takes ceil(pitch / 12) threads, 256 a block, no block spans two frames.
// The entry admits N * blocks-per-frame up to 2^31 - 1 and serves all of them: past 2^24 - 1 blocks the launch goes out in slices, each
// with the flat index of its first block as the kernel's last argument (launch_sliced of launch.h) -- the rule of soft.h, for the
// reason stated there.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace fslic {

enum IngestType { kIngestU8 = 0, kIngestF16 = 1, kIngestBF16 = 2, kIngestF32 = 3 };
constexpr size_t kIngestMaxPitch = (size_t)1 << 33;

inline unsigned long long ingest_blocks_per_frame(size_t pitch) { return ((unsigned long long)(pitch + 11) / 12 + 255ull) / 256ull; }

void launch_pack_rgb(const void* src, int src_type, const long long strides[4], float scale, uint8_t* out, size_t pitch,
                     int N, int H, int W, hipStream_t st);

}  // namespace fslic
