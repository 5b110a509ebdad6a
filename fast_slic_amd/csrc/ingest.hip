// ingest.hip -- k_pack_rgb: N frames of 3 channels in any torch layout -> the engine's uint8 [H][W][3] frames, one pass, gfx950
// (fast_slic_amd/frames.py; ingest.h has the layouts, the arithmetic and the launch rule).
// A streaming kernel: 3 - 12 bytes read and 3 written per pixel.  A thread owns 4 consecutive pixels of the frame's flat index and
// stores their 12 bytes as three dwords, so a wavefront writes 768 consecutive bytes.
//   PLANAR  (column stride 1, row stride W): the 4 pixels are 4 consecutive elements of each channel's plane.  They come in ONE load of
//           4 * sizeof(T) bytes (16 for float32) where the plane's own start has that alignment -- decided per (frame, channel) from the
//           address: with H * W odd every other plane of a contiguous tensor is off by one element -- and in 4 coalesced element loads
//           otherwise, and in the thread that holds a plane's last 1 - 3 pixels.
//   generic (any other strides: channel-last, crops, channels_last): (y, x) of the thread's first pixel by one division, then stepped.
// Both read exactly the elements of pixels below H * W and give the same bytes.  No atomics, no LDS, no dependence on the launch shape.
#include "device_common.h"
#include "ingest.h"

namespace fslic {

template <int TYPE> struct IngestElem { using T = uint16_t; };      // float16 and bfloat16 travel as their 16 bits
template <> struct IngestElem<kIngestU8> { using T = uint8_t; };
template <> struct IngestElem<kIngestF32> { using T = float; };

template <class T> struct alignas(4 * sizeof(T)) Quad { T v[4]; };

// ingest.h: v = x * scale (one rounding), NaN -> 0, clamp to [0, 255], round to nearest even
template <int TYPE> static __device__ __forceinline__ uint32_t to_byte(typename IngestElem<TYPE>::T e, float scale) {
    if constexpr (TYPE == kIngestU8) {
        return (uint32_t)e;
    } else {
        float x;
        if constexpr (TYPE == kIngestF16) x = (float)__builtin_bit_cast(_Float16, e);
        else if constexpr (TYPE == kIngestBF16) x = __uint_as_float((uint32_t)e << 16);
        else x = e;
        float v = x * scale;
        v = v != v ? 0.0f : v;
        v = fminf(fmaxf(v, 0.0f), 255.0f);
        return (uint32_t)__builtin_rintf(v);
    }
}

// `first`: the flat block index of the launch's block 0 (launch_sliced)
template <int TYPE, bool PLANAR>
__global__ __launch_bounds__(256) void k_pack_rgb(const typename IngestElem<TYPE>::T* __restrict__ src, long long sf, long long sc, long long sr,
                                                  long long sw, float scale, uint8_t* __restrict__ out, unsigned long long pitch, uint32_t HW,
                                                  uint32_t W, uint32_t bpf, uint32_t first) {
    using T = typename IngestElem<TYPE>::T;
    const uint32_t blk = first + blockIdx.x, n = blk / bpf, t = (blk - n * bpf) * 256u + threadIdx.x;
    const unsigned long long byte0 = 12ull * t;
    if (byte0 >= pitch) return;
    const unsigned long long p0 = 4ull * t;             // the thread's first pixel; at or past HW: padding only
    const bool whole = p0 + 3ull < (unsigned long long)HW;
    const T* __restrict__ frame = src + (long long)n * sf;
    uint32_t y0 = 0, x0 = 0;
    if constexpr (!PLANAR) {
        if (p0 < HW) { y0 = (uint32_t)p0 / W; x0 = (uint32_t)p0 - y0 * W; }
    }
    uint32_t b[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T* __restrict__ plane = frame + (long long)c * sc;
        if constexpr (PLANAR) {
            if (whole && (reinterpret_cast<uintptr_t>(plane) & (4 * sizeof(T) - 1)) == 0) {
                const Quad<T> q = *reinterpret_cast<const Quad<T>*>(plane + p0);
#pragma unroll
                for (int j = 0; j < 4; ++j) b[c][j] = to_byte<TYPE>(q.v[j], scale);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) b[c][j] = p0 + j < HW ? to_byte<TYPE>(plane[p0 + j], scale) : 0u;
            }
        } else {
            uint32_t y = y0, x = x0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                b[c][j] = p0 + j < HW ? to_byte<TYPE>(plane[(long long)y * sr + (long long)x * sw], scale) : 0u;
                if (++x == W) { x = 0; ++y; }
            }
        }
    }
    // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3; pitch and byte0 are multiples of 4, so a dword that begins below pitch ends there too
    uint32_t* __restrict__ o = reinterpret_cast<uint32_t*>(out + (unsigned long long)n * pitch + byte0);
    const uint32_t w0 = b[0][0] | b[1][0] << 8 | b[2][0] << 16 | b[0][1] << 24;
    const uint32_t w1 = b[1][1] | b[2][1] << 8 | b[0][2] << 16 | b[1][2] << 24;
    const uint32_t w2 = b[2][2] | b[0][3] << 8 | b[1][3] << 16 | b[2][3] << 24;
    if (byte0 + 12ull <= pitch) {            // every thread of a frame but its last: 12 bytes back to back
        o[0] = w0; o[1] = w1; o[2] = w2;
    } else {                                 // pitch - byte0 is 4 or 8
        o[0] = w0;
        if (byte0 + 4ull < pitch) o[1] = w1;
    }
}

// ---- launch (the entry of ingestapi.cpp has checked every argument: N * blocks-per-frame is below 2^31, out is 4-byte aligned) ----
template <int TYPE>
static void launch_pack_type(const void* src, const long long s[4], float scale, uint8_t* out, size_t pitch, int N, int H, int W, hipStream_t st) {
    using T = typename IngestElem<TYPE>::T;
    const uint32_t HW = (uint32_t)H * (uint32_t)W, bpf = (uint32_t)ingest_blocks_per_frame(pitch);
    const unsigned long long blocks = (unsigned long long)bpf * (unsigned long long)N;
    const bool planar = (s[3] == 1 || W == 1) && (s[2] == (long long)W || H == 1);
    const T* p = reinterpret_cast<const T*>(src);
    if (planar) launch_sliced(k_pack_rgb<TYPE, true>, blocks, st, p, s[0], s[1], s[2], s[3], scale, out, (unsigned long long)pitch, HW, (uint32_t)W, bpf);
    else launch_sliced(k_pack_rgb<TYPE, false>, blocks, st, p, s[0], s[1], s[2], s[3], scale, out, (unsigned long long)pitch, HW, (uint32_t)W, bpf);
}

void launch_pack_rgb(const void* src, int src_type, const long long strides[4], float scale, uint8_t* out, size_t pitch,
                     int N, int H, int W, hipStream_t st) {
    if (src_type == kIngestU8) launch_pack_type<kIngestU8>(src, strides, scale, out, pitch, N, H, W, st);
    else if (src_type == kIngestF16) launch_pack_type<kIngestF16>(src, strides, scale, out, pitch, N, H, W, st);
    else if (src_type == kIngestBF16) launch_pack_type<kIngestBF16>(src, strides, scale, out, pitch, N, H, W, st);
    else launch_pack_type<kIngestF32>(src, strides, scale, out, pitch, N, H, W, st);
}

}  // namespace fslic
