// ingestapi.cpp -- the C ABI of the frame ingest (include/fslic_hip.h, fslic_hip_pack_rgb; kernel in ingest.hip), on streamapi.h.
#include "ingest.h"
#include "streamapi.h"

#include <cmath>

using namespace fslic;

extern "C" {

int fslic_hip_pack_rgb(int device, void* stream, int N, int H, int W, const void* src, int src_type, const long long strides[4],
                       float scale, uint8_t* out, size_t pitch) {
    const int rc = check_device(device);
    if (rc) return rc;
    if (!src || !strides || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (N < 1 || H < 1 || W < 1) return fail(FSLIC_E_INVALID, "N, H and W must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail(FSLIC_E_INVALID, "H * W must be below 2^31");
    if (src_type != kIngestU8 && src_type != kIngestF16 && src_type != kIngestBF16 && src_type != kIngestF32)
        return fail(FSLIC_E_INVALID, "unknown source type");
    if (pitch < (size_t)H * (size_t)W * 3 || (pitch & 15) != 0) return fail(FSLIC_E_INVALID, "pitch must be at least H * W * 3 and a multiple of 16");
    if (pitch > kIngestMaxPitch) return fail(FSLIC_E_INVALID, "pitch must be at most 2^33");
    if (!std::isfinite(scale)) return fail(FSLIC_E_INVALID, "scale must be finite");
    if (reinterpret_cast<uintptr_t>(out) & 3) return fail(FSLIC_E_INVALID, "out is not 4-byte aligned");
    const uintptr_t elem = src_type == kIngestU8 ? 1 : src_type == kIngestF32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(src) & (elem - 1)) return fail(FSLIC_E_INVALID, "src is not aligned to its element type");
    if ((unsigned long long)N * ingest_blocks_per_frame(pitch) >= (1ull << 31)) return fail(FSLIC_E_INVALID, "too many frames");
    return on_stream(device, stream, "pack launch", [&](hipStream_t st) -> int {
        launch_pack_rgb(src, src_type, strides, scale, out, pitch, N, H, W, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
