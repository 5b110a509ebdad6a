// pixelapi.cpp -- the C ABI of the pixels over neighbour lists (include/fslic_hip.h, fslic_hip_pixel_*; kernels in pixel.hip), on
// streamapi.h; nothing here synchronises, allocates or copies to the host.
#include "pixel.h"
#include "streamapi.h"

using namespace fslic;

namespace {

// the device, the cells of a [N][C][K] array, the label map, the slots, the heads, the cells of the pixel-side arrays and the entries
int check_call(int device, int N, int C, int H, int W, int K, int S, int heads, long long nnz, int label_type) {
    int rc = check_device(device);
    if (rc || (rc = check_cells(N, C, K, "K")) || (rc = check_label_map(N, H, W, label_type))) return rc;
    if (S < 1 || S > kPixelMaxSlots) return fail(FSLIC_E_INVALID, "S must be in [1, 32]");
    if (heads < 1) return fail(FSLIC_E_INVALID, "heads must be positive");
    if (C % heads != 0) return fail(FSLIC_E_INVALID, "C must be a multiple of heads");
    const long long pixels = (long long)N * H * W;                     // N < 2^31 and H * W < 2^31
    if (pixels >= (1ll << 31) || pixels * C >= (1ll << 31)) return fail(FSLIC_E_INVALID, "N * C * H * W must be below 2^31");
    if (pixels * S >= (1ll << 31) || pixels * S * heads >= (1ll << 31)) return fail(FSLIC_E_INVALID, "N * heads * S * H * W must be below 2^31");
    return check_entry_count(nnz, "nnz");
}

PixelGeom geom(int N, int C, int H, int W, int K, int S, int heads, long long nnz, int label_type, const void* labels, const int64_t* offsets,
               const int32_t* indices) {
    return PixelGeom{N, C, H, W, K, S, heads, nnz, label_type, labels, i64(offsets), indices};
}

// the map and the lists: without entries the indices are not read
bool no_lists(const void* labels, const int64_t* offsets, const int32_t* indices, long long nnz) { return !labels || !offsets || (nnz > 0 && !indices); }

}  // namespace

extern "C" {

int fslic_hip_pixel_dot(int device, void* stream, int N, int C, int H, int W, int K, int S, int heads, long long nnz, int label_type,
                        const void* labels, const int64_t* offsets, const int32_t* indices, const float* a, const float* b, float* out) {
    const int rc = check_call(device, N, C, H, W, K, S, heads, nnz, label_type);
    if (rc) return rc;
    if (no_lists(labels, offsets, indices, nnz) || !a || !b || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "pixel launch", [&](hipStream_t st) -> int {
        launch_pixel_dot(geom(N, C, H, W, K, S, heads, nnz, label_type, labels, offsets, indices), a, b, out, st);
        return FSLIC_OK;
    });
}

int fslic_hip_pixel_mix(int device, void* stream, int N, int C, int H, int W, int K, int S, int heads, long long nnz, int label_type,
                        const void* labels, const int64_t* offsets, const int32_t* indices, const float* values, const float* weight, float* out) {
    const int rc = check_call(device, N, C, H, W, K, S, heads, nnz, label_type);
    if (rc) return rc;
    if (no_lists(labels, offsets, indices, nnz) || !values || !weight || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "pixel launch", [&](hipStream_t st) -> int {
        launch_pixel_mix(geom(N, C, H, W, K, S, heads, nnz, label_type, labels, offsets, indices), values, weight, out, st);
        return FSLIC_OK;
    });
}

int fslic_hip_pixel_softmax(int device, void* stream, int N, int C, int H, int W, int K, int S, int heads, long long nnz, int label_type,
                            const void* labels, const int64_t* offsets, const int32_t* indices, int backward, const float* in, const float* grad,
                            float* out) {
    const int rc = check_call(device, N, C, H, W, K, S, heads, nnz, label_type);
    if (rc) return rc;
    if (backward != 0 && backward != 1) return fail(FSLIC_E_INVALID, "backward must be 0 or 1");
    if (no_lists(labels, offsets, indices, nnz) || !in || !out || (backward && !grad)) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "pixel launch", [&](hipStream_t st) -> int {
        launch_pixel_softmax(geom(N, C, H, W, K, S, heads, nnz, label_type, labels, offsets, indices), in, backward ? grad : nullptr, out, st);
        return FSLIC_OK;
    });
}

int fslic_hip_pixel_scatter_workspace_size(int N, int C, int K, size_t* bytes) {
    return workspace_size(bytes, [&] { return check_cells(N, C, K, "K"); }, [&] { return pixel_scatter_workspace_bytes(N, C, K); });
}

int fslic_hip_pixel_scatter(int device, void* stream, int N, int C, int H, int W, int K, int S, int heads, long long nnz, int label_type,
                            const void* labels, const int64_t* offsets, const int32_t* indices, const float* x, const float* weight, float* out,
                            void* workspace, size_t workspace_bytes) {
    int rc = check_call(device, N, C, H, W, K, S, heads, nnz, label_type);
    if (rc) return rc;
    if (no_lists(labels, offsets, indices, nnz) || !x || !weight || !out || !workspace) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const size_t need = pixel_scatter_workspace_bytes(N, C, K);
    if ((rc = check_workspace(workspace_bytes, need))) return rc;
    return on_stream(device, stream, "pixel launch", [&](hipStream_t st) -> int {
        HIPCHK(hipMemsetAsync(workspace, 0, need, st));
        launch_pixel_scatter(geom(N, C, H, W, K, S, heads, nnz, label_type, labels, offsets, indices), x, weight, workspace, out, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
