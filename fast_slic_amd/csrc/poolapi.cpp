// poolapi.cpp -- the C ABI of superpixel pooling (include/fslic_hip.h, fslic_hip_pool*; kernels in pool.hip), on streamapi.h.
#include "pool.h"
#include "streamapi.h"

using namespace fslic;

namespace {

int check_common(int device, int N, int C, int K, int reduce) {
    int rc = check_device(device);
    if (rc) return rc;
    if (N < 1 || C < 1) return fail(FSLIC_E_INVALID, "N and C must be positive");
    if ((rc = check_node_count(K, "K"))) return rc;
    if (reduce != kPoolSum && reduce != kPoolMean && reduce != kPoolMax) return fail(FSLIC_E_INVALID, "unknown reduce");
    if ((long long)N * C * K >= (1ll << 40)) return fail(FSLIC_E_INVALID, "N * C * K must be below 2^40");
    return FSLIC_OK;
}

}  // namespace

extern "C" {

int fslic_hip_pool_workspace_size(int N, int C, int K, int reduce, size_t* bytes) {
    return workspace_size(bytes, [&] { return check_common(0, N, C, K, reduce); }, [&] { return pool_workspace_bytes(N, C, K, reduce); });
}

int fslic_hip_pool(int device, void* stream, int N, int C, int H, int W, int K, int reduce, const float* features,
                   const void* labels, int label_type, void* workspace, size_t workspace_bytes) {
    int rc = check_common(device, N, C, K, reduce);
    if (rc || (rc = check_label_map(N, H, W, label_type))) return rc;
    if (!features || !labels || !workspace) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const size_t need = pool_workspace_bytes(N, C, K, reduce);
    if ((rc = check_workspace(workspace_bytes, need))) return rc;
    return on_stream(device, stream, "pool launch", [&](hipStream_t st) -> int {
        HIPCHK(hipMemsetAsync(workspace, 0, need, st));
        launch_pool_tiles(features, labels, label_type, reduce, workspace, N, C, H, W, K, st);
        return FSLIC_OK;
    });
}

int fslic_hip_pool_finalize(int device, void* stream, int N, int C, int K, int reduce, const void* workspace, size_t workspace_bytes,
                            float* values, int32_t* counts, int32_t* argmax) {
    const int rc = check_common(device, N, C, K, reduce);
    if (rc) return rc;
    if (!workspace || !values) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (argmax && reduce != kPoolMax) return fail(FSLIC_E_INVALID, "argmax needs reduce == FSLIC_POOL_MAX");
    if (workspace_bytes < pool_workspace_bytes(N, C, K, reduce)) return fail(FSLIC_E_INVALID, "workspace too small");
    return on_stream(device, stream, "pool launch", [&](hipStream_t st) -> int {
        launch_pool_finalize(workspace, reduce, values, counts, argmax, N, C, K, st);
        return FSLIC_OK;
    });
}

int fslic_hip_unpool(int device, void* stream, int N, int C, int H, int W, int K, const float* values, const void* labels,
                     int label_type, const int32_t* argmax, float fill, float* out) {
    int rc = check_common(device, N, C, K, kPoolSum);
    if (rc || (rc = check_label_map(N, H, W, label_type))) return rc;
    if (!values || !labels || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "pool launch", [&](hipStream_t st) -> int {
        launch_unpool(values, labels, label_type, argmax, fill, out, N, C, H, W, K, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
