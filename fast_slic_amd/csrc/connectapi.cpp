// connectapi.cpp -- the C ABI of the connectivity pass on label tensors (include/fslic_hip.h, fslic_hip_connect*; kernels in
// connect.hip), on streamapi.h; nothing here synchronises or copies to the host.
#include "connect.h"
#include "streamapi.h"

using namespace fslic;

namespace {

int check_connect_map(int N, int H, int W, int label_type) {
    if (N < 1) return fail(FSLIC_E_INVALID, "N must be positive");
    if (H < 1 || W < 1) return fail(FSLIC_E_INVALID, "H and W must be positive");
    if ((long long)H * W >= (1ll << 31) || (long long)N * ((long long)H * W) >= (1ll << 31)) return fail(FSLIC_E_INVALID, "N * H * W must be below 2^31");
    return check_label_type(label_type);
}

int run_connect(int device, void* stream, int N, int H, int W, const void* labels, int label_type, int32_t* out, int32_t* counts,
                void* workspace, size_t workspace_bytes, bool enforce, long long min_size) {
    int rc = check_device(device);
    if (rc || (rc = check_connect_map(N, H, W, label_type))) return rc;
    if (min_size < 0) return fail(FSLIC_E_INVALID, "min_size must be >= 0");
    if (!labels || !out || !counts || !workspace) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if ((rc = check_workspace(workspace_bytes, connect_workspace_bytes(N, H, W)))) return rc;
    const long long HW = (long long)H * W;
    return on_stream(device, stream, "connect launch", [&](hipStream_t st) -> int {
        launch_connect(labels, label_type, out, counts, workspace, N, H, W, enforce, (uint32_t)(min_size > HW ? HW + 1 : min_size), st);
        return FSLIC_OK;
    });
}

}  // namespace

extern "C" {

int fslic_hip_connect_workspace_size(int N, int H, int W, size_t* bytes) {
    return workspace_size(bytes, [&] { return check_connect_map(N, H, W, kLabelI32); }, [&] { return connect_workspace_bytes(N, H, W); });
}

int fslic_hip_connected_components(int device, void* stream, int N, int H, int W, const void* labels, int label_type,
                                   int32_t* components, int32_t* counts, void* workspace, size_t workspace_bytes) {
    return run_connect(device, stream, N, H, W, labels, label_type, components, counts, workspace, workspace_bytes, false, 0);
}

int fslic_hip_connect_enforce(int device, void* stream, int N, int H, int W, const void* labels, int label_type, long long min_size,
                              int32_t* out, int32_t* counts, void* workspace, size_t workspace_bytes) {
    return run_connect(device, stream, N, H, W, labels, label_type, out, counts, workspace, workspace_bytes, true, min_size);
}

}  // extern "C"
