// softapi.cpp -- the C ABI of soft superpixel assignment (include/fslic_hip.h, fslic_hip_soft_*; kernels in soft.hip), on streamapi.h.
#include "soft.h"
#include "streamapi.h"

using namespace fslic;

namespace {

// The two block counts are admitted up to 2^31 - 1 and all of them are served: soft.hip issues a launch in slices the runtime
// supports (soft.h, the launch rule).
int check_soft(int device, int N, int C, int H, int W, int gh, int gw) {
    const int rc = check_device(device);
    if (rc) return rc;
    if (N < 1 || C < 1) return fail(FSLIC_E_INVALID, "N and C must be positive");
    if (H < 1 || W < 1) return fail(FSLIC_E_INVALID, "H and W must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail(FSLIC_E_INVALID, "H * W must be below 2^31");
    if (gh < 1 || gh > H || gw < 1 || gw > W) return fail(FSLIC_E_INVALID, "the grid must be 1 <= gh <= H and 1 <= gw <= W");
    if ((long long)gh * gw > kSoftMaxK) return fail(FSLIC_E_INVALID, "gh * gw must be at most 65534");
    if ((long long)N * (((long long)H * W + 255) / 256) >= (1ll << 31)) return fail(FSLIC_E_INVALID, "too many frames");
    if (soft_pool_items(N, C, gh * gw) >= (1ull << 31)) return fail(FSLIC_E_INVALID, "N * gh * gw * ceil(C / 16) must be below 2^31");
    return FSLIC_OK;
}

}  // namespace

extern "C" {

int fslic_hip_soft_assign(int device, void* stream, int N, int C, int H, int W, int gh, int gw, const float* features,
                          const float* centres, float* q) {
    const int rc = check_soft(device, N, C, H, W, gh, gw);
    if (rc) return rc;
    if (!features || !centres || !q) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "soft launch", [&](hipStream_t st) -> int {
        launch_soft_assign(features, centres, q, N, C, H, W, gh, gw, st);
        return FSLIC_OK;
    });
}

int fslic_hip_soft_assign_backward(int device, void* stream, int N, int C, int H, int W, int gh, int gw, const float* features,
                                   const float* centres, const float* q, const float* grad_q, float* grad_d, float* grad_features) {
    const int rc = check_soft(device, N, C, H, W, gh, gw);
    if (rc) return rc;
    if (!features || !centres || !q || !grad_q || !grad_d || !grad_features) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "soft launch", [&](hipStream_t st) -> int {
        launch_soft_assign_bwd(features, centres, q, grad_q, grad_d, grad_features, N, C, H, W, gh, gw, st);
        return FSLIC_OK;
    });
}

int fslic_hip_soft_pool(int device, void* stream, int N, int C, int H, int W, int gh, int gw, const float* features, const float* q,
                        const float* centres, float* sums, float* weights) {
    const int rc = check_soft(device, N, C, H, W, gh, gw);
    if (rc) return rc;
    if (!features || !q || !sums) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "soft launch", [&](hipStream_t st) -> int {
        launch_soft_pool(features, q, centres, sums, weights, N, C, H, W, gh, gw, st);
        return FSLIC_OK;
    });
}

int fslic_hip_soft_unpool(int device, void* stream, int N, int C, int H, int W, int gh, int gw, const float* values, const float* q,
                          float* out) {
    const int rc = check_soft(device, N, C, H, W, gh, gw);
    if (rc) return rc;
    if (!values || !q || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "soft launch", [&](hipStream_t st) -> int {
        launch_soft_unpool(values, q, out, N, C, H, W, gh, gw, st);
        return FSLIC_OK;
    });
}

int fslic_hip_soft_dot(int device, void* stream, int N, int C, int H, int W, int gh, int gw, const float* a, const float* b,
                       const float* bias, float* out) {
    const int rc = check_soft(device, N, C, H, W, gh, gw);
    if (rc) return rc;
    if (!a || !b || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "soft launch", [&](hipStream_t st) -> int {
        launch_soft_dot(a, b, bias, out, N, C, H, W, gh, gw, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
