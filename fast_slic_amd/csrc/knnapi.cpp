// knnapi.cpp -- the C ABI of the nearest neighbours in feature space (include/fslic_hip.h, fslic_hip_knn_graph; kernel in knn.hip), on
// streamapi.h; nothing here synchronises, allocates or copies to the host.
#include "knn.h"
#include "streamapi.h"

using namespace fslic;

extern "C" {

int fslic_hip_knn_graph(int device, void* stream, int N, int D, int K, int k, int loop, const float* points, const float* other,
                        const uint8_t* valid, int32_t* indices, float* dist) {
    int rc = check_device(device);
    if (rc || (rc = check_cells(N, D, K, "K"))) return rc;
    if (k < 1 || k > kKnnMaxK) return fail(FSLIC_E_INVALID, "k must be in [1, 32]");
    if ((long long)N * K * k >= (1ll << 31)) return fail(FSLIC_E_INVALID, "N * K * k must be below 2^31");
    if (loop && other) return fail(FSLIC_E_INVALID, "loop goes with points alone, not with other");
    if (!points || !indices || !dist) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "knn launch", [&](hipStream_t st) -> int {
        launch_knn_graph(points, other, valid, indices, dist, N, D, K, k, loop != 0, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
