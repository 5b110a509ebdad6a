// ragapi.cpp -- the C ABI of the region adjacency graph (include/fslic_hip.h, fslic_hip_rag*; kernels in rag.hip), on streamapi.h.
#include "rag.h"
#include "streamapi.h"

using namespace fslic;

namespace {

int check_tables(int device, int N, int K, int C, long long capacity) {
    int rc = check_pair_table(device, N, capacity);
    if (rc || (rc = check_node_count(K, "K"))) return rc;
    if (C < 0 || C > kPairMaxChannels) return fail(FSLIC_E_INVALID, "C must be in [0, 4] (0: no image)");
    return FSLIC_OK;
}

}  // namespace

extern "C" {

int fslic_hip_rag_workspace_size(int N, int K, int C, long long capacity, size_t* bytes) {
    return workspace_size(bytes, [&] { return check_tables(0, N, K, C, capacity); }, [&] { return pair_workspace_bytes(N, C, (uint32_t)capacity); });
}

int fslic_hip_rag_accumulate(int device, void* stream, int N, int H, int W, int K, int connectivity, const void* labels, int label_type,
                             const uint8_t* image, int C, long long capacity, void* workspace, size_t workspace_bytes) {
    int rc = check_tables(device, N, K, C, capacity);
    if (rc || (rc = check_label_map(N, H, W, label_type))) return rc;
    if ((long long)H * W >= (1ll << 29)) return fail(FSLIC_E_INVALID, "H * W must be below 2^29");      // 4 pairs a pixel in an int32 count
    if (connectivity != 4 && connectivity != 8) return fail(FSLIC_E_INVALID, "connectivity must be 4 or 8");
    if (!labels || !workspace) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if ((image != nullptr) != (C > 0)) return fail(FSLIC_E_INVALID, "an image needs C in [1, 4], no image needs C == 0");
    const size_t need = pair_workspace_bytes(N, C, (uint32_t)capacity);
    if ((rc = check_workspace(workspace_bytes, need))) return rc;
    return on_stream(device, stream, "rag launch", [&](hipStream_t st) -> int {
        HIPCHK(hipMemsetAsync(workspace, 0, need, st));
        launch_rag_accumulate(labels, label_type, image, workspace, N, C, H, W, K, connectivity, (uint32_t)capacity, st);
        return FSLIC_OK;
    });
}

int fslic_hip_rag_compact(int device, void* stream, int N, int C, long long capacity, void* workspace, size_t workspace_bytes,
                          int64_t* keys, int32_t* boundary, int64_t* contrast, long long max_edges) {
    const int rc = check_tables(device, N, 1, C, capacity);
    if (rc) return rc;
    if (!workspace || !keys || !boundary) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (contrast && C == 0) return fail(FSLIC_E_INVALID, "contrast needs C in [1, 4]");
    if (max_edges < 0) return fail(FSLIC_E_INVALID, "max_edges must be >= 0");
    if (workspace_bytes < pair_workspace_bytes(N, C, (uint32_t)capacity)) return fail(FSLIC_E_INVALID, "workspace too small");
    return on_stream(device, stream, "rag launch", [&](hipStream_t st) -> int {
        HIPCHK(hipMemsetAsync(reinterpret_cast<char*>(workspace) + offsetof(PairHeader, cursor), 0, sizeof(unsigned long long), st));
        launch_pair_compact(workspace, N, C, (uint32_t)capacity, 0u, true, u64(keys), boundary, u64(contrast), (unsigned long long)max_edges, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
