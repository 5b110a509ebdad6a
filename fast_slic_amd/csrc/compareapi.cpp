// compareapi.cpp -- the C ABI of the comparison of two label maps (include/fslic_hip.h, fslic_hip_overlap*, fslic_hip_boundary_match;
// kernels in compare.hip), on streamapi.h.
#include "compare.h"
#include "streamapi.h"

using namespace fslic;

extern "C" {

int fslic_hip_overlap_workspace_size(int N, long long capacity, size_t* bytes) {
    return workspace_size(bytes, [&] { return check_pair_table(0, N, capacity); }, [&] { return pair_workspace_bytes(N, 0, (uint32_t)capacity); });
}

int fslic_hip_overlap_accumulate(int device, void* stream, int N, int H, int W, int K, int M, const void* labels, int label_type,
                                 const void* other, int other_type, long long capacity, void* workspace, size_t workspace_bytes) {
    int rc = check_pair_table(device, N, capacity);
    if (rc || (rc = check_label_map(N, H, W, label_type)) || (rc = check_label_type(other_type))) return rc;
    if ((rc = check_node_count(K, "K")) || (rc = check_node_count(M, "M"))) return rc;
    if (!labels || !other || !workspace) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const size_t need = pair_workspace_bytes(N, 0, (uint32_t)capacity);
    if ((rc = check_workspace(workspace_bytes, need))) return rc;
    return on_stream(device, stream, "compare launch", [&](hipStream_t st) -> int {
        HIPCHK(hipMemsetAsync(workspace, 0, need, st));
        launch_overlap_accumulate(labels, label_type, other, other_type, workspace, N, H, W, K, M, (uint32_t)capacity, st);
        return FSLIC_OK;
    });
}

int fslic_hip_overlap_compact(int device, void* stream, int N, long long capacity, void* workspace, size_t workspace_bytes,
                              int64_t* keys, int32_t* count, long long max_pairs) {
    const int rc = check_pair_table(device, N, capacity);
    if (rc) return rc;
    if (!workspace || !keys || !count) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (max_pairs < 0) return fail(FSLIC_E_INVALID, "max_pairs must be >= 0");
    if (workspace_bytes < pair_workspace_bytes(N, 0, (uint32_t)capacity)) return fail(FSLIC_E_INVALID, "workspace too small");
    return on_stream(device, stream, "compare launch", [&](hipStream_t st) -> int {
        HIPCHK(hipMemsetAsync(reinterpret_cast<char*>(workspace) + offsetof(PairHeader, cursor), 0, sizeof(unsigned long long), st));
        launch_pair_compact(workspace, N, 0, (uint32_t)capacity, 1u, false, u64(keys), count, nullptr, (unsigned long long)max_pairs, st);
        return FSLIC_OK;
    });
}

int fslic_hip_boundary_match(int device, void* stream, int N, int H, int W, const void* labels, int label_type,
                             const void* other, int other_type, int tolerance, int64_t* counts) {
    int rc = check_device(device);
    if (rc) return rc;
    if (N < 1) return fail(FSLIC_E_INVALID, "N must be positive");
    if ((rc = check_label_map(N, H, W, label_type)) || (rc = check_label_type(other_type))) return rc;
    if (tolerance < 0 || tolerance > kMatchMaxTolerance) return fail(FSLIC_E_INVALID, "tolerance must be in [0, 15]");
    if (!labels || !other || !counts) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "compare launch", [&](hipStream_t st) -> int {
        HIPCHK(hipMemsetAsync(counts, 0, (size_t)N * 3 * sizeof(int64_t), st));
        launch_boundary_match(labels, label_type, other, other_type, u64(counts), N, H, W, tolerance, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
