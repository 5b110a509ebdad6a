// mergeapi.cpp -- the C ABI of merging on the region adjacency graph (include/fslic_hip.h, fslic_hip_merge*; kernels in merge.hip),
// on streamapi.h; nothing here synchronises or copies to the host.
#include "merge.h"
#include "streamapi.h"

using namespace fslic;

namespace {

int check_nodes(int device, int N, int K) {
    int rc = check_device(device);
    if (rc) return rc;
    if (N < 1) return fail(FSLIC_E_INVALID, "N must be positive");
    if ((rc = check_node_count(K, "K"))) return rc;
    if ((long long)N * K >= (1ll << 31)) return fail(FSLIC_E_INVALID, "N * K must be below 2^31");
    return FSLIC_OK;
}

// the edges of a graph: E of them, and with any the two arrays that say where they are
int check_edges(long long E, const void* edge_index, const void* offsets) {
    const int rc = check_entry_count(E, "E");
    if (rc) return rc;
    if (!offsets || (E > 0 && !edge_index)) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return FSLIC_OK;
}

}  // namespace

extern "C" {

int fslic_hip_merge_best_workspace_size(int N, int K, size_t* bytes) {
    return workspace_size(bytes, [&] { return check_nodes(0, N, K); }, [&] { return merge_best_workspace_bytes(N, K); });
}

int fslic_hip_merge_best_edges(int device, void* stream, int N, int K, long long E, const int64_t* edge_index, const int64_t* offsets,
                               const float* weight, int has_threshold, double threshold, uint8_t* join, void* workspace,
                               size_t workspace_bytes) {
    int rc = check_nodes(device, N, K);
    if (rc || (rc = check_edges(E, edge_index, offsets))) return rc;
    if (E > 0 && (!weight || !join)) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (!workspace) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const size_t need = merge_best_workspace_bytes(N, K);
    if ((rc = check_workspace(workspace_bytes, need))) return rc;
    if (E == 0) return FSLIC_OK;
    return on_stream(device, stream, "merge launch", [&](hipStream_t st) -> int {
        HIPCHK(hipMemsetAsync(workspace, 0xFF, need, st));
        launch_merge_best_edges(i64(edge_index), i64(offsets), weight, has_threshold == 0, threshold, join, workspace, N, K, E, st);
        return FSLIC_OK;
    });
}

int fslic_hip_merge_components_workspace_size(int N, int K, size_t* bytes) {
    return workspace_size(bytes, [&] { return check_nodes(0, N, K); }, [&] { return merge_components_workspace_bytes(N, K); });
}

int fslic_hip_merge_components(int device, void* stream, int N, int K, long long E, const int64_t* edge_index, const int64_t* offsets,
                               const uint8_t* join, const void* members, int members_type, int32_t* mapping, int32_t* counts,
                               void* workspace, size_t workspace_bytes) {
    int rc = check_nodes(device, N, K);
    if (rc || (rc = check_edges(E, edge_index, offsets))) return rc;
    if (E > 0 && !join) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (members && members_type != kLabelI32 && members_type != kLabelI64) return fail(FSLIC_E_INVALID, "members must be int32 or int64");
    if (!mapping || !counts || !workspace) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if ((rc = check_workspace(workspace_bytes, merge_components_workspace_bytes(N, K)))) return rc;
    return on_stream(device, stream, "merge launch", [&](hipStream_t st) -> int {
        launch_merge_components(i64(edge_index), i64(offsets), join, members, members ? members_type : kLabelI32, mapping, counts, workspace, N, K, E, st);
        return FSLIC_OK;
    });
}

int fslic_hip_merge_labels(int device, void* stream, int N, int H, int W, int K, const void* labels, int label_type,
                           const int32_t* mapping, int32_t* out) {
    int rc = check_nodes(device, N, K);
    if (rc) return rc;
    if (H < 1 || W < 1) return fail(FSLIC_E_INVALID, "H and W must be positive");
    if ((long long)H * W >= (1ll << 31) || (long long)N * ((long long)H * W) >= (1ll << 31)) return fail(FSLIC_E_INVALID, "N * H * W must be below 2^31");
    if ((rc = check_label_type(label_type))) return rc;
    if (!labels || !mapping || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (reinterpret_cast<uintptr_t>(out) & 3u) return fail(FSLIC_E_INVALID, "out must be 4-byte aligned");
    return on_stream(device, stream, "merge launch", [&](hipStream_t st) -> int {
        launch_merge_labels(labels, label_type, mapping, out, N, (long long)H * W, K, st);
        return FSLIC_OK;
    });
}

int fslic_hip_merge_contract_accumulate(int device, void* stream, int N, int K, int K2, long long E, const int64_t* edge_index,
                                        const int64_t* offsets, const int32_t* boundary, const int64_t* contrast, int C,
                                        const int32_t* mapping, long long capacity, void* workspace, size_t workspace_bytes) {
    int rc = check_nodes(device, N, K);
    if (rc || (rc = check_pair_table(device, N, capacity)) || (rc = check_edges(E, edge_index, offsets))) return rc;
    if ((rc = check_node_count(K2, "K2"))) return rc;
    if (C < 0 || C > kPairMaxChannels) return fail(FSLIC_E_INVALID, "C must be in [0, 4] (0: no contrast)");
    if ((contrast != nullptr) != (C > 0) && E > 0) return fail(FSLIC_E_INVALID, "contrast needs C in [1, 4], no contrast needs C == 0");
    if ((E > 0 && !boundary) || !mapping || !workspace) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const size_t need = pair_workspace_bytes(N, C, (uint32_t)capacity);
    if ((rc = check_workspace(workspace_bytes, need))) return rc;
    return on_stream(device, stream, "merge launch", [&](hipStream_t st) -> int {
        HIPCHK(hipMemsetAsync(workspace, 0, need, st));
        if (E > 0)
            launch_merge_contract(i64(edge_index), i64(offsets), boundary, i64(contrast), mapping, workspace, N, C, K, K2, E, (uint32_t)capacity, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
