// regionapi.cpp -- the C ABI of the features of merged regions (include/fslic_hip.h, fslic_hip_region*; kernels in region.hip),
// on streamapi.h; nothing here synchronises or copies to the host.
#include "region.h"
#include "streamapi.h"

using namespace fslic;

namespace {

int check_counts_type(int counts_type) {
    if (counts_type != kLabelI32 && counts_type != kLabelI64) return fail(FSLIC_E_INVALID, "counts must be int32 or int64");
    return FSLIC_OK;
}

}  // namespace

extern "C" {

int fslic_hip_region_sums_workspace_size(int N, int C, int K2, size_t* bytes) {
    return workspace_size(bytes, [&] { return check_cells(N, C, K2, "K2"); }, [&] { return region_sums_workspace_bytes(N, C, K2); });
}

int fslic_hip_region_sums(int device, void* stream, int N, int C, int K, int K2, const float* values, const int32_t* mapping,
                          const void* counts, int counts_type, float* sums, void* counts_out, void* workspace, size_t workspace_bytes) {
    int rc = check_device(device);
    if (rc || (rc = check_cells(N, C, K, "K")) || (rc = check_cells(N, C, K2, "K2"))) return rc;
    if (counts && (rc = check_counts_type(counts_type))) return rc;
    if ((counts != nullptr) != (counts_out != nullptr)) return fail(FSLIC_E_INVALID, "counts and counts_out go together");
    if (!values || !mapping || !sums || !workspace) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const size_t need = region_sums_workspace_bytes(N, C, K2);
    if ((rc = check_workspace(workspace_bytes, need))) return rc;
    return on_stream(device, stream, "region launch", [&](hipStream_t st) -> int {
        HIPCHK(hipMemsetAsync(workspace, 0, need, st));
        if (counts_out) HIPCHK(hipMemsetAsync(counts_out, 0, (size_t)N * (size_t)K2 * (counts_type == kLabelI64 ? 8 : 4), st));
        launch_region_sums(values, mapping, counts, counts_type, sums, counts_out, workspace, N, C, K, K2, st);
        return FSLIC_OK;
    });
}

int fslic_hip_region_edge_weights(int device, void* stream, int N, int C, int K, long long E, const int64_t* edge_index, const int64_t* offsets,
                                  const float* sums, const void* counts, int counts_type, int mode, float* weight) {
    int rc = check_device(device);
    if (rc || (rc = check_cells(N, C, K, "K")) || (rc = check_counts_type(counts_type)) || (rc = check_entry_count(E, "E"))) return rc;
    if (mode != kRegionMean && mode != kRegionWard) return fail(FSLIC_E_INVALID, "mode must be 0 (mean) or 1 (ward)");
    if (!offsets || !sums || !counts || (E > 0 && (!edge_index || !weight))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (E == 0) return FSLIC_OK;
    return on_stream(device, stream, "region launch", [&](hipStream_t st) -> int {
        launch_region_edge_weights(i64(edge_index), i64(offsets), sums, counts, counts_type, mode, weight, N, C, K, E, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
