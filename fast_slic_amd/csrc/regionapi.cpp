// regionapi.cpp -- the C ABI of the features of merged regions (include/fslic_hip.h, fslic_hip_region*; kernels in region.hip).
// No engine: the caller names the device and the stream and owns every buffer.  Every argument is checked before the first HIP call;
// nothing here synchronises or copies to the host.
#include "engine_internal.h"
#include "region.h"
#include "streamapi.h"

using namespace fslic;

namespace {

// the frames, the channels and the nodes (or groups) of a [N][C][K] array: what = "K" or "K2"
int check_cells(int N, int C, int K, const char* what) {
    if (N < 1) return fail(FSLIC_E_INVALID, "N must be positive");
    if (C < 1) return fail(FSLIC_E_INVALID, "C must be positive");
    if (K < 1 || K > 65534) return fail(FSLIC_E_INVALID, std::string(what) + " must be in [1, 65534]");
    if ((long long)N * K >= (1ll << 31) || (long long)N * K * C >= (1ll << 31))
        return fail(FSLIC_E_INVALID, std::string("N * C * ") + what + " must be below 2^31");
    return FSLIC_OK;
}

int check_counts_type(int counts_type) {
    if (counts_type != kLabelI32 && counts_type != kLabelI64) return fail(FSLIC_E_INVALID, "counts must be int32 or int64");
    return FSLIC_OK;
}

}  // namespace

extern "C" {

int fslic_hip_region_sums_workspace_size(int N, int C, int K2, size_t* bytes) {
    if (!bytes) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const int rc = check_cells(N, C, K2, "K2");
    if (rc) return rc;
    *bytes = region_sums_workspace_bytes(N, C, K2);
    return FSLIC_OK;
}

int fslic_hip_region_sums(int device, void* stream, int N, int C, int K, int K2, const float* values, const int32_t* mapping,
                          const void* counts, int counts_type, float* sums, void* counts_out, void* workspace, size_t workspace_bytes) {
    if (device < 0) return fail(FSLIC_E_INVALID, "device must be >= 0");
    int rc = check_cells(N, C, K, "K");
    if (rc || (rc = check_cells(N, C, K2, "K2"))) return rc;
    if (counts && (rc = check_counts_type(counts_type))) return rc;
    if ((counts != nullptr) != (counts_out != nullptr)) return fail(FSLIC_E_INVALID, "counts and counts_out go together");
    if (!values || !mapping || !sums || !workspace) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const size_t need = region_sums_workspace_bytes(N, C, K2);
    if (workspace_bytes < need) return fail(FSLIC_E_INVALID, "workspace too small: " + std::to_string(need) + " bytes needed");
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(hipMemsetAsync(workspace, 0, need, st));
    if (counts_out) HIPCHK(hipMemsetAsync(counts_out, 0, (size_t)N * (size_t)K2 * (counts_type == kLabelI64 ? 8 : 4), st));
    launch_region_sums(values, mapping, counts, counts_type, sums, counts_out, workspace, N, C, K, K2, st);
    return launched("region launch");
}

int fslic_hip_region_edge_weights(int device, void* stream, int N, int C, int K, long long E, const int64_t* edge_index, const int64_t* offsets,
                                  const float* sums, const void* counts, int counts_type, int mode, float* weight) {
    if (device < 0) return fail(FSLIC_E_INVALID, "device must be >= 0");
    int rc = check_cells(N, C, K, "K");
    if (rc || (rc = check_counts_type(counts_type))) return rc;
    if (E < 0 || E >= (1ll << 31)) return fail(FSLIC_E_INVALID, "E must be in [0, 2^31)");
    if (mode != kRegionMean && mode != kRegionWard) return fail(FSLIC_E_INVALID, "mode must be 0 (mean) or 1 (ward)");
    if (!offsets || !sums || !counts || (E > 0 && (!edge_index || !weight))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (E == 0) return FSLIC_OK;
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    launch_region_edge_weights(reinterpret_cast<const long long*>(edge_index), reinterpret_cast<const long long*>(offsets), sums, counts, counts_type,
                               mode, weight, N, C, K, E, reinterpret_cast<hipStream_t>(stream));
    return launched("region launch");
}

}  // extern "C"
