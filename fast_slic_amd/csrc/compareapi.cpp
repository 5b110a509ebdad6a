// compareapi.cpp -- the C ABI of the comparison of two label maps (include/fslic_hip.h, fslic_hip_overlap*, fslic_hip_boundary_match;
// kernels in compare.hip).  No engine: the caller names the device and the stream and owns every buffer.  Every argument is checked
// before the first HIP call.
#include "engine_internal.h"
#include "compare.h"
#include "streamapi.h"

using namespace fslic;

namespace {

int check_tables(int device, int N, long long capacity) {
    if (device < 0) return fail(FSLIC_E_INVALID, "device must be >= 0");
    if (N < 1) return fail(FSLIC_E_INVALID, "N must be positive");
    if (capacity < (long long)kOverlapMinCapacity || capacity > (long long)kOverlapMaxCapacity || (capacity & (capacity - 1)) != 0)
        return fail(FSLIC_E_INVALID, "capacity must be a power of two in [64, 2^31]");
    if ((long long)N * capacity >= (1ll << 40)) return fail(FSLIC_E_INVALID, "N * capacity must be below 2^40");
    return FSLIC_OK;
}

int check_label_type(int label_type) {
    if (label_type != kLabelU16 && label_type != kLabelI32 && label_type != kLabelI64) return fail(FSLIC_E_INVALID, "unknown label type");
    return FSLIC_OK;
}

int launched() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FSLIC_OK : fail(FSLIC_E_HIP, std::string("compare launch: ") + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int fslic_hip_overlap_workspace_size(int N, long long capacity, size_t* bytes) {
    if (!bytes) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const int rc = check_tables(0, N, capacity);
    if (rc) return rc;
    *bytes = overlap_workspace_bytes(N, (uint32_t)capacity);
    return FSLIC_OK;
}

int fslic_hip_overlap_accumulate(int device, void* stream, int N, int H, int W, int K, int M, const void* labels, int label_type,
                                 const void* other, int other_type, long long capacity, void* workspace, size_t workspace_bytes) {
    int rc = check_tables(device, N, capacity);
    if (rc || (rc = check_label_map(N, H, W, label_type)) || (rc = check_label_type(other_type))) return rc;
    if (K < 1 || K > 65534) return fail(FSLIC_E_INVALID, "K must be in [1, 65534]");
    if (M < 1 || M > 65534) return fail(FSLIC_E_INVALID, "M must be in [1, 65534]");
    if (!labels || !other || !workspace) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const size_t need = overlap_workspace_bytes(N, (uint32_t)capacity);
    if (workspace_bytes < need) return fail(FSLIC_E_INVALID, "workspace too small: " + std::to_string(need) + " bytes needed");
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(hipMemsetAsync(workspace, 0, need, st));
    launch_overlap_accumulate(labels, label_type, other, other_type, workspace, N, H, W, K, M, (uint32_t)capacity, st);
    return launched();
}

int fslic_hip_overlap_compact(int device, void* stream, int N, long long capacity, void* workspace, size_t workspace_bytes,
                              int64_t* keys, int32_t* count, long long max_pairs) {
    int rc = check_tables(device, N, capacity);
    if (rc) return rc;
    if (!workspace || !keys || !count) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (max_pairs < 0) return fail(FSLIC_E_INVALID, "max_pairs must be >= 0");
    if (workspace_bytes < overlap_workspace_bytes(N, (uint32_t)capacity)) return fail(FSLIC_E_INVALID, "workspace too small");
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(hipMemsetAsync(reinterpret_cast<char*>(workspace) + offsetof(RagHeader, cursor), 0, sizeof(unsigned long long), st));
    launch_overlap_compact(workspace, N, (uint32_t)capacity, reinterpret_cast<unsigned long long*>(keys), count,
                           (unsigned long long)max_pairs, st);
    return launched();
}

int fslic_hip_boundary_match(int device, void* stream, int N, int H, int W, const void* labels, int label_type,
                             const void* other, int other_type, int tolerance, int64_t* counts) {
    if (device < 0) return fail(FSLIC_E_INVALID, "device must be >= 0");
    if (N < 1) return fail(FSLIC_E_INVALID, "N must be positive");
    int rc = check_label_map(N, H, W, label_type);
    if (rc || (rc = check_label_type(other_type))) return rc;
    if (tolerance < 0 || tolerance > kMatchMaxTolerance) return fail(FSLIC_E_INVALID, "tolerance must be in [0, 15]");
    if (!labels || !other || !counts) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)N * 3 * sizeof(int64_t), st));
    launch_boundary_match(labels, label_type, other, other_type, reinterpret_cast<unsigned long long*>(counts), N, H, W, tolerance, st);
    return launched();
}

}  // extern "C"
