// aggregateapi.cpp -- the C ABI of the aggregation over neighbour lists (include/fslic_hip.h, fslic_hip_aggregate*; kernels in
// aggregate.hip).  No engine: the caller names the device and the stream and owns every buffer.  Every argument is checked before the
// first HIP call; nothing here synchronises, allocates or copies to the host.
#include "engine_internal.h"
#include "aggregate.h"
#include "streamapi.h"

using namespace fslic;

namespace {

// the device, the cells of a [N][C][K] array and the entries of the lists
int check_call(int device, int N, int C, int K, long long nnz) {
    if (device < 0) return fail(FSLIC_E_INVALID, "device must be >= 0");
    if (N < 1) return fail(FSLIC_E_INVALID, "N must be positive");
    if (C < 1) return fail(FSLIC_E_INVALID, "C must be positive");
    if (K < 1 || K > 65534) return fail(FSLIC_E_INVALID, "K must be in [1, 65534]");
    if ((long long)N * K >= (1ll << 31) || (long long)N * K * C >= (1ll << 31)) return fail(FSLIC_E_INVALID, "N * C * K must be below 2^31");
    if (nnz < 0 || nnz >= (1ll << 31)) return fail(FSLIC_E_INVALID, "nnz must be in [0, 2^31)");
    return FSLIC_OK;
}

// the reduction and what goes with it: a weight only with the sum, the argmax with the max, the degree with the mean
int check_reduce(int reduce, const void* weight, const void* argmax, const void* degree) {
    if (reduce != kAggSum && reduce != kAggMean && reduce != kAggMax) return fail(FSLIC_E_INVALID, "reduce must be 0 (sum), 1 (mean) or 2 (max)");
    if (weight && reduce != kAggSum) return fail(FSLIC_E_INVALID, "a weight goes with reduce 0 (sum) only");
    if (reduce == kAggMax && !argmax) return fail(FSLIC_E_INVALID, "reduce 2 (max) needs argmax");
    if (reduce == kAggMean && !degree) return fail(FSLIC_E_INVALID, "reduce 1 (mean) needs degree");
    return FSLIC_OK;
}

}  // namespace

extern "C" {

int fslic_hip_aggregate_forward(int device, void* stream, int N, int C, int K, long long nnz, int reduce, const int64_t* offsets,
                                const int32_t* indices, const float* weight, const float* values, float* out, int32_t* argmax, int32_t* degree) {
    int rc = check_call(device, N, C, K, nnz);
    if (rc || (rc = check_reduce(reduce, weight, argmax, degree))) return rc;
    if (!offsets || !values || !out || (nnz > 0 && !indices)) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    launch_aggregate_forward(reduce, reinterpret_cast<const long long*>(offsets), indices, weight, values, out, argmax, degree, N, C, K, nnz,
                             reinterpret_cast<hipStream_t>(stream));
    return launched("aggregate launch");
}

int fslic_hip_aggregate_backward_values(int device, void* stream, int N, int C, int K, long long nnz, int reduce, const int64_t* t_offsets,
                                        const int32_t* t_entries, const int32_t* t_rows, const float* weight, const int32_t* argmax,
                                        const int32_t* degree, const float* grad_out, float* grad_values) {
    int rc = check_call(device, N, C, K, nnz);
    if (rc || (rc = check_reduce(reduce, weight, argmax, degree))) return rc;
    if (!t_offsets || !grad_out || !grad_values || (nnz > 0 && (!t_entries || !t_rows))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    launch_aggregate_backward_values(reduce, reinterpret_cast<const long long*>(t_offsets), t_entries, t_rows, weight, argmax, degree, grad_out,
                                     grad_values, N, C, K, nnz, reinterpret_cast<hipStream_t>(stream));
    return launched("aggregate launch");
}

int fslic_hip_aggregate_backward_weight(int device, void* stream, int N, int C, int K, long long nnz, const int32_t* rows, const int32_t* indices,
                                        const float* values, const float* grad_out, float* grad_weight) {
    int rc = check_call(device, N, C, K, nnz);
    if (rc) return rc;
    if (!values || !grad_out || (nnz > 0 && (!rows || !indices || !grad_weight))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (nnz == 0) return FSLIC_OK;
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    launch_aggregate_backward_weight(rows, indices, values, grad_out, grad_weight, N, C, K, nnz, reinterpret_cast<hipStream_t>(stream));
    return launched("aggregate launch");
}

}  // extern "C"
