// aggregateapi.cpp -- the C ABI of the aggregation over neighbour lists (include/fslic_hip.h, fslic_hip_aggregate*; kernels in
// aggregate.hip), on streamapi.h; nothing here synchronises, allocates or copies to the host.
#include "aggregate.h"
#include "streamapi.h"

using namespace fslic;

namespace {

// the device, the cells of a [N][C][K] array and the entries of the lists
int check_call(int device, int N, int C, int K, long long nnz) {
    int rc = check_device(device);
    if (rc || (rc = check_cells(N, C, K, "K"))) return rc;
    return check_entry_count(nnz, "nnz");
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
    return on_stream(device, stream, "aggregate launch", [&](hipStream_t st) -> int {
        launch_aggregate_forward(reduce, i64(offsets), indices, weight, values, out, argmax, degree, N, C, K, nnz, st);
        return FSLIC_OK;
    });
}

int fslic_hip_aggregate_backward_values(int device, void* stream, int N, int C, int K, long long nnz, int reduce, const int64_t* t_offsets,
                                        const int32_t* t_entries, const int32_t* t_rows, const float* weight, const int32_t* argmax,
                                        const int32_t* degree, const float* grad_out, float* grad_values) {
    int rc = check_call(device, N, C, K, nnz);
    if (rc || (rc = check_reduce(reduce, weight, argmax, degree))) return rc;
    if (!t_offsets || !grad_out || !grad_values || (nnz > 0 && (!t_entries || !t_rows))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "aggregate launch", [&](hipStream_t st) -> int {
        launch_aggregate_backward_values(reduce, i64(t_offsets), t_entries, t_rows, weight, argmax, degree, grad_out, grad_values, N, C, K, nnz, st);
        return FSLIC_OK;
    });
}

int fslic_hip_aggregate_backward_weight(int device, void* stream, int N, int C, int K, long long nnz, const int32_t* rows, const int32_t* indices,
                                        const float* values, const float* grad_out, float* grad_weight) {
    const int rc = check_call(device, N, C, K, nnz);
    if (rc) return rc;
    if (!values || !grad_out || (nnz > 0 && (!rows || !indices || !grad_weight))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (nnz == 0) return FSLIC_OK;
    return on_stream(device, stream, "aggregate launch", [&](hipStream_t st) -> int {
        launch_aggregate_backward_weight(rows, indices, values, grad_out, grad_weight, N, C, K, nnz, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
