// messageapi.cpp -- the C ABI of the messages over neighbour lists (include/fslic_hip.h, fslic_hip_message_*; kernels in
// message.hip), on streamapi.h; nothing here synchronises, allocates or copies to the host.
#include "message.h"
#include "streamapi.h"

using namespace fslic;

namespace {

// the device, the cells of a [N][C][K] array, the entries of the lists and the cells of a [C][nnz] array
int check_call(int device, int N, int C, int K, long long nnz) {
    int rc = check_device(device);
    if (rc || (rc = check_cells(N, C, K, "K")) || (rc = check_entry_count(nnz, "nnz"))) return rc;
    if ((long long)C * nnz >= (1ll << 31)) return fail(FSLIC_E_INVALID, "C * nnz must be below 2^31");
    return FSLIC_OK;
}

}  // namespace

extern "C" {

int fslic_hip_message_gather(int device, void* stream, int N, int C, int K, long long nnz, int end, const int32_t* rows, const int32_t* indices,
                             const float* values, const int32_t* scale_degree, const int32_t* argmax, float* out) {
    const int rc = check_call(device, N, C, K, nnz);
    if (rc) return rc;
    if (end != kMsgTarget && end != kMsgSource) return fail(FSLIC_E_INVALID, "end must be 0 (target) or 1 (source)");
    if (!values || (nnz > 0 && (!rows || !indices || !out))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (nnz == 0) return FSLIC_OK;
    return on_stream(device, stream, "message launch", [&](hipStream_t st) -> int {
        launch_message_gather(end, rows, indices, values, scale_degree, argmax, out, N, C, K, nnz, st);
        return FSLIC_OK;
    });
}

int fslic_hip_message_reduce(int device, void* stream, int N, int C, int K, long long nnz, int reduce, int transposed, const int64_t* offsets,
                             const int32_t* ia, const int32_t* ib, const float* messages, float* out, int32_t* argmax, int32_t* degree) {
    const int rc = check_call(device, N, C, K, nnz);
    if (rc) return rc;
    if (reduce != kMsgSum && reduce != kMsgMean && reduce != kMsgMax && reduce != kMsgMin)
        return fail(FSLIC_E_INVALID, "reduce must be 0 (sum), 1 (mean), 2 (max) or 3 (min)");
    if (transposed != 0 && transposed != 1) return fail(FSLIC_E_INVALID, "transposed must be 0 or 1");
    if ((reduce == kMsgMax || reduce == kMsgMin) && !argmax) return fail(FSLIC_E_INVALID, "reduce 2 (max) and 3 (min) need argmax");
    if (reduce == kMsgMean && !degree) return fail(FSLIC_E_INVALID, "reduce 1 (mean) needs degree");
    if (!offsets || !out || (nnz > 0 && (!ia || !messages || (transposed && !ib)))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "message launch", [&](hipStream_t st) -> int {
        launch_message_reduce(reduce, transposed != 0, i64(offsets), ia, ib, messages, out, argmax, degree, N, C, K, nnz, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
