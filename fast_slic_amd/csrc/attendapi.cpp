// attendapi.cpp -- the C ABI of attention over neighbour lists (include/fslic_hip.h, fslic_hip_attend_*; kernels in attend.hip), on
// streamapi.h; nothing here synchronises, allocates or copies to the host.
#include "attend.h"
#include "streamapi.h"

using namespace fslic;

namespace {

// the heads, the channels they divide (C = 0: an entry without channels) and the cells of a [heads][nnz] array
int check_heads(int heads, int C, long long nnz) {
    if (heads < 1) return fail(FSLIC_E_INVALID, "heads must be positive");
    if (C % heads != 0) return fail(FSLIC_E_INVALID, "C must be a multiple of heads");
    if ((long long)heads * nnz >= (1ll << 31)) return fail(FSLIC_E_INVALID, "heads * nnz must be below 2^31");
    return FSLIC_OK;
}

// the device, the cells of a [N][C][K] array, the entries of the lists and the heads
int check_call(int device, int N, int C, int K, long long nnz, int heads) {
    int rc = check_device(device);
    if (rc || (rc = check_cells(N, C, K, "K")) || (rc = check_entry_count(nnz, "nnz"))) return rc;
    return check_heads(heads, C, nnz);
}

// the same for the softmax, which sees rows and no channels
int check_rows_call(int device, int N, int K, long long nnz, int heads) {
    int rc = check_device(device);
    if (rc) return rc;
    if (N < 1) return fail(FSLIC_E_INVALID, "N must be positive");
    if ((rc = check_node_count(K, "K"))) return rc;
    if ((long long)N * K >= (1ll << 31)) return fail(FSLIC_E_INVALID, "N * K must be below 2^31");
    if ((rc = check_entry_count(nnz, "nnz"))) return rc;
    return check_heads(heads, 0, nnz);
}

}  // namespace

extern "C" {

int fslic_hip_attend_dot(int device, void* stream, int N, int C, int K, long long nnz, int heads, const int32_t* rows, const int32_t* indices,
                         const float* a, const float* b, float* out) {
    const int rc = check_call(device, N, C, K, nnz, heads);
    if (rc) return rc;
    if (!a || !b || (nnz > 0 && (!rows || !indices || !out))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (nnz == 0) return FSLIC_OK;
    return on_stream(device, stream, "attend launch", [&](hipStream_t st) -> int {
        launch_attend_dot(rows, indices, a, b, out, N, C, K, nnz, heads, st);
        return FSLIC_OK;
    });
}

int fslic_hip_attend_softmax(int device, void* stream, int N, int K, long long nnz, int heads, const int64_t* offsets, const int32_t* indices,
                             const float* scores, float* out) {
    const int rc = check_rows_call(device, N, K, nnz, heads);
    if (rc) return rc;
    if (!offsets || (nnz > 0 && (!indices || !scores || !out))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (nnz == 0) return FSLIC_OK;
    return on_stream(device, stream, "attend launch", [&](hipStream_t st) -> int {
        launch_attend_softmax(i64(offsets), indices, scores, nullptr, out, N, K, nnz, heads, st);
        return FSLIC_OK;
    });
}

int fslic_hip_attend_softmax_backward(int device, void* stream, int N, int K, long long nnz, int heads, const int64_t* offsets,
                                      const int32_t* indices, const float* alpha, const float* grad_out, float* grad_scores) {
    const int rc = check_rows_call(device, N, K, nnz, heads);
    if (rc) return rc;
    if (!offsets || (nnz > 0 && (!indices || !alpha || !grad_out || !grad_scores))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (nnz == 0) return FSLIC_OK;
    return on_stream(device, stream, "attend launch", [&](hipStream_t st) -> int {
        launch_attend_softmax(i64(offsets), indices, alpha, grad_out, grad_scores, N, K, nnz, heads, st);
        return FSLIC_OK;
    });
}

int fslic_hip_attend_apply(int device, void* stream, int N, int C, int K, long long nnz, int heads, int transposed, const int64_t* offsets,
                           const int32_t* ia, const int32_t* ib, const float* weight, const float* src, float* dst) {
    const int rc = check_call(device, N, C, K, nnz, heads);
    if (rc) return rc;
    if (transposed != 0 && transposed != 1) return fail(FSLIC_E_INVALID, "transposed must be 0 or 1");
    if (!offsets || !src || !dst || (nnz > 0 && (!ia || !weight || (transposed && !ib)))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "attend launch", [&](hipStream_t st) -> int {
        launch_attend_apply(transposed != 0, attend_pack(C / heads), i64(offsets), ia, ib, weight, src, dst, N, C, K, nnz, heads, st);
        return FSLIC_OK;
    });
}

}  // extern "C"
