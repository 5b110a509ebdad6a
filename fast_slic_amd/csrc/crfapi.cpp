// crfapi.cpp -- the C ABI of SimpleCRF inference on device tensors (include/fslic_hip.h, fslic_hip_crf_tensor_*; kernels in
// crf_tensor.hip, crf_tensor_grad.hip).  No engine: the caller names the device and the stream and owns every buffer.  Every argument is checked before the
// first HIP call; the call enqueues and returns.
#include "engine_internal.h"
#include "crf_tensor.h"
#include "crf_tensor_grad.h"
#include "streamapi.h"

using namespace fslic;

namespace {

int check_sizes(int N, int C, int K, long long nnz) {
    if (N < 1 || C < 1 || K < 1) return fail(FSLIC_E_INVALID, "N, C and K must be positive");
    if (nnz < 0 || nnz >= (1ll << 31)) return fail(FSLIC_E_INVALID, "nnz must be in [0, 2^31)");
    if ((long long)N * C * K >= (1ll << 31) || (long long)N * K + 1 >= (1ll << 31))
        return fail(FSLIC_E_INVALID, "N * C * K and N * K + 1 must be below 2^31");
    return FSLIC_OK;
}

// What fslic_hip_crf_tensor_inference checks ahead of its pointers, for the entries of the differentiable path.
int check_call(int device, int N, int C, int K, long long nnz, int temporal, int max_iter) {
    if (device < 0) return fail(FSLIC_E_INVALID, "device must be >= 0");
    const int rc = check_sizes(N, C, K, nnz);
    if (rc) return rc;
    if (temporal != 0 && temporal != 1) return fail(FSLIC_E_INVALID, "temporal must be 0 or 1");
    if (max_iter < 0) return fail(FSLIC_E_INVALID, "max_iter must be >= 0");
    return FSLIC_OK;
}

int check_workspace(const void* workspace, size_t workspace_bytes, size_t needed) {
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(FSLIC_E_INVALID, "workspace must be 16-byte aligned");
    if (workspace_bytes < needed) return fail(FSLIC_E_INVALID, "workspace too small: " + std::to_string(needed) + " bytes needed");
    return FSLIC_OK;
}

// Where a call's energies come from: computed from host params and the clusters' yxrgb, or given per entry and per link.
struct EnergySource {
    const fslic_crf_params* params;     // with yxrgb; NULL: the energies are given
    const float* yxrgb;
    const float* edge;                  // [nnz]
    const float* links;                 // [N][2][K] or NULL
};

CrfTensorParams tensor_params(int N, int C, int K, int temporal, long long nnz, const EnergySource& src) {
    CrfTensorParams dp = {};
    dp.N = N; dp.C = C; dp.K = K; dp.temporal = temporal; dp.nnz = nnz;
    if (src.params) dp.p = *src.params;
    return dp;
}

void launch_edges(const CrfTensorParams& dp, const EnergySource& src, const int32_t* members, const int64_t* offsets,
                  const int32_t* indices, uint2* rows, float2* edge, float4* tmp, hipStream_t st) {
    if (src.params) launch_crf_tensor_edges(dp, src.yxrgb, members, offsets, indices, rows, edge, tmp, st);
    else launch_crf_tensor_edges_given(dp, src.edge, src.links, members, offsets, indices, rows, edge, tmp, st);
}

int launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FSLIC_OK : fail(FSLIC_E_HIP, std::string("crf tensor launch: ") + hipGetErrorString(e));
}

// The bodies of the entries below, behind their argument checks.
int run_inference(int device, void* stream, int N, int C, int K, int temporal, int max_iter, const EnergySource& src,
                  const float* compat, const int32_t* members, const int64_t* offsets, const int32_t* indices, long long nnz,
                  const float* unaries, const float* q0, float* q_out, void* workspace, const CrfTensorWorkspace& ws) {
    int rc;
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(workspace);
    float* buf[2] = {q_out, reinterpret_cast<float*>(base + ws.q)};
    // sweep `it` writes buf[(max_iter - 1 - it) & 1], so that the last one writes q_out; the starting q sits where the first sweep
    // does not write: q0 itself when it is given (it is only read), buf[max_iter & 1] otherwise
    const size_t cells = (size_t)N * C * K;
    const float* q_in = q0;
    if (!q0 || max_iter == 0) {
        float* start = buf[max_iter & 1];
        launch_crf_tensor_start(unaries, q0, start, cells, st);
        q_in = start;
    }
    if (max_iter > 0) {
        const CrfTensorParams dp = tensor_params(N, C, K, temporal, nnz, src);
        uint2* rows = reinterpret_cast<uint2*>(base + ws.rows);
        float2* edge = reinterpret_cast<float2*>(base + ws.edge);
        float4* tmp = reinterpret_cast<float4*>(base + ws.temporal);
        float* msg = reinterpret_cast<float*>(base + ws.msg);
        launch_edges(dp, src, members, offsets, indices, rows, edge, tmp, st);
        for (int it = 0; it < max_iter; it++) {
            float* out = buf[(max_iter - 1 - it) & 1];
            launch_crf_tensor_sweep(dp, rows, indices, edge, tmp, unaries, compat, q_in, out, msg, st);
            q_in = out;
        }
    }
    return launch_status();
}

int run_inference_saved(int device, void* stream, int N, int C, int K, int temporal, int max_iter, const EnergySource& src,
                        const float* compat, const int32_t* members, const int64_t* offsets, const int32_t* indices, long long nnz,
                        const float* unaries, const float* q0, float* q_all, void* workspace, const CrfTensorGradWorkspace& ws) {
    int rc;
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(workspace);
    const size_t cells = (size_t)N * C * K;
    // plane 0 is the starting q, plane it + 1 what sweep `it` writes: the ping-pong of fslic_hip_crf_tensor_inference unrolled
    launch_crf_tensor_start(unaries, q0, q_all, cells, st);
    if (max_iter > 0) {
        const CrfTensorParams dp = tensor_params(N, C, K, temporal, nnz, src);
        uint2* rows = reinterpret_cast<uint2*>(base + ws.rows);
        float2* edge = reinterpret_cast<float2*>(base + ws.edge);
        float4* tmp = reinterpret_cast<float4*>(base + ws.temporal);
        float* msg = reinterpret_cast<float*>(base + ws.msg);
        launch_edges(dp, src, members, offsets, indices, rows, edge, tmp, st);
        for (int it = 0; it < max_iter; it++)
            launch_crf_tensor_sweep(dp, rows, indices, edge, tmp, unaries, compat, q_all + (size_t)it * cells,
                                    q_all + (size_t)(it + 1) * cells, msg, st);
    }
    return launch_status();
}

// grad_edge [nnz] and grad_links [N][2][K] (either may be NULL) are zeroed on the stream and filled behind each sweep's adjoint.
int run_backward(int device, void* stream, int N, int C, int K, int temporal, int max_iter, const EnergySource& src,
                 const float* compat, const int32_t* members, const int64_t* offsets, const int32_t* indices, long long nnz,
                 const CrfTensorTransposed& tr, const float* unaries, const float* q_all, const float* grad_q, float* grad_unaries,
                 float* grad_q0, float* grad_compat, float* grad_edge, float* grad_links, void* workspace,
                 const CrfTensorGradWorkspace& ws) {
    int rc;
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(workspace);
    const size_t cells = (size_t)N * C * K, blocks = crf_tensor_grad_blocks(N, K);
    const CrfTensorParams dp = tensor_params(N, C, K, temporal, nnz, src);
    uint2* rows = reinterpret_cast<uint2*>(base + ws.rows);
    float2* edge = reinterpret_cast<float2*>(base + ws.edge);
    float4* tmp = reinterpret_cast<float4*>(base + ws.temporal);
    float* msg = reinterpret_cast<float*>(base + ws.msg);
    float* dm[2] = {reinterpret_cast<float*>(base + ws.dm), reinterpret_cast<float*>(base + ws.dm) + cells};
    float* x = reinterpret_cast<float*>(base + ws.x);
    float* slots = grad_compat ? reinterpret_cast<float*>(base + ws.slots) : nullptr;
    if (grad_edge && nnz > 0) HIPCHK(hipMemsetAsync(grad_edge, 0, (size_t)nnz * sizeof(float), st));
    if (grad_links) HIPCHK(hipMemsetAsync(grad_links, 0, (size_t)N * 2 * K * sizeof(float), st));
    // the energy gradients of a sweep need that sweep's dm alone; without entries and without links there is nothing to add
    const bool energy_grad = (grad_edge && nnz > 0) || (grad_links && temporal && N > 1);
    if (max_iter > 0) {
        // the energies again rather than the forward's workspace: nothing but the iterates stays alive between the two calls
        launch_edges(dp, src, members, offsets, indices, rows, edge, tmp, st);
        for (int it = max_iter - 1; it >= 0; it--) {
            const bool first = it == max_iter - 1;
            launch_crf_tensor_sweep_bwd(dp, rows, indices, edge, tmp, tr, unaries, compat, q_all + (size_t)it * cells,
                                        q_all + (size_t)(it + 1) * cells, first ? grad_q : nullptr, dm[(it + 1) & 1], dm[it & 1],
                                        grad_unaries, slots, msg, x, first, st);
            if (energy_grad)
                launch_crf_tensor_energy_grad(dp, rows, indices, edge, tmp, tr, dm[it & 1], q_all + (size_t)it * cells,
                                              nnz > 0 ? grad_edge : nullptr, grad_links, st);
        }
    }
    launch_crf_tensor_grad_close(dp, rows, edge, tmp, tr, q_all, max_iter > 0 ? nullptr : grad_q, dm[0], grad_unaries, grad_q0,
                                 max_iter == 0, st);
    if (grad_compat) launch_crf_tensor_grad_compat(slots, max_iter > 0 ? blocks : 0, C, grad_compat, st);
    return launch_status();
}

}  // namespace

extern "C" {

int fslic_hip_crf_tensor_workspace_size(int N, int C, int K, long long nnz, size_t* bytes) {
    if (!bytes) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const int rc = check_sizes(N, C, K, nnz);
    if (rc) return rc;
    *bytes = crf_tensor_workspace(N, C, K, nnz).bytes;
    return FSLIC_OK;
}

int fslic_hip_crf_tensor_inference(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                   const fslic_crf_params* params, const float* compat, const float* yxrgb, const int32_t* members,
                                   const int64_t* offsets, const int32_t* indices, long long nnz, const float* unaries, const float* q0,
                                   float* q_out, void* workspace, size_t workspace_bytes) {
    if (device < 0) return fail(FSLIC_E_INVALID, "device must be >= 0");
    int rc = check_sizes(N, C, K, nnz);
    if (rc) return rc;
    if (temporal != 0 && temporal != 1) return fail(FSLIC_E_INVALID, "temporal must be 0 or 1");
    if (max_iter < 0) return fail(FSLIC_E_INVALID, "max_iter must be >= 0");
    if (!params || !compat || !yxrgb || !members || !offsets || !unaries || !q_out || !workspace || (!indices && nnz > 0))
        return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(FSLIC_E_INVALID, "workspace must be 16-byte aligned");
    const CrfTensorWorkspace ws = crf_tensor_workspace(N, C, K, nnz);
    if (workspace_bytes < ws.bytes) return fail(FSLIC_E_INVALID, "workspace too small: " + std::to_string(ws.bytes) + " bytes needed");
    const EnergySource src = {params, yxrgb, nullptr, nullptr};
    return run_inference(device, stream, N, C, K, temporal, max_iter, src, compat, members, offsets, indices, nnz, unaries, q0, q_out,
                         workspace, ws);
}

int fslic_hip_crf_tensor_grad_workspace_size(int N, int C, int K, long long nnz, int backward, int with_compat, size_t* bytes) {
    if (!bytes) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const int rc = check_sizes(N, C, K, nnz);
    if (rc) return rc;
    if ((backward != 0 && backward != 1) || (with_compat != 0 && with_compat != 1))
        return fail(FSLIC_E_INVALID, "backward and with_compat must be 0 or 1");
    *bytes = crf_tensor_grad_workspace(N, C, K, nnz, backward != 0, with_compat != 0).bytes;
    return FSLIC_OK;
}

int fslic_hip_crf_tensor_inference_saved(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                         const fslic_crf_params* params, const float* compat, const float* yxrgb, const int32_t* members,
                                         const int64_t* offsets, const int32_t* indices, long long nnz, const float* unaries,
                                         const float* q0, float* q_all, void* workspace, size_t workspace_bytes) {
    int rc = check_call(device, N, C, K, nnz, temporal, max_iter);
    if (rc) return rc;
    if (!params || !compat || !yxrgb || !members || !offsets || !unaries || !q_all || !workspace || (!indices && nnz > 0))
        return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const CrfTensorGradWorkspace ws = crf_tensor_grad_workspace(N, C, K, nnz, false, false);
    if ((rc = check_workspace(workspace, workspace_bytes, ws.bytes))) return rc;
    const EnergySource src = {params, yxrgb, nullptr, nullptr};
    return run_inference_saved(device, stream, N, C, K, temporal, max_iter, src, compat, members, offsets, indices, nnz, unaries, q0,
                               q_all, workspace, ws);
}

int fslic_hip_crf_tensor_backward(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                  const fslic_crf_params* params, const float* compat, const float* yxrgb, const int32_t* members,
                                  const int64_t* offsets, const int32_t* indices, long long nnz, const int64_t* t_offsets,
                                  const int32_t* t_entries, const int32_t* t_rows, const float* unaries, const float* q_all,
                                  const float* grad_q, float* grad_unaries, float* grad_q0, float* grad_compat, void* workspace,
                                  size_t workspace_bytes) {
    int rc = check_call(device, N, C, K, nnz, temporal, max_iter);
    if (rc) return rc;
    if (!params || !compat || !yxrgb || !members || !offsets || !t_offsets || !unaries || !q_all || !grad_q || !grad_unaries ||
        !workspace || ((!indices || !t_entries || !t_rows) && nnz > 0))
        return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const CrfTensorGradWorkspace ws = crf_tensor_grad_workspace(N, C, K, nnz, true, grad_compat != nullptr);
    if ((rc = check_workspace(workspace, workspace_bytes, ws.bytes))) return rc;
    const EnergySource src = {params, yxrgb, nullptr, nullptr};
    const CrfTensorTransposed tr = {t_offsets, t_entries, t_rows};
    return run_backward(device, stream, N, C, K, temporal, max_iter, src, compat, members, offsets, indices, nnz, tr, unaries, q_all,
                        grad_q, grad_unaries, grad_q0, grad_compat, nullptr, nullptr, workspace, ws);
}

// ---- the energies as tensors: forward, backward to the params, and the three entries above with given energies ----
int fslic_hip_crf_tensor_energies(int device, void* stream, int N, int K, int temporal, const float* params, const float* yxrgb,
                                  const int32_t* members, const int64_t* offsets, const int32_t* indices, long long nnz,
                                  float* edge, float* links) {
    int rc = check_call(device, N, 1, K, nnz, temporal, 0);
    if (rc) return rc;
    if (!params || !yxrgb || !members || !offsets || !links || ((!indices || !edge) && nnz > 0))
        return fail(FSLIC_E_INVALID, "NULL pointer argument");
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const EnergySource none = {};
    const CrfTensorParams dp = tensor_params(N, 1, K, temporal, nnz, none);
    if (nnz > 0) HIPCHK(hipMemsetAsync(edge, 0, (size_t)nnz * sizeof(float), st));      // the entries outside every clamped row
    launch_crf_tensor_energies(dp, params, yxrgb, members, offsets, indices, edge, links, st);
    return launch_status();
}

int fslic_hip_crf_tensor_energies_backward_workspace_size(int N, int K, size_t* bytes) {
    if (!bytes) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const int rc = check_sizes(N, 1, K, 0);
    if (rc) return rc;
    *bytes = crf_tensor_param_grad_workspace(N, K);
    return FSLIC_OK;
}

int fslic_hip_crf_tensor_energies_backward(int device, void* stream, int N, int K, int temporal, const float* params, const float* yxrgb,
                                           const int64_t* offsets, const int32_t* indices, long long nnz, const float* grad_edge,
                                           const float* grad_links, float* grad_params, void* workspace, size_t workspace_bytes) {
    int rc = check_call(device, N, 1, K, nnz, temporal, 0);
    if (rc) return rc;
    if (!params || !yxrgb || !offsets || !grad_params || !workspace || (!indices && nnz > 0))
        return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if ((rc = check_workspace(workspace, workspace_bytes, crf_tensor_param_grad_workspace(N, K)))) return rc;
    DeviceScope scope;
    if ((rc = scope.enter(device))) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const EnergySource none = {};
    const CrfTensorParams dp = tensor_params(N, 1, K, temporal, nnz, none);
    launch_crf_tensor_param_grad(dp, params, yxrgb, offsets, indices, nnz > 0 ? grad_edge : nullptr, grad_links,
                                 reinterpret_cast<double*>(workspace), grad_params, st);
    return launch_status();
}

int fslic_hip_crf_tensor_inference_energies(int device, void* stream, int N, int C, int K, int temporal, int max_iter, const float* compat,
                                            const int32_t* members, const int64_t* offsets, const int32_t* indices, long long nnz,
                                            const float* edge, const float* links, const float* unaries, const float* q0, float* q_out,
                                            void* workspace, size_t workspace_bytes) {
    int rc = check_call(device, N, C, K, nnz, temporal, max_iter);
    if (rc) return rc;
    if (!compat || !members || !offsets || !unaries || !q_out || !workspace || ((!indices || !edge) && nnz > 0))
        return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const CrfTensorWorkspace ws = crf_tensor_workspace(N, C, K, nnz);
    if ((rc = check_workspace(workspace, workspace_bytes, ws.bytes))) return rc;
    const EnergySource src = {nullptr, nullptr, edge, links};
    return run_inference(device, stream, N, C, K, temporal, max_iter, src, compat, members, offsets, indices, nnz, unaries, q0, q_out,
                         workspace, ws);
}

int fslic_hip_crf_tensor_inference_saved_energies(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                                  const float* compat, const int32_t* members, const int64_t* offsets,
                                                  const int32_t* indices, long long nnz, const float* edge, const float* links,
                                                  const float* unaries, const float* q0, float* q_all, void* workspace,
                                                  size_t workspace_bytes) {
    int rc = check_call(device, N, C, K, nnz, temporal, max_iter);
    if (rc) return rc;
    if (!compat || !members || !offsets || !unaries || !q_all || !workspace || ((!indices || !edge) && nnz > 0))
        return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const CrfTensorGradWorkspace ws = crf_tensor_grad_workspace(N, C, K, nnz, false, false);
    if ((rc = check_workspace(workspace, workspace_bytes, ws.bytes))) return rc;
    const EnergySource src = {nullptr, nullptr, edge, links};
    return run_inference_saved(device, stream, N, C, K, temporal, max_iter, src, compat, members, offsets, indices, nnz, unaries, q0,
                               q_all, workspace, ws);
}

int fslic_hip_crf_tensor_backward_energies(int device, void* stream, int N, int C, int K, int temporal, int max_iter, const float* compat,
                                           const int32_t* members, const int64_t* offsets, const int32_t* indices, long long nnz,
                                           const float* edge, const float* links, const int64_t* t_offsets, const int32_t* t_entries,
                                           const int32_t* t_rows, const float* unaries, const float* q_all, const float* grad_q,
                                           float* grad_unaries, float* grad_q0, float* grad_compat, float* grad_edge, float* grad_links,
                                           void* workspace, size_t workspace_bytes) {
    int rc = check_call(device, N, C, K, nnz, temporal, max_iter);
    if (rc) return rc;
    if (!compat || !members || !offsets || !t_offsets || !unaries || !q_all || !grad_q || !grad_unaries || !workspace ||
        ((!indices || !edge || !t_entries || !t_rows) && nnz > 0))
        return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const CrfTensorGradWorkspace ws = crf_tensor_grad_workspace(N, C, K, nnz, true, grad_compat != nullptr);
    if ((rc = check_workspace(workspace, workspace_bytes, ws.bytes))) return rc;
    const EnergySource src = {nullptr, nullptr, edge, links};
    const CrfTensorTransposed tr = {t_offsets, t_entries, t_rows};
    return run_backward(device, stream, N, C, K, temporal, max_iter, src, compat, members, offsets, indices, nnz, tr, unaries, q_all,
                        grad_q, grad_unaries, grad_q0, grad_compat, grad_edge, grad_links, workspace, ws);
}

}  // extern "C"
