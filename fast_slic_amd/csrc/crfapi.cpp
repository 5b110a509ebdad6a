// crfapi.cpp -- the C ABI of SimpleCRF inference on device tensors (include/fslic_hip.h, fslic_hip_crf_tensor_*; kernels in
// crf_tensor.hip, crf_tensor_grad.hip), on streamapi.h; a call enqueues and returns.
#include "crf_tensor.h"
#include "crf_tensor_grad.h"
#include "streamapi.h"

using namespace fslic;

namespace {

int check_sizes(int N, int C, int K, long long nnz) {
    if (N < 1 || C < 1 || K < 1) return fail(FSLIC_E_INVALID, "N, C and K must be positive");
    const int rc = check_entry_count(nnz, "nnz");
    if (rc) return rc;
    if ((long long)N * C * K >= (1ll << 31) || (long long)N * K + 1 >= (1ll << 31))
        return fail(FSLIC_E_INVALID, "N * C * K and N * K + 1 must be below 2^31");
    return FSLIC_OK;
}

// What every entry with a device checks ahead of its pointers.
int check_call(int device, int N, int C, int K, long long nnz, int temporal, int max_iter) {
    int rc = check_device(device);
    if (rc || (rc = check_sizes(N, C, K, nnz))) return rc;
    if (temporal != 0 && temporal != 1) return fail(FSLIC_E_INVALID, "temporal must be 0 or 1");
    if (max_iter < 0) return fail(FSLIC_E_INVALID, "max_iter must be >= 0");
    return FSLIC_OK;
}

// the parts of a workspace are 16-byte aligned from its start
int check_aligned_workspace(const void* workspace, size_t workspace_bytes, size_t need) {
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(FSLIC_E_INVALID, "workspace must be 16-byte aligned");
    return check_workspace(workspace_bytes, need);
}

// Where a call's energies come from: computed from host params and the clusters' yxrgb, or given per entry and per link.
struct EnergySource {
    const fslic_crf_params* params;     // with yxrgb; NULL: the energies are given
    const float* yxrgb;
    const float* edge;                  // [nnz]
    const float* links;                 // [N][2][K] or NULL
};

// One call of the three entries with sweeps and of their _energies forms: what all of them are given.
struct CrfCall {
    int device;
    void* stream;
    int N, C, K, temporal, max_iter;
    long long nnz;
    EnergySource src;
    const float* compat;
    const int32_t* members;
    const int64_t* offsets;
    const int32_t* indices;
    const float* unaries;
    void* workspace;
    size_t workspace_bytes;
};

CrfTensorParams tensor_params(int N, int C, int K, int temporal, long long nnz, const fslic_crf_params* params) {
    CrfTensorParams dp = {};
    dp.N = N; dp.C = C; dp.K = K; dp.temporal = temporal; dp.nnz = nnz;
    if (params) dp.p = *params;
    return dp;
}

// The checks of such a call, in the order of every entry: the numbers, the pointers (`own`: the entry's own and its energy source's
// are there), the workspace.  -> the layout of the workspace in *ws.
int check(const CrfCall& c, bool own, CrfTensorCall kind, bool with_compat, CrfTensorWorkspace* ws) {
    const int rc = check_call(c.device, c.N, c.C, c.K, c.nnz, c.temporal, c.max_iter);
    if (rc) return rc;
    if (!own || !c.compat || !c.members || !c.offsets || !c.unaries || !c.workspace || (!c.indices && c.nnz > 0))
        return fail(FSLIC_E_INVALID, "NULL pointer argument");
    *ws = crf_tensor_workspace(c.N, c.C, c.K, c.nnz, kind, with_compat);
    return check_aligned_workspace(c.workspace, c.workspace_bytes, ws->bytes);
}

void launch_edges(const CrfCall& c, const CrfTensorParams& dp, const CrfTensorBuffers& b, hipStream_t st) {
    if (c.src.params) launch_crf_tensor_edges(dp, c.src.yxrgb, c.members, c.offsets, c.indices, b.rows, b.edge, b.temporal, st);
    else launch_crf_tensor_edges_given(dp, c.src.edge, c.src.links, c.members, c.offsets, c.indices, b.rows, b.edge, b.temporal, st);
}

// The bodies of the entries below.
// The forward: the start, the edge pass and max_iter sweeps.  at(it) is where iterate `it` lives: sweep `it` reads at(it) and writes
// at(it + 1).  `placed`: the starting q where it already is; NULL: the start launch writes it to at(0).
template <class At>
int run_forward(const CrfCall& c, const CrfTensorWorkspace& ws, const float* q0, const float* placed, At at) {
    return on_stream(c.device, c.stream, "crf tensor launch", [&](hipStream_t st) -> int {
        const float* q_in = placed;
        if (!placed) {
            launch_crf_tensor_start(c.unaries, q0, at(0), (size_t)c.N * c.C * c.K, st);
            q_in = at(0);
        }
        if (c.max_iter > 0) {
            const CrfTensorParams dp = tensor_params(c.N, c.C, c.K, c.temporal, c.nnz, c.src.params);
            const CrfTensorBuffers b = crf_tensor_buffers(c.workspace, ws);
            launch_edges(c, dp, b, st);
            for (int it = 0; it < c.max_iter; it++) {
                launch_crf_tensor_sweep(dp, b.lists(), c.indices, c.unaries, c.compat, q_in, at(it + 1), b.msg, st);
                q_in = at(it + 1);
            }
        }
        return FSLIC_OK;
    });
}

int run_inference(const CrfCall& c, bool own, const float* q0, float* q_out) {
    CrfTensorWorkspace ws;
    const int rc = check(c, own && q_out, kCrfCallPlain, false, &ws);
    if (rc) return rc;
    // a ping-pong between q_out and the workspace's q that ends in q_out: iterate `it` lives in buf[(max_iter - it) & 1].  A given
    // q0 is only read, so the first sweep reads it where it is
    float* buf[2] = {q_out, crf_tensor_buffers(c.workspace, ws).q};
    const int max_iter = c.max_iter;
    return run_forward(c, ws, q0, max_iter > 0 ? q0 : nullptr, [&](int it) { return buf[(max_iter - it) & 1]; });
}

int run_inference_saved(const CrfCall& c, bool own, const float* q0, float* q_all) {
    CrfTensorWorkspace ws;
    const int rc = check(c, own && q_all, kCrfCallSaved, false, &ws);
    if (rc) return rc;
    // iterate `it` is plane `it` of q_all: the ping-pong of run_inference unrolled
    const size_t cells = (size_t)c.N * c.C * c.K;
    return run_forward(c, ws, q0, nullptr, [&](int it) { return q_all + (size_t)it * cells; });
}

// grad_edge [nnz] and grad_links [N][2][K] (either may be NULL) are zeroed on the stream and filled behind each sweep's adjoint.
int run_backward(const CrfCall& c, bool own, const CrfTensorTransposed& tr, const float* q_all, const float* grad_q, float* grad_unaries,
                 float* grad_q0, float* grad_compat, float* grad_edge, float* grad_links) {
    CrfTensorWorkspace ws;
    const int rc = check(c, own && tr.offsets && q_all && grad_q && grad_unaries && ((tr.entries && tr.rows) || c.nnz == 0), kCrfCallBackward,
                         grad_compat != nullptr, &ws);
    if (rc) return rc;
    return on_stream(c.device, c.stream, "crf tensor launch", [&](hipStream_t st) -> int {
        const int N = c.N, K = c.K, max_iter = c.max_iter;
        const long long nnz = c.nnz;
        const size_t cells = (size_t)N * c.C * K;
        const CrfTensorParams dp = tensor_params(N, c.C, K, c.temporal, nnz, c.src.params);
        const CrfTensorBuffers b = crf_tensor_buffers(c.workspace, ws);
        const CrfGradLists lists = {b.lists(), tr};
        float* dm[2] = {b.dm, b.dm + cells};
        float* slots = grad_compat ? b.slots : nullptr;
        if (grad_edge && nnz > 0) HIPCHK(hipMemsetAsync(grad_edge, 0, (size_t)nnz * sizeof(float), st));
        if (grad_links) HIPCHK(hipMemsetAsync(grad_links, 0, (size_t)N * 2 * K * sizeof(float), st));
        // the energy gradients of a sweep need that sweep's dm alone; without entries and without links there is nothing to add
        const bool energy_grad = (grad_edge && nnz > 0) || (grad_links && c.temporal && N > 1);
        if (max_iter > 0) {
            // the energies again rather than the forward's workspace: nothing but the iterates stays alive between the two calls
            launch_edges(c, dp, b, st);
            for (int it = max_iter - 1; it >= 0; it--) {
                const bool first = it == max_iter - 1;
                launch_crf_tensor_sweep_bwd(dp, lists, c.indices, c.unaries, c.compat, q_all + (size_t)it * cells,
                                            q_all + (size_t)(it + 1) * cells, first ? grad_q : nullptr, dm[(it + 1) & 1], dm[it & 1],
                                            grad_unaries, slots, b.msg, b.x, first, st);
                if (energy_grad)
                    launch_crf_tensor_energy_grad(dp, lists, c.indices, dm[it & 1], q_all + (size_t)it * cells, nnz > 0 ? grad_edge : nullptr,
                                                  grad_links, st);
            }
        }
        launch_crf_tensor_grad_close(dp, lists, q_all, max_iter > 0 ? nullptr : grad_q, dm[0], grad_unaries, grad_q0, max_iter == 0, st);
        if (grad_compat)
            launch_crf_tensor_grad_compat(slots, max_iter > 0 ? crf_tensor_sweep_shape(N, c.C, K).grid : 0, c.C, grad_compat, st);
        return FSLIC_OK;
    });
}

}  // namespace

extern "C" {

int fslic_hip_crf_tensor_workspace_size(int N, int C, int K, long long nnz, size_t* bytes) {
    return workspace_size(bytes, [&] { return check_sizes(N, C, K, nnz); }, [&] { return crf_tensor_workspace(N, C, K, nnz, kCrfCallPlain, false).bytes; });
}

int fslic_hip_crf_tensor_inference(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                   const fslic_crf_params* params, const float* compat, const float* yxrgb, const int32_t* members,
                                   const int64_t* offsets, const int32_t* indices, long long nnz, const float* unaries, const float* q0,
                                   float* q_out, void* workspace, size_t workspace_bytes) {
    const CrfCall c = {device, stream, N, C, K, temporal, max_iter, nnz, {params, yxrgb, nullptr, nullptr},
                       compat, members, offsets, indices, unaries, workspace, workspace_bytes};
    return run_inference(c, params && yxrgb, q0, q_out);
}

int fslic_hip_crf_tensor_grad_workspace_size(int N, int C, int K, long long nnz, int backward, int with_compat, size_t* bytes) {
    const auto check = [&] {
        const int rc = check_sizes(N, C, K, nnz);
        if (rc) return rc;
        if ((backward != 0 && backward != 1) || (with_compat != 0 && with_compat != 1))
            return fail(FSLIC_E_INVALID, "backward and with_compat must be 0 or 1");
        return (int)FSLIC_OK;
    };
    return workspace_size(bytes, check, [&] { return crf_tensor_workspace(N, C, K, nnz, backward ? kCrfCallBackward : kCrfCallSaved, with_compat != 0).bytes; });
}

int fslic_hip_crf_tensor_inference_saved(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                         const fslic_crf_params* params, const float* compat, const float* yxrgb, const int32_t* members,
                                         const int64_t* offsets, const int32_t* indices, long long nnz, const float* unaries,
                                         const float* q0, float* q_all, void* workspace, size_t workspace_bytes) {
    const CrfCall c = {device, stream, N, C, K, temporal, max_iter, nnz, {params, yxrgb, nullptr, nullptr},
                       compat, members, offsets, indices, unaries, workspace, workspace_bytes};
    return run_inference_saved(c, params && yxrgb, q0, q_all);
}

int fslic_hip_crf_tensor_backward(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                  const fslic_crf_params* params, const float* compat, const float* yxrgb, const int32_t* members,
                                  const int64_t* offsets, const int32_t* indices, long long nnz, const int64_t* t_offsets,
                                  const int32_t* t_entries, const int32_t* t_rows, const float* unaries, const float* q_all,
                                  const float* grad_q, float* grad_unaries, float* grad_q0, float* grad_compat, void* workspace,
                                  size_t workspace_bytes) {
    const CrfCall c = {device, stream, N, C, K, temporal, max_iter, nnz, {params, yxrgb, nullptr, nullptr},
                       compat, members, offsets, indices, unaries, workspace, workspace_bytes};
    return run_backward(c, params && yxrgb, {t_offsets, t_entries, t_rows}, q_all, grad_q, grad_unaries, grad_q0, grad_compat, nullptr,
                        nullptr);
}

// ---- the energies as tensors: forward, backward to the params, and the three entries above with given energies ----
int fslic_hip_crf_tensor_energies(int device, void* stream, int N, int K, int temporal, const float* params, const float* yxrgb,
                                  const int32_t* members, const int64_t* offsets, const int32_t* indices, long long nnz,
                                  float* edge, float* links) {
    const int rc = check_call(device, N, 1, K, nnz, temporal, 0);
    if (rc) return rc;
    if (!params || !yxrgb || !members || !offsets || !links || ((!indices || !edge) && nnz > 0))
        return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return on_stream(device, stream, "crf tensor launch", [&](hipStream_t st) -> int {
        const CrfTensorParams dp = tensor_params(N, 1, K, temporal, nnz, nullptr);
        if (nnz > 0) HIPCHK(hipMemsetAsync(edge, 0, (size_t)nnz * sizeof(float), st));      // the entries outside every clamped row
        launch_crf_tensor_energies(dp, params, yxrgb, members, offsets, indices, edge, links, st);
        return FSLIC_OK;
    });
}

int fslic_hip_crf_tensor_energies_backward_workspace_size(int N, int K, size_t* bytes) {
    return workspace_size(bytes, [&] { return check_sizes(N, 1, K, 0); }, [&] { return crf_tensor_param_grad_workspace(N, K); });
}

int fslic_hip_crf_tensor_energies_backward(int device, void* stream, int N, int K, int temporal, const float* params, const float* yxrgb,
                                           const int64_t* offsets, const int32_t* indices, long long nnz, const float* grad_edge,
                                           const float* grad_links, float* grad_params, void* workspace, size_t workspace_bytes) {
    int rc = check_call(device, N, 1, K, nnz, temporal, 0);
    if (rc) return rc;
    if (!params || !yxrgb || !offsets || !grad_params || !workspace || (!indices && nnz > 0))
        return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if ((rc = check_aligned_workspace(workspace, workspace_bytes, crf_tensor_param_grad_workspace(N, K)))) return rc;
    return on_stream(device, stream, "crf tensor launch", [&](hipStream_t st) -> int {
        const CrfTensorParams dp = tensor_params(N, 1, K, temporal, nnz, nullptr);
        launch_crf_tensor_param_grad(dp, params, yxrgb, offsets, indices, nnz > 0 ? grad_edge : nullptr, grad_links,
                                     reinterpret_cast<double*>(workspace), grad_params, st);
        return FSLIC_OK;
    });
}

int fslic_hip_crf_tensor_inference_energies(int device, void* stream, int N, int C, int K, int temporal, int max_iter, const float* compat,
                                            const int32_t* members, const int64_t* offsets, const int32_t* indices, long long nnz,
                                            const float* edge, const float* links, const float* unaries, const float* q0, float* q_out,
                                            void* workspace, size_t workspace_bytes) {
    const CrfCall c = {device, stream, N, C, K, temporal, max_iter, nnz, {nullptr, nullptr, edge, links},
                       compat, members, offsets, indices, unaries, workspace, workspace_bytes};
    return run_inference(c, edge || nnz == 0, q0, q_out);
}

int fslic_hip_crf_tensor_inference_saved_energies(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                                  const float* compat, const int32_t* members, const int64_t* offsets,
                                                  const int32_t* indices, long long nnz, const float* edge, const float* links,
                                                  const float* unaries, const float* q0, float* q_all, void* workspace,
                                                  size_t workspace_bytes) {
    const CrfCall c = {device, stream, N, C, K, temporal, max_iter, nnz, {nullptr, nullptr, edge, links},
                       compat, members, offsets, indices, unaries, workspace, workspace_bytes};
    return run_inference_saved(c, edge || nnz == 0, q0, q_all);
}

int fslic_hip_crf_tensor_backward_energies(int device, void* stream, int N, int C, int K, int temporal, int max_iter, const float* compat,
                                           const int32_t* members, const int64_t* offsets, const int32_t* indices, long long nnz,
                                           const float* edge, const float* links, const int64_t* t_offsets, const int32_t* t_entries,
                                           const int32_t* t_rows, const float* unaries, const float* q_all, const float* grad_q,
                                           float* grad_unaries, float* grad_q0, float* grad_compat, float* grad_edge, float* grad_links,
                                           void* workspace, size_t workspace_bytes) {
    const CrfCall c = {device, stream, N, C, K, temporal, max_iter, nnz, {nullptr, nullptr, edge, links},
                       compat, members, offsets, indices, unaries, workspace, workspace_bytes};
    return run_backward(c, edge || nnz == 0, {t_offsets, t_entries, t_rows}, q_all, grad_q, grad_unaries, grad_q0, grad_compat, grad_edge,
                        grad_links);
}

}  // extern "C"
