// crf_tensor_grad.h -- the backward of SimpleCRF inference on device tensors (crf_tensor_grad.hip, crfapi.cpp).  Internal to the library.
// The workspace of a backward call is crf_tensor.h's.
//
// Workspace of one fslic_hip_crf_tensor_energies_backward call:
//   slots[blocks][7]     double  -- per block of 256 (frame, node) threads its part of the gradient of the seven params,
//                                   blocks = ceil(N * K / 256)
#pragma once
#include "crf_tensor.h"

namespace fslic {

constexpr int kCrfParamCount = 7;             // the floats of fslic_crf_params
constexpr int kCrfParamGradBlock = 256;       // (frame, node) threads per block of k_crf_tensor_param_grad
inline size_t crf_tensor_param_grad_blocks(int N, int K) { return ((size_t)N * (size_t)K + kCrfParamGradBlock - 1) / kCrfParamGradBlock; }
inline size_t crf_tensor_param_grad_workspace(int N, int K) {
    return (crf_tensor_param_grad_blocks(N, K) * kCrfParamCount * sizeof(double) + 15) & ~(size_t)15;
}

// The transposed neighbour lists: for (frame, node) g the entries t_offsets[g] <= t < t_offsets[g + 1] name the neighbour entries
// t_entries[t] of the rows t_rows[t] whose target g is, in ascending entry order.
struct CrfTensorTransposed {
    const int64_t* offsets;     // [N * K + 1]
    const int32_t* entries;     // [nnz]
    const int32_t* rows;        // [nnz]
};

// What the adjoint kernels read: the prepared lists and the transposed ones.
struct CrfGradLists : CrfTensorLists {
    CrfTensorTransposed tr;
};

// The adjoint of the sweep q_in -> q_new.  grad_new: the gradient with respect to q_new (the first launch of a backward), or NULL:
// it is gathered from dm_in.  Writes dm_out, stores (first) or adds da to grad_unaries, and with slots != NULL stores or adds the
// block's part of the gradient of compat.
void launch_crf_tensor_sweep_bwd(const CrfTensorParams& dp, const CrfGradLists& lists, const int32_t* indices, const float* unaries,
                                 const float* compat, const float* q_in, const float* q_new, const float* grad_new, const float* dm_in,
                                 float* dm_out, float* grad_unaries, float* slots, float* msg, float* x, bool first, hipStream_t st);
// The last gather and the start of the chain.  grad_start: grad_q itself (no sweep ran) or NULL: gathered from dm_in.  With
// grad_q0 != NULL that is the gradient of q0; otherwise -q_start * it goes into grad_unaries (q_start = crf_expf(-unaries)).
// first: no sweep ran, grad_unaries is stored rather than added to.
void launch_crf_tensor_grad_close(const CrfTensorParams& dp, const CrfGradLists& lists, const float* q_start, const float* grad_start,
                                  const float* dm_in, float* grad_unaries, float* grad_q0, bool first, hipStream_t st);
// grad_compat[c] = the sum of slots[b][c] over the blocks in ascending order (blocks == 0: zero).
void launch_crf_tensor_grad_compat(const float* slots, size_t blocks, int C, float* grad_compat, hipStream_t st);
// The gradient of the energies from one sweep, behind its launch_crf_tensor_sweep_bwd: dm is what that launch left in dm_out, q_in
// the sweep's input iterate.  Adds to grad_edge [nnz] (live entries inside the clamped rows, each found through its position in the
// transposed lists) and to grad_links [N][2][K] (cells with a neighbouring frame, only with dp.temporal); either may be NULL.  The
// caller zeroes both before the first launch.
void launch_crf_tensor_energy_grad(const CrfTensorParams& dp, const CrfGradLists& lists, const int32_t* indices, const float* dm,
                                   const float* q_in, float* grad_edge, float* grad_links, hipStream_t st);
// The backward of launch_crf_tensor_energies: grad_params[7] from grad_edge [nnz] and grad_links [N][2][K] (either may be NULL: zero)
// and the params in device memory; slots is the workspace above.  Nothing flows to yxrgb.
void launch_crf_tensor_param_grad(const CrfTensorParams& dp, const float* params, const float* yxrgb, const int64_t* offsets,
                                  const int32_t* indices, const float* grad_edge, const float* grad_links, double* slots,
                                  float* grad_params, hipStream_t st);

}  // namespace fslic
