// crf_tensor.h -- SimpleCRF inference on device tensors the caller owns, and its backward (crf_tensor.hip, crf_tensor_grad.hip,
// crfapi.cpp).  Internal to the library.
//
// Workspace of one call (crf_tensor_workspace; offsets from its start, every part 16-byte aligned, a part a call does not use empty):
//   rows[N * K]          uint2   -- the row bounds of (frame, node) after clamping: 0 <= x <= y <= nnz
//   temporal[N * K]      float4  -- (energy, factor) towards t - 1 and t + 1; zero when temporal is off or at the window's ends
//   edge[nnz]            float2  -- per neighbour entry (energy, factor); factor kCrfDeadEntry: the index is outside [0, K)
//   q[N * C * K]         float   -- kCrfCallPlain alone: the second buffer of the ping-pong (the first is q_out)
//   msg[N * C * K]       float   -- the messages, only for C > kCrfTensorLdsClasses
// and for kCrfCallBackward alone:
//   dm[2][N * C * K]     float   -- the gradient with respect to the messages, ping-pong: sweep `it` writes dm[it & 1] and gathers
//                                   from dm[(it + 1) & 1]
//   x[N * C * K]         float   -- exponentials, then G' q', then da, only for C > kCrfTensorLdsClasses
//   slots[blocks][C]     float   -- per block of the sweep its part of the gradient of compat, blocks = N * ceil(K / 64); only
//                                   when that gradient is asked for
// With given energies (fslic_hip_crf_tensor_*_energies) the layout is the same: rows, temporal and edge are filled from the caller's
// edge [nnz] and links [N][2][K] with the member factors and dead flags computed on the device; the gradients of the energies go to
// caller tensors and need no part of their own.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "../../include/fslic_hip.h"

namespace fslic {

constexpr int kCrfTensorNodes = 64;           // nodes per block of the sweep: the lanes of a wavefront
constexpr int kCrfTensorWaves = 16;           // at most this many wavefronts (class slices) per block
// Messages and exponentials of up to this many classes stay in LDS: 2 x 256 B per class, 64 KB per block (what a kernel may take
// without raising hipFuncAttributeMaxDynamicSharedMemorySize).  Above it the messages go to msg and the exponentials to q_out.
constexpr int kCrfTensorLdsClasses = 128;
constexpr float kCrfDeadEntry = -1.0f;        // no factor is negative (a square root)

struct CrfTensorParams {
    int N, C, K, temporal;
    long long nnz;
    fslic_crf_params p;
};

// The forms of the edge pass (k_crf_tensor_edges) and the caller tensors of the two that have some.
enum { kCrfEdgesHost = 0, kCrfEdgesOut = 1, kCrfEdgesGiven = 2 };
struct CrfEdgeTensors {
    const float* params;        // kCrfEdgesOut: the seven params in the order of fslic_crf_params, device memory
    float* edge_out;            //               [nnz]
    float* links_out;           //               [N][2][K]: towards n - 1, towards n + 1
    const float* edge_in;       // kCrfEdgesGiven: [nnz]
    const float* links_in;      //                 [N][2][K], or NULL: no temporal energy
};

// What the edge pass prepares for the sweeps of a call: the first three parts of the workspace.
struct CrfTensorLists {
    const uint2* rows;
    const float2* edge;
    const float4* temporal;
};

// The launch shape of a sweep and of its adjoint: a block is 64 consecutive nodes of one frame times the fewest equal class slices
// that fit kCrfTensorWaves wavefronts (21 classes -> 11 waves of 2 classes, the last of 1); both planes of a block in LDS up to
// kCrfTensorLdsClasses classes.
struct CrfSweepShape {
    unsigned grid, block, lds;
};
inline CrfSweepShape crf_tensor_sweep_shape(int N, int C, int K) {
    const int per = (C + kCrfTensorWaves - 1) / kCrfTensorWaves, waves = (C + per - 1) / per;
    return {(unsigned)N * (unsigned)((K + kCrfTensorNodes - 1) / kCrfTensorNodes), (unsigned)(kCrfTensorNodes * waves),
            C <= kCrfTensorLdsClasses ? (unsigned)(2 * sizeof(float) * kCrfTensorNodes * C) : 0u};
}

// The three calls that take a workspace: fslic_hip_crf_tensor_inference, _inference_saved and _backward (and their _energies forms).
enum CrfTensorCall { kCrfCallPlain, kCrfCallSaved, kCrfCallBackward };
struct CrfTensorWorkspace {
    size_t rows, temporal, edge, q, msg, dm, x, slots, bytes;
};
inline CrfTensorWorkspace crf_tensor_workspace(int N, int C, int K, long long nnz, CrfTensorCall call, bool with_compat) {
    const auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t n = (size_t)N * (size_t)K, cells = n * (size_t)C;
    const size_t plane = C > kCrfTensorLdsClasses ? up(cells * sizeof(float)) : 0;
    const bool backward = call == kCrfCallBackward;
    CrfTensorWorkspace w;
    w.rows = 0;
    w.temporal = w.rows + up(n * sizeof(uint2));
    w.edge = w.temporal + up(n * sizeof(float4));
    w.q = w.edge + up((size_t)nnz * sizeof(float2));
    w.msg = w.q + (call == kCrfCallPlain ? up(cells * sizeof(float)) : 0);
    w.dm = w.msg + plane;
    w.x = w.dm + (backward ? up(2 * cells * sizeof(float)) : 0);
    w.slots = w.x + (backward ? plane : 0);
    w.bytes = w.slots + (backward && with_compat ? up((size_t)crf_tensor_sweep_shape(N, C, K).grid * (size_t)C * sizeof(float)) : 0);
    return w;
}

// The parts of a workspace as pointers.
struct CrfTensorBuffers {
    uint2* rows;
    float4* temporal;
    float2* edge;
    float *q, *msg, *dm, *x, *slots;
    CrfTensorLists lists() const { return {rows, edge, temporal}; }
};
inline CrfTensorBuffers crf_tensor_buffers(void* workspace, const CrfTensorWorkspace& w) {
    char* base = reinterpret_cast<char*>(workspace);
    const auto at = [base](size_t off) { return reinterpret_cast<float*>(base + off); };
    return {reinterpret_cast<uint2*>(base + w.rows), reinterpret_cast<float4*>(base + w.temporal),
            reinterpret_cast<float2*>(base + w.edge), at(w.q), at(w.msg), at(w.dm), at(w.x), at(w.slots)};
}

// The starting q: q0 when it is given, crf_expf(-unaries) otherwise.
void launch_crf_tensor_start(const float* unaries, const float* q0, float* out, size_t n, hipStream_t st);
void launch_crf_tensor_edges(const CrfTensorParams& dp, const float* yxrgb, const int32_t* members, const int64_t* offsets,
                             const int32_t* indices, uint2* rows, float2* edge, float4* temporal, hipStream_t st);
// The energies alone, from params in device memory: edge_out[k] for the entries inside the clamped rows (the caller zeroes the rest),
// every cell of links_out.  dp.p is not read.
void launch_crf_tensor_energies(const CrfTensorParams& dp, const float* params, const float* yxrgb, const int32_t* members,
                                const int64_t* offsets, const int32_t* indices, float* edge_out, float* links_out, hipStream_t st);
// launch_crf_tensor_edges with the energies taken from edge_in [nnz] and links_in [N][2][K] (NULL: none).  dp.p is not read.
void launch_crf_tensor_edges_given(const CrfTensorParams& dp, const float* edge_in, const float* links_in, const int32_t* members,
                                   const int64_t* offsets, const int32_t* indices, uint2* rows, float2* edge, float4* temporal,
                                   hipStream_t st);
void launch_crf_tensor_sweep(const CrfTensorParams& dp, const CrfTensorLists& lists, const int32_t* indices, const float* unaries,
                             const float* compat, const float* q_in, float* q_out, float* msg, hipStream_t st);

}  // namespace fslic
