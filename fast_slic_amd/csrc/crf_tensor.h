// crf_tensor.h -- SimpleCRF inference on device tensors the caller owns (crf_tensor.hip, crfapi.cpp).  Internal to the library.
//
// Workspace of one fslic_hip_crf_tensor_inference call (offsets from its start, every part 16-byte aligned):
//   rows[N * K]     uint2   -- the row bounds of (frame, node) after clamping: 0 <= x <= y <= nnz
//   temporal[N * K] float4  -- (energy, factor) towards t - 1 and t + 1; zero when temporal is off or at the window's ends
//   edge[nnz]       float2  -- per neighbour entry (energy, factor); factor kCrfDeadEntry: the index is outside [0, K)
//   q[N * C * K]    float   -- the second buffer of the ping-pong (the first is q_out)
//   msg[N * C * K]  float   -- the messages, only for C > kCrfTensorLdsClasses
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

struct CrfTensorWorkspace {
    size_t rows, temporal, edge, q, msg, bytes;
};
inline CrfTensorWorkspace crf_tensor_workspace(int N, int C, int K, long long nnz) {
    const auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t n = (size_t)N * (size_t)K, cells = n * (size_t)C;
    CrfTensorWorkspace w;
    w.rows = 0;
    w.temporal = w.rows + up(n * sizeof(uint2));
    w.edge = w.temporal + up(n * sizeof(float4));
    w.q = w.edge + up((size_t)nnz * sizeof(float2));
    w.msg = w.q + up(cells * sizeof(float));
    w.bytes = w.msg + (C > kCrfTensorLdsClasses ? up(cells * sizeof(float)) : 0);
    return w;
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
void launch_crf_tensor_sweep(const CrfTensorParams& dp, const uint2* rows, const int32_t* indices, const float2* edge,
                             const float4* temporal, const float* unaries, const float* compat, const float* q_in, float* q_out,
                             float* msg, hipStream_t st);

}  // namespace fslic
