// crf.h -- SimpleCRF (src/simple-crf.{h,hpp,cpp}): mean-field inference of a Potts CRF over the superpixel graph, spatial edges
// inside a frame and temporal edges between consecutive frames.  Internal to the library; the public boundary is the fslic_hip_crf_*
// part of include/fslic_hip.h (wrappers in capi.cpp), the device side of inference() is in crf.hip.  Its kernels are the tensor
// CRF's edge pass and sweep (crf_tensor.h, crf_tensor.hip): one copy of the mean-field arithmetic serves both surfaces.
//
// Frame data lives on the host (clusters, neighbour lists, unaries, and q until the first inference): every getter and setter is a
// host operation and a CRF can be built and filled without a GPU.  inference() uploads what changed since the last call (per-frame
// dirty flags) into a window of device slices, one per frame in time order, and leaves q on the device; the host copy of a frame's q
// is refreshed the next time it is read.
//
// Bit-exactness with the reference build (setup.py: g++ -O2 -std=c++11 -mavx2 -mfma).  For C++, -std=c++11 does NOT switch GCC's
// contraction off (only the ISO C modes do), so that build fuses products into sums where GCC's widening_mul pass finds them: the
// energies, the message terms and the compatibility sum below write each of those fusions out with __builtin_fmaf (read off the
// reference's object code, simple_crf_frame_spatial_pairwise_energy and SimpleCRF::infer_once) and every other operation unfused:
// every function here opens with `#pragma clang fp contract(off)` and crf.hip is compiled with -ffp-contract=off.  The operand
// order is the reference's and the exponential is crf_expf, a copy of the host libm's expf.
#pragma once
#include "engine_internal.h"

#include <cmath>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <vector>

namespace fslic {

// ---- crf_expf: glibc's expf, bit for bit ----------------------------------------------------------------------------------------
// The reference calls expf from glibc (2.28 and later: sysdeps/ieee754/flt-32/e_expf.c, 2^(k/32) table + cubic in double precision;
// on x86_64 with FMA the ifunc picks the build of that file compiled with -mfma, __expf_fma, whose compiler fused the five products
// written below with __builtin_fma).  It is NOT correctly rounded: (float)exp((double)x) differs from it on 170 648 finite inputs.
// The same expressions in double precision reproduce it on all 2^32 inputs (scripts/crf_expf_sweep.py).  The
// build of that file without FMA (a CPU without FMA) differs from this one on two inputs, 0xc27c65d9 and 0x4202422f (1 ulp each).
struct CrfExpTable { uint64_t t[32]; };
__host__ __device__ inline float crf_expf(float x) {
#pragma clang fp contract(off)
    // tab[i] = bits(2^(i/32)) - (i << 47)   (__exp2f_data.tab)
    constexpr CrfExpTable T = {{
        0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
        0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
        0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
        0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
        0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
        0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
        0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
        0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull}};
    constexpr double kInvLn2N = 0x1.71547652b82fep+5, kShift = 0x1.8p+52;
    constexpr double kC0 = 0x1.c6af84b912394p-20, kC1 = 0x1.ebfce50fac4f3p-13, kC2 = 0x1.62e42ff0c52d6p-6;
    uint32_t ux;
    memcpy(&ux, &x, 4);
    const uint32_t abstop = (ux >> 20) & 0x7ffu;
    if (abstop >= 0x42bu) {                              // |x| >= 88 or NaN
        if (ux == 0xff800000u) return 0.0f;
        if (abstop >= 0x7f8u) return x + x;              // +inf, NaN (quietened)
        if (x > 0x1.62e42ep6f) return INFINITY;          // overflow
        if (x < -0x1.9fe368p6f) return 0.0f;             // underflow
    }
    const double xd = (double)x;
    double kd = __builtin_fma(kInvLn2N, xd, kShift);     // z + SHIFT, z = InvLn2N * xd fused
    uint64_t ki;
    memcpy(&ki, &kd, 8);
    kd -= kShift;
    const double r = __builtin_fma(kInvLn2N, xd, -kd);   // z - kd
    const double z = __builtin_fma(kC0, r, kC1);
    const double r2 = r * r;
    double y = __builtin_fma(kC2, r, 1.0);
    y = __builtin_fma(z, r2, y);
    uint64_t t = T.t[ki % 32];
    t += ki << 47;
    double s;
    memcpy(&s, &t, 8);
    return (float)(y * s);
}

__host__ __device__ inline float crf_fmaf(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// ---- pairwise energies (src/simple-crf.hpp:135-175) -----------------------------------------------------------------------------
// The sum of the three squared colour terms as the reference build evaluates -(R^2 + G^2 + B^2): -fma(B, B, fma(R, R, G * G)).
__host__ __device__ inline float crf_neg_sq3(float R, float G, float B) {
#pragma clang fp contract(off)
    return -__builtin_fmaf(B, B, __builtin_fmaf(R, R, G * G));
}
// -(X^2 + Y^2): -fma(X, X, Y * Y).
__host__ __device__ inline float crf_neg_sq2(float X, float Y) {
#pragma clang fp contract(off)
    return -__builtin_fmaf(X, X, Y * Y);
}
// calc_temporal_pairwise_energy(node, other) with `c1` = this frame's cluster, `c2` = the other frame's (hpp:135-147).
__host__ __device__ inline float crf_temporal_energy(const fslic_crf_params& p, const fslic_cluster& c1, const fslic_cluster& c2) {
#pragma clang fp contract(off)
    const float stdev = p.temporal_srgb, weight = p.temporal_w;
    const float exponent = crf_neg_sq3((c1.r - c2.r) / stdev, (c1.g - c2.g) / stdev, (c1.b - c2.b) / stdev) * 0.5f;   // (/ 2.0f)
    return weight * crf_expf(exponent);
}
// calc_spatial_pairwise_energy(node_i, node_j) with c1 = clusters[node_i], c2 = clusters[node_j], node_i != node_j (hpp:149-175):
// exponent = rgb / 2 + xy / 2 as fma(rgb, 0.5, xy * 0.5), the result as fma(weight, expf(exponent), smooth_weight * expf(smooth)).
__host__ __device__ inline float crf_spatial_energy(const fslic_crf_params& p, const fslic_cluster& c1, const fslic_cluster& c2) {
#pragma clang fp contract(off)
    const float stdev = p.spatial_srgb, weight = p.spatial_w, sxy = p.spatial_sxy;
    const float smooth_weight = p.spatial_smooth_w, smooth_sxy = p.spatial_smooth_sxy;
    const float rgb = crf_neg_sq3((c1.r - c2.r) / stdev, (c1.g - c2.g) / stdev, (c1.b - c2.b) / stdev);
    const float xy = crf_neg_sq2((c1.x - c2.x) / sxy, (c1.y - c2.y) / sxy);
    const float exponent = __builtin_fmaf(rgb, 0.5f, xy * 0.5f);
    const float smooth_exponent = crf_neg_sq2((c1.x - c2.x) / smooth_sxy, (c1.y - c2.y) / smooth_sxy) * 0.5f;
    return __builtin_fmaf(weight, crf_expf(exponent), smooth_weight * crf_expf(smooth_exponent));
}
// The factor of a message from a node with `m_from` members to one with `m_to` (simple-crf.cpp:78-81, 88, 92, 97):
// sqrtf((float)num_members_from / num_members_to), the receiver's count read as int and taken as 1 when <= 0.
__host__ __device__ inline float crf_member_factor(uint32_t m_from, uint32_t m_to) {
    int n = (int)m_to;
    if (n <= 0) n = 1;
    return sqrtf((float)m_from / (float)n);
}

// ---- the clusters as the tensor kernels read them (crf_tensor.h) ------------------------------------------------------------------
// A window of T frames is 6 * T * K words: the planes yxrgb [T][5][K] float32, then members [T][K] int32 holding the 32 bits of
// num_members.  This writes frame `w` of it from the frame's K clusters; host only, no device involved.
inline void crf_stage_clusters(const fslic_cluster* cl, size_t w, size_t T, size_t K, float* window) {
    float* planes = window + w * 5 * K;
    float* members = window + T * 5 * K + w * K;
    for (size_t i = 0; i < K; i++) {
        planes[i] = cl[i].y;
        planes[K + i] = cl[i].x;
        planes[2 * K + i] = cl[i].r;
        planes[3 * K + i] = cl[i].g;
        planes[4 * K + i] = cl[i].b;
        memcpy(members + i, &cl[i].num_members, 4);
    }
}

}  // namespace fslic

// ---- host state -----------------------------------------------------------------------------------------------------------------
struct fslic_crf;
struct fslic_crf_frame {                    // SimpleCRFFrame (src/simple-crf.hpp:14-67)
    fslic_crf* parent = nullptr;
    int time = 0;
    std::vector<fslic_cluster> clusters;
    std::vector<std::vector<uint32_t>> edges;
    std::vector<float> unaries;
    std::vector<float> q;                   // [num_classes][num_nodes]
    // device bookkeeping (guarded by the parent's mutex)
    int dev_pos = -1;                       // window position whose device slices hold this frame (-1: none)
    bool dirty_graph = true;                // clusters / edges changed since the last upload
    bool dirty_unary = true;
    bool dirty_q = true;                    // the host's q is newer than the device's
    bool q_on_device = false;               // the device's q is newer than the host's (after inference)
};

struct fslic_crf {                          // SimpleCRF (src/simple-crf.hpp:70-126)
    size_t C = 0, K = 0;
    int next_time = 0;
    std::deque<std::unique_ptr<fslic_crf_frame>> frames;     // consecutive times, oldest first
    std::vector<float> compat;
    fslic_crf_params params{};
    std::mutex mu;                          // every entry point holds it for its duration
    // device state: the window of the last inference, bound to one engine
    fslic_engine* eng = nullptr;
    int capT = 0;                           // frames the buffers are sized for
    long long nnz = 0;                      // neighbour entries of the window as uploaded
    fslic::Device<float> d_q[2];                // [capT][C][K] each, d_q[cur] holds the current q
    int cur = 0;
    fslic::Device<float> d_unary;
    fslic::Device<float> d_compat;
    fslic::Device<float> d_cl;                  // [6 * capT * K]: the uploaded frames' yxrgb planes, then their member counts (crf_stage_clusters)
    fslic::Device<int64_t> d_offsets;           // [capT * K + 1]: the neighbour lists of the window as one CSR over (frame, node)
    fslic::Device<int32_t> d_idx;               // [nnz]
    fslic::Device<char> d_work;                 // rows, temporal, edge and msg: crf_tensor_workspace(T, C, K, nnz, kCrfCallSaved, false)
    bool graph_uploaded = false;
};

namespace fslic {
// crf.hip.  All with the CRF's mutex held.
int crf_inference(fslic_crf* crf, fslic_engine* e, size_t max_iter);
int crf_pull_q(fslic_crf* crf, fslic_crf_frame* f);       // refresh the host's q of `f` from the device when the device's is newer
void crf_release_device(fslic_crf* crf);                  // free the device state (the host's q must have been pulled first)
int crf_expf_device(fslic_engine* e, const float* in, float* out, size_t n);
}  // namespace fslic
