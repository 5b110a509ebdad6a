// crf_tensor.hip -- SimpleCRF inference (src/simple-crf.cpp:62-153) on device tensors the caller owns (crf_tensor.h; the C ABI is in
// crfapi.cpp).  The arithmetic is crf.hip's, operation by operation; the layout of the sweep is not.
//   k_crf_tensor_start  the starting q: q0, or crf_expf(-unaries) (SimpleCRF::initialize).
//   k_crf_tensor_edges  once per call, one thread per (frame, node): the row's bounds clamped into [0, nnz] and to non-decreasing,
//                       per neighbour entry the spatial energy and the member factor (an index outside [0, K) makes the entry dead),
//                       per node the temporal energies and factors towards t-1 and t+1.  Clusters are built in registers from the
//                       channel-first yxrgb planes and the member counts.  Two more forms of the same body write the energies alone
//                       to caller tensors from params in device memory, and take the energies from caller tensors.
//   k_crf_tensor_sweep  one Jacobi sweep.  A block is 64 consecutive nodes of one frame (the lanes) times one wavefront per class
//                       slice (wave v does classes v, v + waves, ...), so every [N][C][K] plane is read and written coalesced.
//                       Messages of (node, class) -> LDS [C][64]; barrier; the compatibility sum of (node, class) over the other
//                       classes from LDS and its crf_expf -> LDS [C][64]; barrier; every thread adds its node's C exponentials in
//                       ascending order itself (C LDS reads, no third barrier) and divides its own.  Above kCrfTensorLdsClasses
//                       classes the messages go to a plane of the workspace and the exponentials to q_out, with one more barrier
//                       between the sums and the in-place division.
// Every grid is exact (one trip): blocks of 256 over N * C * K (start) and N * K (edges), N * ceil(K / 64) blocks (sweep); all of
// them are below 2^31 because N * C * K and N * K are.
#include "crf_tensor_sweep.h"

// The roundings are crf.hip's (see there and crf.h): products fused exactly where the reference build fuses them, nothing else.
#pragma clang fp contract(off)

namespace fslic {

__global__ __launch_bounds__(256) void k_crf_tensor_start(const float* __restrict__ unaries, const float* __restrict__ q0,
                                                          float* __restrict__ out, size_t n) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    out[p] = q0 ? q0[p] : crf_expf(-unaries[p]);
}

// The Cluster of node i from a frame's planes: y, x, r, g, b of yxrgb[5][K] and the 32 bits of members[K].
static __device__ __forceinline__ fslic_cluster crf_tensor_cluster(const float* __restrict__ planes, const int32_t* __restrict__ members,
                                                                   size_t K, int i) {
    fslic_cluster c = {};
    c.y = planes[i];
    c.x = planes[K + i];
    c.r = planes[2 * K + i];
    c.g = planes[3 * K + i];
    c.b = planes[4 * K + i];
    c.num_members = (uint32_t)members[i];
    return c;
}

// The three forms of the edge pass share this body, so their arithmetic cannot drift apart:
//   kCrfEdgesHost    the params of dp.p -> rows, edge (energy, factor), temporal (energy, factor twice): what a call with host params runs;
//   kCrfEdgesOut     the seven params from device memory (io.params) -> io.edge_out[nnz] and io.links_out[N][2][K]: the energies
//                    alone, 0.0 for a self-loop, for a dead entry, at the window's ends and without temporal links (entries outside
//                    every clamped row are not touched: the caller zeroes edge_out first);
//   kCrfEdgesGiven   the energies from io.edge_in / io.links_in (NULL: no links) -> rows, edge, temporal with the member factors and the
//                    dead flags computed here; yxrgb is not read.  A self-loop keeps the energy it was given.
template <int MODE>
__global__ __launch_bounds__(256) void k_crf_tensor_edges(CrfTensorParams dp, const float* __restrict__ yxrgb, const int32_t* __restrict__ members,
                                                          const int64_t* __restrict__ offsets, const int32_t* __restrict__ idx,
                                                          uint2* __restrict__ rows, float2* __restrict__ edge, float4* __restrict__ temporal,
                                                          CrfEdgeTensors io) {
    const int n = dp.N * dp.K;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int K = dp.K;
    const int w = g / K, i = g - w * K;
    fslic_crf_params p = dp.p;
    if (MODE == kCrfEdgesOut) {                        // in the order of fslic_crf_params
        p.spatial_w = io.params[0]; p.temporal_w = io.params[1]; p.spatial_srgb = io.params[2]; p.temporal_srgb = io.params[3];
        p.spatial_sxy = io.params[4]; p.spatial_smooth_w = io.params[5]; p.spatial_smooth_sxy = io.params[6];
    }
    const float* planes = MODE == kCrfEdgesGiven ? nullptr : yxrgb + (size_t)w * 5 * K;
    const int32_t* mem = members + (size_t)w * K;
    // the Cluster of node `node` of the frame `frames` away; without yxrgb only its member count
    const auto cluster = [&](int frames, int node) {
        if (MODE != kCrfEdgesGiven) return crf_tensor_cluster(planes + (ptrdiff_t)frames * 5 * K, mem + (ptrdiff_t)frames * K, K, node);
        fslic_cluster c = {};
        c.num_members = (uint32_t)mem[(ptrdiff_t)frames * K + node];
        return c;
    };
    const fslic_cluster ci = cluster(0, i);
    // idx[k] and edge[k] are touched for r.x <= k < r.y only, here and in the sweep
    const uint2 r = crf_clamped_bounds(offsets, (size_t)g, dp.nnz);
    if (MODE != kCrfEdgesOut) rows[g] = r;
    for (uint32_t k = r.x; k < r.y; ++k) {
        const int32_t j = idx[k];
        if ((uint32_t)j >= (uint32_t)K) {              // contributes nothing, as pooling treats a label outside [0, K)
            if (MODE == kCrfEdgesOut) io.edge_out[k] = 0.0f;
            else edge[k] = make_float2(0.0f, kCrfDeadEntry);
            continue;
        }
        const fslic_cluster cj = cluster(0, j);
        // calc_spatial_pairwise_energy(neighbor, i) (simple-crf.cpp:86): 0 for a self-loop
        const float e = MODE == kCrfEdgesGiven ? io.edge_in[k] : (j == i ? 0.0f : crf_spatial_energy(p, cj, ci));
        if (MODE == kCrfEdgesOut) io.edge_out[k] = e;
        else edge[k] = make_float2(e, crf_member_factor(cj.num_members, ci.num_members));
    }
    const bool given = MODE == kCrfEdgesGiven && io.links_in;
    const size_t link = ((size_t)w * 2) * K + i;       // links[w][0][i]; [w][1][i] is K further
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (dp.temporal && w > 0) {                        // simple-crf.cpp:90-93
        const fslic_cluster cp = cluster(-1, i);
        t.x = MODE == kCrfEdgesGiven ? (given ? io.links_in[link] : 0.0f) : crf_temporal_energy(p, ci, cp);
        t.y = crf_member_factor(cp.num_members, ci.num_members);
    }
    if (dp.temporal && w < dp.N - 1) {                 // :95-99
        const fslic_cluster cn = cluster(1, i);
        t.z = MODE == kCrfEdgesGiven ? (given ? io.links_in[link + K] : 0.0f) : crf_temporal_energy(p, ci, cn);
        t.w = crf_member_factor(cn.num_members, ci.num_members);
    }
    if (MODE == kCrfEdgesOut) {
        io.links_out[link] = t.x;
        io.links_out[link + K] = t.z;
    } else {
        temporal[g] = t;
    }
}

// The second plane holds the exponentials: LDS, or q_out itself above kCrfTensorLdsClasses classes (crf_tensor_sweep.h).
template <bool LDS>
__global__ __launch_bounds__(kCrfTensorNodes * kCrfTensorWaves) void k_crf_tensor_sweep(
        CrfTensorParams dp, CrfTensorLists L, const int32_t* __restrict__ idx, const float* __restrict__ unary,
        const float* __restrict__ compat, const float* __restrict__ q_in, float* q_out, float* msg) {
    extern __shared__ float s_crf[];
    const int C = dp.C, K = dp.K;
    const CrfSweepThread t = crf_sweep_thread<LDS>(dp, s_crf, msg, q_out);

    if (t.live) {
        const uint2 r = L.rows[(size_t)t.w * K + t.i];
        const float4 tl = L.temporal[(size_t)t.w * K + t.i];
        for (int cls = t.wave; cls < C; cls += t.waves) t.m[cls * t.stride] = crf_sweep_message(t, K, r, tl, idx, L.edge, q_in, cls);
    }
    __syncthreads();
    if (t.live)
        for (int cls = t.wave; cls < C; cls += t.waves) t.x[cls * t.stride] = crf_sweep_exp(t, C, K, compat, unary, cls);
    __syncthreads();
    float sum = 0.0f;
    if (t.live) {
        sum = crf_sweep_class_sum(t, C);
        if (crf_sweep_clamps(sum)) sum = (float)1e-5;
    }
    if (!LDS) __syncthreads();                                                 // x is q_out: every sum is taken before a division lands
    if (t.live)
        for (int cls = t.wave; cls < C; cls += t.waves) q_out[t.base + (size_t)cls * K + t.i] = t.x[cls * t.stride] / sum;
}

void launch_crf_tensor_start(const float* unaries, const float* q0, float* out, size_t n, hipStream_t st) {
    launch(k_crf_tensor_start, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, unaries, q0, out, n);
}

void launch_crf_tensor_edges(const CrfTensorParams& dp, const float* yxrgb, const int32_t* members, const int64_t* offsets,
                             const int32_t* indices, uint2* rows, float2* edge, float4* temporal, hipStream_t st) {
    const unsigned n = (unsigned)dp.N * (unsigned)dp.K;
    launch(k_crf_tensor_edges<kCrfEdgesHost>, dim3((n + 255) / 256), dim3(256), 0, st, dp, yxrgb, members, offsets, indices, rows, edge,
           temporal, CrfEdgeTensors{});
}

void launch_crf_tensor_energies(const CrfTensorParams& dp, const float* params, const float* yxrgb, const int32_t* members,
                                const int64_t* offsets, const int32_t* indices, float* edge_out, float* links_out, hipStream_t st) {
    const unsigned n = (unsigned)dp.N * (unsigned)dp.K;
    CrfEdgeTensors io = {};
    io.params = params; io.edge_out = edge_out; io.links_out = links_out;
    launch(k_crf_tensor_edges<kCrfEdgesOut>, dim3((n + 255) / 256), dim3(256), 0, st, dp, yxrgb, members, offsets, indices,
           (uint2*)nullptr, (float2*)nullptr, (float4*)nullptr, io);
}

void launch_crf_tensor_edges_given(const CrfTensorParams& dp, const float* edge_in, const float* links_in, const int32_t* members,
                                   const int64_t* offsets, const int32_t* indices, uint2* rows, float2* edge, float4* temporal,
                                   hipStream_t st) {
    const unsigned n = (unsigned)dp.N * (unsigned)dp.K;
    CrfEdgeTensors io = {};
    io.edge_in = edge_in; io.links_in = links_in;
    launch(k_crf_tensor_edges<kCrfEdgesGiven>, dim3((n + 255) / 256), dim3(256), 0, st, dp, (const float*)nullptr, members, offsets, indices,
           rows, edge, temporal, io);
}

void launch_crf_tensor_sweep(const CrfTensorParams& dp, const CrfTensorLists& lists, const int32_t* indices, const float* unaries,
                             const float* compat, const float* q_in, float* q_out, float* msg, hipStream_t st) {
    const CrfSweepShape sh = crf_tensor_sweep_shape(dp.N, dp.C, dp.K);
    launch(sh.lds ? k_crf_tensor_sweep<true> : k_crf_tensor_sweep<false>, dim3(sh.grid), dim3(sh.block), sh.lds, st, dp, lists, indices,
           unaries, compat, q_in, q_out, msg);
}

}  // namespace fslic
