// crf.hip -- SimpleCRF inference (src/simple-crf.cpp:62-153) on gfx950, and the device side of its host state (crf.h).
//   k_crf_edges      once per inference(), every frame: per neighbour entry the spatial energy and the member factor, per node the
//                    temporal energies and factors towards t-1 and t+1.  None of them depends on the class or the iteration.
//   k_crf_iteration  one Jacobi sweep of SimpleCRF::infer_once over every frame: reads q of the previous sweep, writes the other buffer
//                    (the reference's new_probas).  One thread per (frame, node) does all its classes: messages (kept in LDS), the
//                    compatibility transform, the exponential, the clamp at 1e-5 and the normalisation, each sum in the reference's order.
// max_iter sweeps go back to back on one slot's stream; one synchronisation at the end.
#include "crf.h"

#include <algorithm>

// Every rounding of this file is the reference build's: a product is fused into a sum exactly where that build fuses it (__builtin_fmaf,
// see crf.h) and nowhere else (see realdist.hip for what hipcc's default would do), division and sqrtf are the correctly rounded ones
// (HIP's default), the exponential is crf_expf.
#pragma clang fp contract(off)

namespace fslic {

constexpr int kCrfBlock = 64;                          // nodes per block: one wavefront
constexpr int kCrfLdsClasses = 256;                    // messages of up to this many classes stay in LDS (64 KB per block)

__global__ __launch_bounds__(256) void k_crf_edges(CrfDevParams dp, const fslic_cluster* __restrict__ cl, const uint32_t* __restrict__ rowptr,
                                                   const uint32_t* __restrict__ idx, float2* __restrict__ edge, float4* __restrict__ temporal) {
    const int n = dp.T * dp.K;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const int w = g / dp.K, i = g - w * dp.K;
    const fslic_cluster ci = cl[g];
    const fslic_cluster* frame = cl + (size_t)w * dp.K;
    for (uint32_t k = rowptr[g], k1 = rowptr[g + 1]; k < k1; ++k) {
        const uint32_t j = idx[k];
        const fslic_cluster cj = frame[j];
        // calc_spatial_pairwise_energy(neighbor, i) (simple-crf.cpp:86): 0 for a self-loop
        const float e = (int)j == i ? 0.0f : crf_spatial_energy(dp.p, cj, ci);
        edge[k] = make_float2(e, crf_member_factor(cj.num_members, ci.num_members));
    }
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (w > 0) {                                       // simple-crf.cpp:90-93
        const fslic_cluster cp = cl[g - dp.K];
        t.x = crf_temporal_energy(dp.p, ci, cp);
        t.y = crf_member_factor(cp.num_members, ci.num_members);
    }
    if (w < dp.T - 1) {                                // :95-99
        const fslic_cluster cn = cl[g + dp.K];
        t.z = crf_temporal_energy(dp.p, ci, cn);
        t.w = crf_member_factor(cn.num_members, ci.num_members);
    }
    temporal[g] = t;
}

// Messages of the thread's node: m[cls * mstride] (LDS, or the global scratch for more than kCrfLdsClasses classes).
template <bool LDS>
__global__ __launch_bounds__(kCrfBlock) void k_crf_iteration(CrfDevParams dp, const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ idx,
                                                             const float2* __restrict__ edge, const float4* __restrict__ temporal,
                                                             const float* __restrict__ unary, const float* __restrict__ compat,
                                                             const float* __restrict__ q_in, float* __restrict__ q_out, float* __restrict__ scratch) {
    extern __shared__ float s_msg[];
    const int n = dp.T * dp.K;
    const int g = blockIdx.x * kCrfBlock + threadIdx.x;
    if (g >= n) return;
    const int C = dp.C, K = dp.K;
    const int w = g / K, i = g - w * K;
    const size_t CK = (size_t)C * K;
    const size_t base = (size_t)w * CK;
    float* m = LDS ? s_msg + threadIdx.x : scratch + g;
    const size_t mstride = LDS ? (size_t)kCrfBlock : (size_t)n;
    const uint32_t k0 = rowptr[g], k1 = rowptr[g + 1];
    const float4 t = temporal[g];
    const bool has_prev = w > 0, has_next = w < dp.T - 1;
    // message passing (simple-crf.cpp:71-102): neighbours in list order, then t-1, then t+1; each term fma(e * q, factor, message)
    for (int cls = 0; cls < C; ++cls) {
        const float* qc = q_in + base + (size_t)cls * K;
        float message = 0.0f;
        for (uint32_t k = k0; k < k1; ++k) {
            const float2 es = edge[k];
            message = __builtin_fmaf(es.x * qc[idx[k]], es.y, message);
        }
        if (has_prev) message = __builtin_fmaf(t.x * qc[i - (ptrdiff_t)CK], t.y, message);
        if (has_next) message = __builtin_fmaf(t.z * qc[i + CK], t.w, message);
        m[cls * mstride] = message;
    }
    // compatibility transform (:104-114): the Potts sum over the other classes in ascending order (fused), then expf
    float* out = q_out + base + i;
    const float* un = unary + base + i;
    float sum = 0.0f;
    for (int cls = 0; cls < C; ++cls) {
        float gathered = 0.0f;
        for (int o = 0; o < C; ++o) {
            if (o == cls) continue;
            gathered = __builtin_fmaf(compat[o], m[o * mstride], gathered);
        }
        const float ex = crf_expf(-(un[(size_t)cls * K] + gathered));
        out[(size_t)cls * K] = ex;
    }
    // normalisation (:116-133): the sum over classes in ascending order, clamped at 1e-5 (a double comparison, as written there)
    for (int cls = 0; cls < C; ++cls) sum += out[(size_t)cls * K];
    if ((double)sum < 1e-5) sum = (float)1e-5;
    for (int cls = 0; cls < C; ++cls) out[(size_t)cls * K] = out[(size_t)cls * K] / sum;
}

__global__ __launch_bounds__(256) void k_crf_expf(const float* __restrict__ in, float* __restrict__ out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) out[p] = crf_expf(in[p]);
}

bool crf_messages_in_lds(int C) { return C <= kCrfLdsClasses; }

void launch_crf_edges(const CrfDevParams& dp, const fslic_cluster* cl, const uint32_t* rowptr, const uint32_t* idx, float2* edge,
                      float4* temporal, hipStream_t st) {
    const int n = dp.T * dp.K;
    launch(k_crf_edges, dim3((n + 255) / 256), dim3(256), 0, st, dp, cl, rowptr, idx, edge, temporal);
}

void launch_crf_iteration(const CrfDevParams& dp, const uint32_t* rowptr, const uint32_t* idx, const float2* edge, const float4* temporal,
                          const float* unary, const float* compat, const float* q_in, float* q_out, float* scratch, hipStream_t st) {
    const int n = dp.T * dp.K;
    const dim3 grid((n + kCrfBlock - 1) / kCrfBlock);
    if (crf_messages_in_lds(dp.C))
        launch(k_crf_iteration<true>, grid, dim3(kCrfBlock), (unsigned)(sizeof(float) * kCrfBlock * dp.C), st,
               dp, rowptr, idx, edge, temporal, unary, compat, q_in, q_out, scratch);
    else
        launch(k_crf_iteration<false>, grid, dim3(kCrfBlock), 0, st, dp, rowptr, idx, edge, temporal, unary, compat, q_in, q_out, scratch);
}

void launch_crf_expf(const float* in, float* out, size_t n, hipStream_t st) {
    const size_t blocks = std::min<size_t>((n + 255) / 256, 8192);
    launch(k_crf_expf, dim3((unsigned)std::max<size_t>(blocks, 1)), dim3(256), 0, st, in, out, n);
}

// ---- host side of inference() ------------------------------------------------------------------------------------------------------
void crf_release_device(fslic_crf* crf) {
    if (crf->eng) (void)hipSetDevice(crf->eng->device);
    crf->d_q[0].release(); crf->d_q[1].release(); crf->d_unary.release(); crf->d_compat.release(); crf->d_scratch.release();
    crf->d_cl.release(); crf->d_rowptr.release(); crf->d_idx.release(); crf->d_edge.release(); crf->d_temporal.release();
    crf->capT = 0;
    crf->cap_edges = 0;
    crf->cur = 0;
    crf->graph_uploaded = false;
    crf->eng = nullptr;
    for (auto& f : crf->frames) {
        f->dev_pos = -1;
        f->dirty_graph = f->dirty_unary = f->dirty_q = true;
        f->q_on_device = false;
    }
}

int crf_pull_q(fslic_crf* crf, fslic_crf_frame* f) {
    if (!f->q_on_device) return FSLIC_OK;
    fslic_engine* e = crf->eng;
    HIPCHK(hipSetDevice(e->device));
    SlotLease lease(e);
    int rc = lease.take();
    if (rc) return rc;
    hipStream_t st = e->slots[lease.slot].st;
    const size_t CK = crf->C * crf->K;
    HIPCHK(hipMemcpyAsync(f->q.data(), crf->d_q[crf->cur] + (size_t)f->dev_pos * CK, CK * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    f->q_on_device = false;                 // host and device agree
    return FSLIC_OK;
}

static int crf_inference_on(fslic_crf* crf, fslic_engine* e, hipStream_t st, size_t max_iter, std::vector<uint32_t>& rowptr,
                            std::vector<uint32_t>& idx) {
    const int T = (int)crf->frames.size();
    const size_t C = crf->C, K = crf->K, CK = C * K;
    // 1. frames that move to another window position (a pop shifts them, more frames reallocate) take their q along through the host
    const bool realloc = T > crf->capT;
    bool moved = realloc || !crf->graph_uploaded;
    for (int w = 0; w < T; w++) {
        fslic_crf_frame* f = crf->frames[w].get();
        if (f->dev_pos == w && !realloc) continue;
        moved = true;
        if (f->q_on_device) HIPCHK(hipMemcpyAsync(f->q.data(), crf->d_q[crf->cur] + (size_t)f->dev_pos * CK, CK * sizeof(float),
                                                  hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int w = 0; w < T; w++) {
        fslic_crf_frame* f = crf->frames[w].get();
        if (f->dev_pos == w && !realloc) continue;
        if (f->q_on_device) f->q_on_device = false;
        f->dev_pos = w;
        f->dirty_graph = f->dirty_unary = f->dirty_q = true;
    }
    // 2. buffers
    if (realloc) {
        crf->d_q[0].release(); crf->d_q[1].release(); crf->d_unary.release(); crf->d_scratch.release(); crf->d_cl.release();
        crf->d_rowptr.release(); crf->d_temporal.release();
        const size_t n = (size_t)T * K;
        int rc;
        if ((rc = crf->d_q[0].reserve((size_t)T * CK)) || (rc = crf->d_q[1].reserve((size_t)T * CK)) ||
            (rc = crf->d_unary.reserve((size_t)T * CK)) || (rc = crf->d_cl.reserve(n)) || (rc = crf->d_rowptr.reserve(n + 1)) ||
            (rc = crf->d_temporal.reserve(n)))
            return rc;
        if (!crf_messages_in_lds((int)C) && (rc = crf->d_scratch.reserve((size_t)T * CK))) return rc;
        if (!crf->d_compat && (rc = crf->d_compat.reserve(C))) return rc;
        crf->capT = T;
        crf->cur = 0;
    }
    // 3. uploads: the neighbour lists of the window as one CSR over (frame, node), whenever a frame's graph or position changed
    bool graph = moved;
    for (auto& f : crf->frames) graph = graph || f->dirty_graph;
    if (graph) {
        rowptr.assign((size_t)T * K + 1, 0u);
        size_t total = 0;
        for (int w = 0; w < T; w++)
            for (size_t i = 0; i < K; i++) {
                total += crf->frames[w]->edges[i].size();
                if (total >= (1ull << 31)) return fail(FSLIC_E_INVALID, "the frames hold 2^31 or more neighbour entries");
                rowptr[(size_t)w * K + i + 1] = (uint32_t)total;
            }
        idx.resize(total);
        for (int w = 0; w < T; w++)
            for (size_t i = 0; i < K; i++) {
                const auto& l = crf->frames[w]->edges[i];
                std::copy(l.begin(), l.end(), idx.begin() + rowptr[(size_t)w * K + i]);
            }
        if (total > crf->cap_edges || !crf->d_idx) {
            crf->d_idx.release(); crf->d_edge.release();
            int rc;
            if ((rc = crf->d_idx.reserve(total)) || (rc = crf->d_edge.reserve(total))) return rc;
            crf->cap_edges = total;
        }
        HIPCHK(hipMemcpyAsync(crf->d_rowptr, rowptr.data(), rowptr.size() * 4, hipMemcpyHostToDevice, st));
        if (total) HIPCHK(hipMemcpyAsync(crf->d_idx, idx.data(), total * 4, hipMemcpyHostToDevice, st));
        crf->graph_uploaded = true;
    }
    for (int w = 0; w < T; w++) {
        fslic_crf_frame* f = crf->frames[w].get();
        if (f->dirty_graph || graph)
            HIPCHK(hipMemcpyAsync(crf->d_cl + (size_t)w * K, f->clusters.data(), K * sizeof(fslic_cluster), hipMemcpyHostToDevice, st));
        if (f->dirty_unary)
            HIPCHK(hipMemcpyAsync(crf->d_unary + (size_t)w * CK, f->unaries.data(), CK * sizeof(float), hipMemcpyHostToDevice, st));
        if (f->dirty_q)
            HIPCHK(hipMemcpyAsync(crf->d_q[crf->cur] + (size_t)w * CK, f->q.data(), CK * sizeof(float), hipMemcpyHostToDevice, st));
        f->dirty_graph = f->dirty_unary = f->dirty_q = false;
    }
    HIPCHK(hipMemcpyAsync(crf->d_compat, crf->compat.data(), C * sizeof(float), hipMemcpyHostToDevice, st));
    // 4. the edge kernel, then max_iter sweeps ping-ponging between the two q buffers
    CrfDevParams dp;
    dp.T = T; dp.C = (int)C; dp.K = (int)K; dp.p = crf->params;
    launch_crf_edges(dp, crf->d_cl, crf->d_rowptr, crf->d_idx, crf->d_edge, crf->d_temporal, st);
    for (size_t it = 0; it < max_iter; it++) {
        launch_crf_iteration(dp, crf->d_rowptr, crf->d_idx, crf->d_edge, crf->d_temporal, crf->d_unary, crf->d_compat,
                             crf->d_q[crf->cur], crf->d_q[crf->cur ^ 1], crf->d_scratch, st);
        crf->cur ^= 1;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    for (auto& f : crf->frames) f->q_on_device = true;
    return FSLIC_OK;
}

int crf_inference(fslic_crf* crf, fslic_engine* e, size_t max_iter) {
    if (max_iter == 0) return FSLIC_OK;                          // the reference's loop does nothing
    const int T = (int)crf->frames.size();
    if (T == 0) return fail(FSLIC_E_INVALID, "inference needs at least one frame");
    if (!e) return fail(FSLIC_E_INVALID, "engine is NULL");
    if ((unsigned long long)T * crf->C * crf->K >= (1ull << 31) || (unsigned long long)T * crf->K + 1 >= (1ull << 31))
        return fail(FSLIC_E_INVALID, "frames * num_classes * num_nodes must be below 2^31");
    if (crf->eng && crf->eng != e) {                              // bound to another engine: take q home, start afresh on this one
        for (auto& f : crf->frames) {
            int rc = crf_pull_q(crf, f.get());
            if (rc) return rc;
        }
        crf_release_device(crf);
    }
    HIPCHK(hipSetDevice(e->device));
    SlotLease lease(e);
    int rc = lease.take();
    if (rc) return rc;
    crf->eng = e;
    hipStream_t st = e->slots[lease.slot].st;
    std::vector<uint32_t> rowptr, idx;                           // staging of the CSR upload: alive until the stream is synchronised
    rc = crf_inference_on(crf, e, st, max_iter, rowptr, idx);
    if (rc) {                                                    // nothing may still run against the staging; the device state is rebuilt
        const std::string msg = last_error();
        (void)hipStreamSynchronize(st);
        (void)hipGetLastError();
        for (auto& f : crf->frames) {                            // best effort: keep the q the device holds, then rebuild from the host
            if (f->q_on_device && f->dev_pos >= 0 && crf->d_q[crf->cur])
                (void)hipMemcpy(f->q.data(), crf->d_q[crf->cur] + (size_t)f->dev_pos * crf->C * crf->K, crf->C * crf->K * sizeof(float),
                                hipMemcpyDeviceToHost);
            f->q_on_device = false;
        }
        (void)hipGetLastError();
        crf_release_device(crf);
        set_last_error(msg);
    }
    return rc;
}

int crf_expf_device(fslic_engine* e, const float* in, float* out, size_t n) {
    if (!e || (n && (!in || !out))) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (n == 0) return FSLIC_OK;
    HIPCHK(hipSetDevice(e->device));
    SlotLease lease(e);
    int rc = lease.take();
    if (rc) return rc;
    hipStream_t st = e->slots[lease.slot].st;
    Device<float> d;
    if ((rc = d.reserve(2 * n))) return rc;
    hipError_t he = hipMemcpyAsync(d, in, n * sizeof(float), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) {
        launch_crf_expf(d, d + n, n, st);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(out, d + n, n * sizeof(float), hipMemcpyDeviceToHost, st);
    const hipError_t hs = hipStreamSynchronize(st);
    if (he != hipSuccess || hs != hipSuccess) return fail(FSLIC_E_HIP, std::string("crf_expf on the device: ") + hipGetErrorString(he != hipSuccess ? he : hs));
    return FSLIC_OK;
}

}  // namespace fslic
