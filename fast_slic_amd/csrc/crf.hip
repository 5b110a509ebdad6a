// crf.hip -- the device side of SimpleCRF's host state (crf.h): inference() (src/simple-crf.cpp:62-153) on gfx950.
// The kernels are the tensor CRF's (crf_tensor.h, crf_tensor.hip), so the mean-field arithmetic exists once:
//   launch_crf_tensor_edges  once per inference(), every frame, temporal links on: row bounds, per neighbour entry the spatial energy and
//                            the member factor, per node the temporal energies and factors towards t-1 and t+1.
//   launch_crf_tensor_sweep  one Jacobi sweep of SimpleCRF::infer_once over every frame: reads q of the previous sweep, writes the other
//                            buffer (the reference's new_probas).  A block is 64 nodes of one frame times up to 16 wavefronts, one per
//                            class slice; messages stay in LDS up to kCrfTensorLdsClasses (128) classes and go to a [T][C][K] plane of
//                            the CRF's workspace above that.
// What this file adds is the window: the frames go up in the form those kernels read (clusters as yxrgb planes and member counts, the
// neighbour lists as one int64 / int32 CSR over (frame, node)), q stays on the device between calls.
// max_iter sweeps go back to back on one slot's stream; one synchronisation at the end.
#include "crf.h"
#include "crf_tensor.h"

#include <algorithm>

// Every rounding of the CRF's device code (this file, crf_tensor.hip, crf_tensor_sweep.h) is the reference build's: a product is fused
// into a sum exactly where that build fuses it (__builtin_fmaf, see crf.h) and nowhere else (see realdist.hip for what hipcc's default
// would do), division and sqrtf are the correctly rounded ones (HIP's default), the exponential is crf_expf.
#pragma clang fp contract(off)

namespace fslic {

__global__ __launch_bounds__(256) void k_crf_expf(const float* __restrict__ in, float* __restrict__ out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) out[p] = crf_expf(in[p]);
}

static void launch_crf_expf(const float* in, float* out, size_t n, hipStream_t st) {
    const size_t blocks = std::min<size_t>((n + 255) / 256, 8192);
    launch(k_crf_expf, dim3((unsigned)std::max<size_t>(blocks, 1)), dim3(256), 0, st, in, out, n);
}

// ---- host side of inference() ------------------------------------------------------------------------------------------------------
void crf_release_device(fslic_crf* crf) {
    if (crf->eng) (void)hipSetDevice(crf->eng->device);
    crf->d_q[0].release(); crf->d_q[1].release(); crf->d_unary.release(); crf->d_compat.release();
    crf->d_cl.release(); crf->d_offsets.release(); crf->d_idx.release(); crf->d_work.release();
    crf->capT = 0;
    crf->nnz = 0;
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

// Host staging of the window's upload: alive until the stream is synchronised.
struct CrfStaging {
    std::vector<int64_t> offsets;
    std::vector<uint32_t> idx;
    std::unique_ptr<float[]> cl;            // crf_stage_clusters writes every word: no fill first
};

static int crf_inference_on(fslic_crf* crf, fslic_engine* e, hipStream_t st, size_t max_iter, CrfStaging& s) {
    const int T = (int)crf->frames.size();
    const size_t C = crf->C, K = crf->K, CK = C * K, n = (size_t)T * K;
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
    // 2. the buffers whose size follows the number of frames (reserve frees and allocates anew when it has to grow)
    if (realloc) {
        int rc;
        if ((rc = crf->d_q[0].reserve((size_t)T * CK)) || (rc = crf->d_q[1].reserve((size_t)T * CK)) ||
            (rc = crf->d_unary.reserve((size_t)T * CK)) || (rc = crf->d_cl.reserve(6 * n)) || (rc = crf->d_offsets.reserve(n + 1)) ||
            (rc = crf->d_compat.reserve(C)))
            return rc;
        crf->capT = T;
        crf->cur = 0;
    }
    // 3. uploads.  Whenever a frame's graph or position changed, the whole window anew: its neighbour lists as one CSR over
    //    (frame, node), its clusters as planes and member counts, each with one copy
    bool graph = moved;
    for (auto& f : crf->frames) graph = graph || f->dirty_graph;
    float* yxrgb = crf->d_cl;
    const int32_t* members = reinterpret_cast<const int32_t*>(yxrgb + 5 * n);
    if (graph) {
        s.offsets.assign(n + 1, 0);
        size_t total = 0;
        for (int w = 0; w < T; w++)
            for (size_t i = 0; i < K; i++) {
                total += crf->frames[w]->edges[i].size();
                if (total >= (1ull << 31)) return fail(FSLIC_E_INVALID, "the frames hold 2^31 or more neighbour entries");
                s.offsets[(size_t)w * K + i + 1] = (int64_t)total;
            }
        s.idx.resize(total);
        s.cl.reset(new float[6 * n]);
        for (int w = 0; w < T; w++) {
            for (size_t i = 0; i < K; i++) {
                const auto& l = crf->frames[w]->edges[i];
                std::copy(l.begin(), l.end(), s.idx.begin() + s.offsets[(size_t)w * K + i]);
            }
            crf_stage_clusters(crf->frames[w]->clusters.data(), (size_t)w, (size_t)T, K, s.cl.get());
        }
        int rc;
        if ((rc = crf->d_idx.reserve(total))) return rc;
        crf->nnz = (long long)total;
        HIPCHK(hipMemcpyAsync(crf->d_offsets, s.offsets.data(), s.offsets.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
        // the setters refuse an index >= num_nodes, so the same bytes read as int32 hold no dead entry
        if (total) HIPCHK(hipMemcpyAsync(crf->d_idx, s.idx.data(), total * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(yxrgb, s.cl.get(), 6 * n * sizeof(float), hipMemcpyHostToDevice, st));
        crf->graph_uploaded = true;
    }
    for (int w = 0; w < T; w++) {
        fslic_crf_frame* f = crf->frames[w].get();
        if (f->dirty_unary)
            HIPCHK(hipMemcpyAsync(crf->d_unary + (size_t)w * CK, f->unaries.data(), CK * sizeof(float), hipMemcpyHostToDevice, st));
        if (f->dirty_q)
            HIPCHK(hipMemcpyAsync(crf->d_q[crf->cur] + (size_t)w * CK, f->q.data(), CK * sizeof(float), hipMemcpyHostToDevice, st));
        f->dirty_graph = f->dirty_unary = f->dirty_q = false;
    }
    HIPCHK(hipMemcpyAsync(crf->d_compat, crf->compat.data(), C * sizeof(float), hipMemcpyHostToDevice, st));
    // 4. the edge pass into the workspace (rows, temporal, edge; msg above kCrfTensorLdsClasses classes), then max_iter sweeps
    //    ping-ponging between the two q buffers
    const CrfTensorWorkspace ws = crf_tensor_workspace(T, (int)C, (int)K, crf->nnz, kCrfCallSaved, false);
    int rc = crf->d_work.reserve(ws.bytes);
    if (rc) return rc;
    const CrfTensorBuffers b = crf_tensor_buffers(crf->d_work.get(), ws);
    CrfTensorParams dp;
    dp.N = T; dp.C = (int)C; dp.K = (int)K; dp.temporal = 1; dp.nnz = crf->nnz; dp.p = crf->params;
    launch_crf_tensor_edges(dp, yxrgb, members, crf->d_offsets, crf->d_idx, b.rows, b.edge, b.temporal, st);
    for (size_t it = 0; it < max_iter; it++) {
        launch_crf_tensor_sweep(dp, b.lists(), crf->d_idx, crf->d_unary, crf->d_compat, crf->d_q[crf->cur], crf->d_q[crf->cur ^ 1], b.msg, st);
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
    CrfStaging staging;
    rc = crf_inference_on(crf, e, st, max_iter, staging);
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
