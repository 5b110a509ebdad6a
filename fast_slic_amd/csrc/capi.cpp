// capi.cpp -- the C ABI of include/fslic_hip.h: engine lifetime, iterate() in its synchronous forms, accessors.
// (The asynchronous forms live in pipeline.cpp, the O(K) host functions and stage entry points in host_utils.cpp.)
// Part of the host engine, see engine_internal.h.
#include "engine_internal.h"
#include "crf.h"
#include "forms.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

using namespace fslic;

static_assert(sizeof(fslic_cluster) == 32, "Cluster ABI (src/fast-slic-common.h:10-23)");

extern "C" {

const char* fslic_hip_last_error(void) { return last_error().c_str(); }
const char* fslic_hip_version(void) { return "fast_slic_amd 0.3 (gfx950)"; }

int fslic_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int fslic_hip_create(int device, int n_slots, fslic_engine** out) {
    if (!out) return fail(FSLIC_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n_slots < 1 || n_slots > 64) return fail(FSLIC_E_INVALID, "n_slots must be in [1, 64]");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(FSLIC_E_HIP, "no such HIP device");
    HIPCHK(hipSetDevice(device));
    const HostTables& ht = host_tables();
    fslic_engine* e = new fslic_engine();
    e->device = device;
    e->group_size = knobs().group_size;
    e->slots.resize(n_slots);
    for (auto& s : e->slots) {
        if (hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) != hipSuccess) { fslic_hip_destroy(e); return fail(FSLIC_E_HIP, "hipStreamCreate failed"); }
        for (auto& ps : s.set) for (auto& ev : ps.ev)
            if (hipEventCreate(&ev) != hipSuccess) { fslic_hip_destroy(e); return fail(FSLIC_E_HIP, "hipEventCreate failed"); }
        for (auto& ev : s.ev_it)
            if (hipEventCreate(&ev) != hipSuccess) { fslic_hip_destroy(e); return fail(FSLIC_E_HIP, "hipEventCreate failed"); }
        if (s.d_ptrs.reserve(kPtrTable) || s.set[0].h_ptrs.reserve(kPtrTable) || s.set[1].h_ptrs.reserve(kPtrTable) ||
            s.d_gen.reserve(64) || hipMemset(s.d_gen, 0, 256) != hipSuccess) { fslic_hip_destroy(e); return fail(FSLIC_E_HIP, "pointer table allocation failed"); }
    }
    if (e->d_gamma.reserve(sizeof ht.gamma / sizeof ht.gamma[0]) || e->d_labtbl.reserve(sizeof ht.lab / sizeof ht.lab[0])) { fslic_hip_destroy(e); return fail(FSLIC_E_HIP, "hipMalloc(tables) failed"); }
    if (hipMemcpy(e->d_gamma, ht.gamma, sizeof ht.gamma, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(e->d_labtbl, ht.lab, sizeof ht.lab, hipMemcpyHostToDevice) != hipSuccess) { fslic_hip_destroy(e); return fail(FSLIC_E_HIP, "table upload failed"); }
    e->tables.gamma = e->d_gamma;
    e->tables.labtbl = e->d_labtbl;
    for (int i = 0; i < 9; i++) e->tables.cb[i] = ht.cb[i];
    *out = e;
    return FSLIC_OK;
}

void fslic_hip_destroy(fslic_engine* e) {
    if (!e) return;
    hipSetDevice(e->device);
    for (auto& s : e->slots) stop_slot_thread(e, s);     // a group still in flight is completed by its thread first
    for (auto& s : e->slots) {
        if (s.st) hipStreamSynchronize(s.st);
        free_slot(s);
    }
    delete e;                        // (the tables and whatever a slot still holds: released here, the device being current)
}

// The synchronous forms' common body: one frame on the slot the caller has leased, run to completion, and the calling thread's reports.
// (After a failure, also a late one, nothing touches the frame buffers any more: the caller's, or the stage buffers of a slot about to be
// released.)
static int iterate_on(fslic_engine* e, Slot& s, const fslic_params* p, int H, int W, int K,
                      const uint8_t* d_rgb, fslic_cluster* clusters, uint16_t* d_labels) {
    GroupJob job;
    int rc = fill_job(job, p, H, W, K, 1, &d_rgb, &clusters, &d_labels);
    if (rc) return rc;
    s.launch_timing = e->launch_timing;
    rc = run_group(e, s, job, p->debug_mode != 0);
    if (rc) return rc;
    std::string report;
    rc = make_recorder_report(s, report);
    if (rc) { drain_failed(s); return rc; }
    set_thread_timing_report(make_timing_report(s));
    set_thread_recorder_report(std::move(report));
    return FSLIC_OK;
}

int fslic_hip_iterate_device(fslic_engine* e, int slot, const fslic_params* p, int H, int W, int K,
                             const uint8_t* d_rgb, fslic_cluster* clusters, uint16_t* d_labels) {
    if (!e) return fail(FSLIC_E_INVALID, "engine is NULL");
    if (slot < 0 || slot >= (int)e->slots.size()) return fail(FSLIC_E_INVALID, "slot out of range");
    HIPCHK(hipSetDevice(e->device));
    SlotLease lease(e);
    const int rc = lease.take(slot);
    return rc ? rc : iterate_on(e, e->slots[slot], p, H, W, K, d_rgb, clusters, d_labels);
}

// Host frame in, host label map out, on whichever slot is free: concurrent calls from different threads (different
// SlicModels sharing the process-wide engine) proceed in parallel on different slots.
int fslic_hip_iterate(fslic_engine* e, const fslic_params* p, int H, int W, int K, const uint8_t* rgb,
                      fslic_cluster* clusters, uint16_t* labels) {
    if (!e) return fail(FSLIC_E_INVALID, "engine is NULL");
    if (!rgb || !labels || !clusters) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    HIPCHK(hipSetDevice(e->device));
    int S = 0;
    int rc = validate(p, H, W, K, S);
    if (rc) return rc;
    SlotLease lease(e);
    rc = lease.take();
    if (rc) return rc;
    Slot& s = e->slots[lease.slot];
    const size_t N = (size_t)H * W;
    rc = ensure_prepared(e, s, H, W, K, S, 1);
    if (rc) return rc;
    // Pageable hipMemcpyAsync in and out on the slot's stream (the runtime's own staging).  Measured against it and not kept
    // (profiles/r03_e2e_probe.txt, 1280x720 K=1600, one caller thread: 432 us per call like this): pinned staging read and written
    // in place by the LAB / relabel kernels (490 us: kernels working over PCIe take 84 us longer than on HBM) and pinned staging
    // filled by a pool of copy threads plus copy commands (543 us).
    const double t0 = knobs().host_timing ? now_us() : 0.0;
    HIPCHK(hipMemcpyAsync(s.d_rgb_stage, rgb, N * 3, hipMemcpyHostToDevice, s.st));
    const double t1 = knobs().host_timing ? now_us() : 0.0;
    rc = iterate_on(e, s, p, H, W, K, s.d_rgb_stage, clusters, s.d_out_stage);
    if (rc) return rc;
    const double t2 = s.t_begun_us, t3 = knobs().host_timing ? now_us() : 0.0;
    HIPCHK(hipMemcpyAsync(labels, s.d_out_stage, N * 2, hipMemcpyDeviceToHost, s.st));
    HIPCHK(hipStreamSynchronize(s.st));
    if (knobs().host_timing)
        fprintf(stderr, "[fslic host] iterate: frame in %.1f us, group begin %.1f, group finish (wait + write-back) %.1f, labels out %.1f (device %.1f us)\n",
                t1 - t0, t2 - t1, t3 - t2, now_us() - t3, s.total_ms * 1e3);
    return FSLIC_OK;
}

// The calling thread's recorder report (thread-local like the timing report: SlicModels on other threads sharing the engine do not
// overwrite it).  Empty before the thread's first successful call.
int fslic_hip_last_recorder_report(fslic_engine* e, const char** report, size_t* length) {
    (void)e;
    if (!report || !length) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    const std::string& r = thread_recorder_report();
    *report = r.c_str();
    *length = r.size();
    return FSLIC_OK;
}

int fslic_hip_iterate_batch(fslic_engine* e, const fslic_params* p, int H, int W, int K, int n_frames,
                            const uint8_t* const* rgb, fslic_cluster* const* clusters,
                            uint16_t* const* labels, int device_ptrs) {
    if (!e) return fail(FSLIC_E_INVALID, "engine is NULL");
    if (n_frames < 0 || (n_frames > 0 && (!rgb || !clusters || !labels))) return fail(FSLIC_E_INVALID, "bad batch arguments");
    HIPCHK(hipSetDevice(e->device));
    const int ns = (int)e->slots.size();
    const size_t N = (size_t)H * W;
    int S = 0;
    int rc = validate(p, H, W, K, S);
    if (rc) return rc;
    // Frames are cut into groups of up to group_size; every launch of a group covers all of its frames (frame =
    // last grid dimension).  Groups rotate over the slots (one stream each), so the host-side tail of one group
    // (cluster write-back) overlaps the kernels of the next.
    int G = std::min(std::max(e->group_size, 1), (int)kMaxGroup);
    if (n_frames < G * ns) G = std::max(1, (n_frames + ns - 1) / ns);       // spread a small batch over the slots
    std::vector<GroupJob> jobs((size_t)(n_frames + G - 1) / G);             // checked before anything starts
    for (size_t g = 0; g < jobs.size(); g++) {
        const int first = (int)g * G;
        if ((rc = fill_job(jobs[g], p, H, W, K, std::min(G, n_frames - first), rgb + first, clusters + first, labels + first)) || (rc = check_job(jobs[g], S))) return rc;
    }
    rc = acquire_all_slots(e);
    if (rc) return rc;
    struct Pending { int slot, first, n; };
    std::vector<Pending> inflight;
    auto finish_one = [&](const Pending& pd) -> int {
        Slot& s = e->slots[pd.slot];
        int r = group_finish(e, s);
        if (r) return r;
        if (!device_ptrs) {
            for (int i = 0; i < pd.n; i++)
                HIPCHK(hipMemcpyAsync(labels[pd.first + i], s.at(s.d_out_stage, i), N * 2, hipMemcpyDeviceToHost, s.st));
            HIPCHK(hipStreamSynchronize(s.st));
        }
        return FSLIC_OK;
    };
    // On an error nothing may still be running against the caller's buffers when control returns: every group in
    // flight is waited for first (their results are dropped), then the first error is reported.
    auto bail = [&](int code) -> int {
        for (const Pending& pd : inflight) drain_failed(e->slots[pd.slot]);
        release_all_slots(e);
        return code;
    };
    int next_slot = 0;
    for (int first = 0; first < n_frames; first += G) {
        const int n = std::min(G, n_frames - first);
        const int si = next_slot;
        next_slot = (next_slot + 1) % ns;
        // the slot may still own an unfinished group
        for (size_t q = 0; q < inflight.size(); q++)
            if (inflight[q].slot == si) {
                const Pending pd = inflight[q];
                inflight.erase(inflight.begin() + q);
                rc = finish_one(pd);
                if (rc) return bail(rc);
                break;
            }
        Slot& s = e->slots[si];
        GroupJob& job = jobs[(size_t)(first / G)];
        if (!device_ptrs) {      // the job's frame buffers become the slot's stage buffers
            rc = ensure_prepared(e, s, H, W, K, S, n);
            if (rc) return bail(rc);
            for (int i = 0; i < n; i++) {
                if (hipMemcpyAsync(s.at(s.d_rgb_stage, i), rgb[first + i], N * 3, hipMemcpyHostToDevice, s.st) != hipSuccess)
                    return bail(fail(FSLIC_E_HIP, "frame upload failed"));
                job.d_rgb[i] = s.at(s.d_rgb_stage, i);
                job.d_out[i] = s.at(s.d_out_stage, i);
            }
        }
        s.launch_timing = e->launch_timing;
        inflight.push_back({si, first, n});                  // from here on the slot's stream may hold work of this group
        rc = group_begin(e, s, job);
        if (rc) return bail(rc);
    }
    while (!inflight.empty()) {
        const Pending pd = inflight.front();
        inflight.erase(inflight.begin());
        rc = finish_one(pd);
        if (rc) return bail(rc);
    }
    if (n_frames > 0) set_thread_timing_report(make_timing_report(e->slots[0]));
    release_all_slots(e);
    return FSLIC_OK;
}

int fslic_hip_last_prelabels(fslic_engine* e, int slot, uint16_t* prelabels) {
    if (!e || !prelabels) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (slot < 0 || slot >= (int)e->slots.size()) return fail(FSLIC_E_INVALID, "slot out of range");
    HIPCHK(hipSetDevice(e->device));
    SlotLease lease(e);
    int rc = lease.take(slot);
    if (rc) return rc;
    Slot& s = e->slots[slot];
    if (!s.have_pre || s.keyH == 0) return fail(FSLIC_E_INVALID, "no frame has been processed on this slot");
    HIPCHK(hipMemcpy(prelabels, s.f.labels, (size_t)s.f.N * 2, hipMemcpyDeviceToHost));
    return FSLIC_OK;
}

// Debug entry (tests only, read-only): frame z's feature means and feature-space centroids of the slot's last LSC group, from the
// slot's LSC arena (a synchronous call has completed when it returns; the lease waits for an asynchronous group to be collected)
int fslic_hip_debug_lsc_state(fslic_engine* e, int slot, int z, int K, float* means10, float* cfeat) {
    if (!e || !means10 || !cfeat) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (slot < 0 || slot >= (int)e->slots.size()) return fail(FSLIC_E_INVALID, "slot out of range");
    HIPCHK(hipSetDevice(e->device));
    SlotLease lease(e);
    int rc = lease.take(slot);
    if (rc) return rc;
    Slot& s = e->slots[slot];
    if (!s.have_pre || s.keyH == 0 || s.p.variant != FSLIC_VARIANT_LSC) return fail(FSLIC_E_INVALID, "the slot's last group was not an LSC one");
    if (z < 0 || z >= s.nframes) return fail(FSLIC_E_INVALID, "no such frame in the slot's last group");
    if (K != s.K) return fail(FSLIC_E_INVALID, "K is not that of the slot's last group");
    HIPCHK(hipStreamSynchronize(s.st));
    LscDev l = s.l;
    l.select(z);
    HIPCHK(hipMemcpy(means10, l.means, sizeof(float) * kLscFeat, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy2D(cfeat, sizeof(float) * kLscFeat, l.cfeat, sizeof(float) * kLscCfPitch, sizeof(float) * kLscFeat, (size_t)s.K, hipMemcpyDeviceToHost));
    return FSLIC_OK;
}

// The report of the calling thread's last synchronous call or fslic_hip_wait_group (thread-local, like the reference's
// timer, src/timer.cpp:45); the engine argument is kept for the shape of the reference interface.
const char* fslic_hip_last_timing_report(fslic_engine* e) { return e ? thread_timing_report().c_str() : ""; }

int fslic_hip_last_device_times(fslic_engine* e, int slot, float* total_ms, float* full_assign_ms) {
    if (!e || slot < 0 || slot >= (int)e->slots.size()) return fail(FSLIC_E_INVALID, "bad engine/slot");
    if (total_ms) *total_ms = e->slots[slot].total_ms;
    if (full_assign_ms) *full_assign_ms = e->slots[slot].fa_ms;
    return FSLIC_OK;
}

int fslic_hip_set_launch_timing(fslic_engine* e, int on) {
    if (!e) return fail(FSLIC_E_INVALID, "engine is NULL");
    e->launch_timing = on != 0;
    return FSLIC_OK;
}

int fslic_hip_lab_force_generic(fslic_engine* e, int on) {
    if (!e) return fail(FSLIC_E_INVALID, "engine is NULL");
    e->lab_force_generic.store(on != 0);
    return FSLIC_OK;
}

int fslic_hip_debug_fail_group(fslic_engine* e, int what, int after) {
    if (!e || what < -1 || what > 2 || after < 0) return fail(FSLIC_E_INVALID, "bad arguments");
    e->debug_fail_what.store(-1);
    e->debug_fail_after.store(after);
    e->debug_fail_what.store(what);
    return FSLIC_OK;
}

int fslic_hip_last_assign_loop(fslic_engine* e, int slot, float* sum_ms, double* visited_px, int* launches) {
    if (!e || slot < 0 || slot >= (int)e->slots.size()) return fail(FSLIC_E_INVALID, "bad engine/slot");
    const Slot& s = e->slots[slot];
    if (sum_ms) *sum_ms = s.assign_loop_ms;
    if (visited_px) *visited_px = s.assign_loop_px;
    if (launches) *launches = s.n_timed_iters;
    return FSLIC_OK;
}

int fslic_hip_last_group_frames(fslic_engine* e, int slot) {
    if (!e || slot < 0 || slot >= (int)e->slots.size()) return -1;
    return e->slots[slot].nframes;
}

int fslic_hip_last_launch_mode(fslic_engine* e, int slot) {
    if (!e || slot < 0 || slot >= (int)e->slots.size()) return -1;
    return e->slots[slot].last_launch_mode;
}

int fslic_hip_last_path(fslic_engine* e, int slot) {
    if (!e || slot < 0 || slot >= (int)e->slots.size()) return -1;
    return e->slots[slot].last_path;
}

int fslic_hip_last_host_topk_frames(fslic_engine* e, int slot) {
    if (!e || slot < 0 || slot >= (int)e->slots.size()) return -1;
    return e->slots[slot].n_host_topk;
}

int fslic_hip_separate_pass_redos(fslic_engine* e, int slot) {
    if (!e || slot < 0 || slot >= (int)e->slots.size()) return -1;
    return __atomic_load_n(&e->slots[slot].n_separate_redo, __ATOMIC_RELAXED);
}

int fslic_hip_uncovered_redos(fslic_engine* e, int slot) {
    if (!e || slot < 0 || slot >= (int)e->slots.size()) return -1;
    return __atomic_load_n(&e->slots[slot].n_uncovered_redo, __ATOMIC_RELAXED);
}

long long fslic_hip_overlapped_groups(fslic_engine* e) {
    if (!e) return -1;
    return e->overlapped_groups.load(std::memory_order_relaxed);
}

// ---- the form record (forms.h; the record itself is in host_utils.cpp) ----
int fslic_hip_debug_forms_seen(uint32_t* codes, int cap, int clear) {
    if (cap < 0 || (cap > 0 && !codes)) return -1;
    return fslic::forms_seen(codes, cap, clear != 0);
}

int fslic_hip_debug_forms_all(uint32_t* codes, int cap) {
    if (cap < 0 || (cap > 0 && !codes)) return -1;
    const int na = fslic::assign_forms(codes, cap);
    return na + fslic::preempt_forms(codes + std::min(na, cap), std::max(cap - na, 0));
}

// ---- SimpleCRF (src/simple-crf.{h,hpp,cpp}): host state and bookkeeping here, inference in crf.hip --------------------------------
// Every entry holds the CRF's mutex (a frame's: its parent's) for its duration; the numerics of the setters are the reference's
// expressions (host libm logf, crf_expf for expf).
#define CRF_LOCK(crf) std::lock_guard<std::mutex> crf_lock__((crf)->mu)

static fslic_crf_frame* crf_frame_at(fslic_crf* crf, int time) {
    if (crf->frames.empty()) return nullptr;
    const long long d = (long long)time - crf->frames.front()->time;          // the window holds consecutive times
    if (d < 0 || d >= (long long)crf->frames.size()) return nullptr;
    return crf->frames[(size_t)d].get();
}
// Unaries or q are about to be replaced on the host, or read there.
static void crf_touch_unary(fslic_crf_frame* f) { f->dirty_unary = true; }
static void crf_touch_q(fslic_crf_frame* f) { f->q_on_device = false; f->dirty_q = true; }

int fslic_hip_crf_new(size_t num_classes, size_t num_nodes, fslic_crf** out) {
    if (!out) return fail(FSLIC_E_INVALID, "out is NULL");
    *out = nullptr;
    if (num_classes == 0 || num_nodes == 0) return fail(FSLIC_E_INVALID, "num_classes and num_nodes must be positive");
    if (num_classes >= (1ull << 31) || num_nodes >= (1ull << 31) || (unsigned long long)num_classes * num_nodes >= (1ull << 31))
        return fail(FSLIC_E_INVALID, "num_classes * num_nodes must be below 2^31");
    fslic_crf* crf = new fslic_crf();
    crf->C = num_classes;
    crf->K = num_nodes;
    crf->compat.assign(num_classes, 1.0f);                       // simple-crf.hpp:79-89
    crf->params.spatial_w = 10; crf->params.temporal_w = 10;
    crf->params.spatial_srgb = 13; crf->params.temporal_srgb = 13;
    crf->params.spatial_sxy = 80;
    crf->params.spatial_smooth_w = 0; crf->params.spatial_smooth_sxy = 3;
    *out = crf;
    return FSLIC_OK;
}

void fslic_hip_crf_free(fslic_crf* crf) {
    if (!crf) return;
    crf_release_device(crf);
    delete crf;
}

int fslic_hip_crf_copy(fslic_crf* crf, fslic_crf** out) {
    if (!crf || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    *out = nullptr;
    CRF_LOCK(crf);
    for (auto& f : crf->frames) {
        int rc = crf_pull_q(crf, f.get());
        if (rc) return rc;
    }
    fslic_crf* c = new fslic_crf();
    c->C = crf->C; c->K = crf->K; c->next_time = crf->next_time; c->compat = crf->compat; c->params = crf->params;
    for (auto& f : crf->frames) {
        std::unique_ptr<fslic_crf_frame> g(new fslic_crf_frame());
        g->parent = c; g->time = f->time; g->clusters = f->clusters; g->edges = f->edges; g->unaries = f->unaries; g->q = f->q;
        c->frames.push_back(std::move(g));
    }
    *out = c;
    return FSLIC_OK;
}

int fslic_hip_crf_get_params(fslic_crf* crf, fslic_crf_params* out) {
    if (!crf || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(crf);
    *out = crf->params;
    return FSLIC_OK;
}

int fslic_hip_crf_set_params(fslic_crf* crf, const fslic_crf_params* params) {
    if (!crf || !params) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(crf);
    crf->params = *params;                                       // (the edge kernel reads them at every inference)
    return FSLIC_OK;
}

int fslic_hip_crf_set_compat(fslic_crf* crf, int cls, float compat_value) {
    if (!crf) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(crf);
    if (cls < 0 || (size_t)cls >= crf->C) return fail(FSLIC_E_INVALID, "class out of range");
    crf->compat[(size_t)cls] = compat_value;
    return FSLIC_OK;
}

int fslic_hip_crf_get_compat(fslic_crf* crf, int cls, float* out) {
    if (!crf || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(crf);
    if (cls < 0 || (size_t)cls >= crf->C) return fail(FSLIC_E_INVALID, "class out of range");
    *out = crf->compat[(size_t)cls];
    return FSLIC_OK;
}

int fslic_hip_crf_num_classes(fslic_crf* crf, size_t* num_classes, size_t* num_nodes) {
    if (!crf) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (num_classes) *num_classes = crf->C;
    if (num_nodes) *num_nodes = crf->K;
    return FSLIC_OK;
}

int fslic_hip_crf_first_time(fslic_crf* crf) {
    if (!crf) return -1;
    CRF_LOCK(crf);
    return crf->frames.empty() ? -1 : crf->frames.front()->time;
}

int fslic_hip_crf_last_time(fslic_crf* crf) {
    if (!crf) return -1;
    CRF_LOCK(crf);
    return crf->frames.empty() ? -1 : crf->frames.back()->time;
}

size_t fslic_hip_crf_num_frames(fslic_crf* crf) {
    if (!crf) return 0;
    CRF_LOCK(crf);
    return crf->frames.size();
}

int fslic_hip_crf_pop_frame(fslic_crf* crf) {
    if (!crf) return -1;
    CRF_LOCK(crf);
    if (crf->frames.empty()) return -1;
    const int t = crf->frames.front()->time;
    crf->frames.pop_front();                 // the others keep their device slices until the next inference moves them
    return t;
}

int fslic_hip_crf_push_frame(fslic_crf* crf, fslic_crf_frame** out) {
    if (!crf || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    *out = nullptr;
    CRF_LOCK(crf);
    if (crf->next_time == INT32_MAX) return fail(FSLIC_E_INVALID, "frame times exhausted");
    std::unique_ptr<fslic_crf_frame> f(new fslic_crf_frame());     // SimpleCRFFrame ctor, simple-crf.hpp:29-34
    f->parent = crf;
    f->time = crf->next_time++;
    fslic_cluster one{};
    one.num_members = 1;
    f->clusters.assign(crf->K, one);
    f->edges.resize(crf->K);
    f->unaries.assign(crf->C * crf->K, 0.0f);
    f->q.assign(crf->C * crf->K, 0.0f);
    *out = f.get();
    crf->frames.push_back(std::move(f));
    return FSLIC_OK;
}

int fslic_hip_crf_frame(fslic_crf* crf, int time, fslic_crf_frame** out) {
    if (!crf || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(crf);
    *out = crf_frame_at(crf, time);
    if (!*out) return fail(FSLIC_E_INVALID, "Time out of range");            // simple-crf.hpp:111-115
    return FSLIC_OK;
}

int fslic_hip_crf_frame_time(fslic_crf_frame* frame) { return frame ? frame->time : -1; }

int fslic_hip_crf_frame_set_clusters(fslic_crf_frame* frame, const fslic_cluster* clusters) {
    if (!frame || !clusters) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    std::copy(clusters, clusters + frame->clusters.size(), frame->clusters.begin());
    frame->dirty_graph = true;
    return FSLIC_OK;
}

int fslic_hip_crf_frame_get_clusters(fslic_crf_frame* frame, fslic_cluster* clusters) {
    if (!frame || !clusters) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    std::copy(frame->clusters.begin(), frame->clusters.end(), clusters);
    return FSLIC_OK;
}

// Both forms validate every row before they change one (simple-crf.cpp:11-19 replaces rows 0 .. conn->num_nodes-1).
int fslic_hip_crf_frame_set_connectivity(fslic_crf_frame* frame, int num_rows, const int* num_neighbors, const uint32_t* neighbors,
                                         size_t stride) {
    if (!frame || (num_rows > 0 && !num_neighbors)) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    const size_t K = frame->clusters.size();
    if (num_rows < 0 || (size_t)num_rows > K) return fail(FSLIC_E_INVALID, "more rows than nodes");
    for (int i = 0; i < num_rows; i++) {
        if (num_neighbors[i] < 0 || (size_t)num_neighbors[i] > stride) return fail(FSLIC_E_INVALID, "num_neighbors out of range");
        if (num_neighbors[i] > 0 && !neighbors) return fail(FSLIC_E_INVALID, "NULL pointer argument");
        for (int k = 0; k < num_neighbors[i]; k++)
            if (neighbors[(size_t)i * stride + k] >= K) return fail(FSLIC_E_INVALID, "neighbour index out of range");
    }
    for (int i = 0; i < num_rows; i++) {
        const uint32_t* row = neighbors ? neighbors + (size_t)i * stride : nullptr;
        frame->edges[(size_t)i].assign(row, row + num_neighbors[i]);
    }
    frame->dirty_graph = true;
    return FSLIC_OK;
}

int fslic_hip_crf_frame_set_connectivity_csr(fslic_crf_frame* frame, int num_rows, const int64_t* offsets, const uint32_t* indices) {
    if (!frame || (num_rows > 0 && !offsets)) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    const size_t K = frame->clusters.size();
    if (num_rows < 0 || (size_t)num_rows > K) return fail(FSLIC_E_INVALID, "more rows than nodes");
    if (num_rows > 0 && offsets[0] < 0) return fail(FSLIC_E_INVALID, "offsets must not decrease");
    for (int i = 0; i < num_rows; i++) {
        if (offsets[i + 1] < offsets[i]) return fail(FSLIC_E_INVALID, "offsets must not decrease");
        if (offsets[i + 1] > offsets[i] && !indices) return fail(FSLIC_E_INVALID, "NULL pointer argument");
        for (int64_t k = offsets[i]; k < offsets[i + 1]; k++)
            if (indices[k] >= K) return fail(FSLIC_E_INVALID, "neighbour index out of range");
    }
    for (int i = 0; i < num_rows; i++) {
        if (offsets[i + 1] > offsets[i]) frame->edges[(size_t)i].assign(indices + offsets[i], indices + offsets[i + 1]);
        else frame->edges[(size_t)i].clear();
    }
    frame->dirty_graph = true;
    return FSLIC_OK;
}

int fslic_hip_crf_frame_get_connectivity(fslic_crf_frame* frame, int64_t* offsets, uint32_t* indices) {
    if (!frame || !offsets) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    int64_t o = 0;
    offsets[0] = 0;
    for (size_t i = 0; i < frame->edges.size(); i++) {
        const auto& l = frame->edges[i];
        if (indices) std::copy(l.begin(), l.end(), indices + o);
        o += (int64_t)l.size();
        offsets[i + 1] = o;
    }
    return FSLIC_OK;
}

int fslic_hip_crf_frame_set_mask(fslic_crf_frame* frame, const int32_t* classes, float confidence) {
    if (!frame || !classes) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    const size_t C = frame->parent->C, K = frame->parent->K;
    for (size_t i = 0; i < K; i++)
        if (classes[i] < 0 || (size_t)classes[i] >= C) return fail(FSLIC_E_INVALID, "class out of range");
    // simple-crf.cpp:39-53, float expressions as the reference build evaluates them (num_classes is a size_t; GCC fuses the product
    // of active_proba into its sum, see crf.h)
    const float lowest_proba = 1.0f / (float)C;
    const float active_proba = crf_fmaf(1 - lowest_proba, confidence, lowest_proba);
    const float inactive_proba = (1 - active_proba) / (float)(C - 1);
    const float active_unary = -logf(active_proba), inactive_unary = -logf(inactive_proba);
    std::fill(frame->unaries.begin(), frame->unaries.end(), inactive_unary);
    for (size_t i = 0; i < K; i++) frame->unaries[K * (size_t)classes[i] + i] = active_unary;
    crf_touch_unary(frame);
    return FSLIC_OK;
}

int fslic_hip_crf_frame_set_proba(fslic_crf_frame* frame, const float* probas) {
    if (!frame || !probas) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    for (size_t k = 0; k < frame->unaries.size(); k++) frame->unaries[k] = -logf(probas[k]);     // simple-crf.cpp:53-55
    crf_touch_unary(frame);
    return FSLIC_OK;
}

int fslic_hip_crf_frame_set_unbiased(fslic_crf_frame* frame) {
    if (!frame) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    std::fill(frame->unaries.begin(), frame->unaries.end(), logf((float)frame->parent->C));     // simple-crf.cpp:34-37
    crf_touch_unary(frame);
    return FSLIC_OK;
}

int fslic_hip_crf_frame_set_unary(fslic_crf_frame* frame, const float* unary_energies) {
    if (!frame || !unary_energies) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    std::copy(unary_energies, unary_energies + frame->unaries.size(), frame->unaries.begin());
    crf_touch_unary(frame);
    return FSLIC_OK;
}

int fslic_hip_crf_frame_get_unary(fslic_crf_frame* frame, float* unary_energies) {
    if (!frame || !unary_energies) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    std::copy(frame->unaries.begin(), frame->unaries.end(), unary_energies);
    return FSLIC_OK;
}

int fslic_hip_crf_frame_spatial_energy(fslic_crf_frame* frame, int node_i, int node_j, float* out) {
    if (!frame || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    const size_t K = frame->clusters.size();
    if (node_i < 0 || node_j < 0 || (size_t)node_i >= K || (size_t)node_j >= K) return fail(FSLIC_E_INVALID, "node number is out of range");
    *out = node_i == node_j ? 0.0f : crf_spatial_energy(frame->parent->params, frame->clusters[(size_t)node_i], frame->clusters[(size_t)node_j]);
    return FSLIC_OK;
}

int fslic_hip_crf_frame_temporal_energy(fslic_crf_frame* frame, fslic_crf_frame* other_frame, int node_i, float* out) {
    if (!frame || !other_frame || !out) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    std::unique_lock<std::mutex> a(frame->parent->mu, std::defer_lock), b(other_frame->parent->mu, std::defer_lock);
    if (frame->parent == other_frame->parent) a.lock();
    else std::lock(a, b);
    if (node_i < 0 || (size_t)node_i >= frame->clusters.size() || (size_t)node_i >= other_frame->clusters.size())
        return fail(FSLIC_E_INVALID, "node number is out of range");
    *out = frame == other_frame ? 0.0f
                                : crf_temporal_energy(frame->parent->params, frame->clusters[(size_t)node_i], other_frame->clusters[(size_t)node_i]);
    return FSLIC_OK;
}

int fslic_hip_crf_frame_get_inferred(fslic_crf_frame* frame, float* probas) {
    if (!frame || !probas) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    int rc = crf_pull_q(frame->parent, frame);
    if (rc) return rc;
    std::copy(frame->q.begin(), frame->q.end(), probas);
    return FSLIC_OK;
}

static void crf_reset_inferred(fslic_crf_frame* f) {          // simple-crf.cpp:57-59
    for (size_t k = 0; k < f->q.size(); k++) f->q[k] = crf_expf(-f->unaries[k]);
    crf_touch_q(f);
}

int fslic_hip_crf_frame_reset_inferred(fslic_crf_frame* frame) {
    if (!frame) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(frame->parent);
    crf_reset_inferred(frame);
    return FSLIC_OK;
}

int fslic_hip_crf_initialize(fslic_crf* crf) {
    if (!crf) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(crf);
    for (auto& f : crf->frames) crf_reset_inferred(f.get());    // simple-crf.cpp:153-157
    return FSLIC_OK;
}

int fslic_hip_crf_inference(fslic_crf* crf, fslic_engine* e, size_t max_iter) {
    if (!crf) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    CRF_LOCK(crf);
    return crf_inference(crf, e, max_iter);
}

int fslic_hip_crf_expf_host(const float* in, float* out, size_t n, int use_libm) {
    if (n && (!in || !out)) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    if (use_libm) for (size_t k = 0; k < n; k++) out[k] = expf(in[k]);
    else for (size_t k = 0; k < n; k++) out[k] = crf_expf(in[k]);
    return FSLIC_OK;
}

int fslic_hip_crf_expf_device(fslic_engine* e, const float* in, float* out, size_t n) { return crf_expf_device(e, in, out, n); }

#ifdef FSLIC_LAB
// lab build only: the status words of frame `frame` of the last group on `slot` as the export left them in pinned memory
int fslic_hip_debug_status_words(fslic_engine* e, int slot, int frame, uint32_t* out16) {
    if (!e || slot < 0 || slot >= (int)e->slots.size() || frame < 0 || frame >= (int)kMaxGroup || !out16) return FSLIC_E_INVALID;
    std::memcpy(out16, status(e->slots[slot], frame), sizeof(uint32_t) * kStatusWords);
    return FSLIC_OK;
}
// lab build only: the last `nwords` words of frame `frame`'s candidate-leader array (where lab build 2 leaves the tile
// kernel's time stamps)
int fslic_hip_debug_cand_tail(fslic_engine* e, int slot, int frame, int nwords, int32_t* out) {
    if (!e || slot < 0 || slot >= (int)e->slots.size() || !out) return FSLIC_E_INVALID;
    Slot& s = e->slots[slot];
    const int32_t* base = s.at(s.c.cand_leader, frame) + (size_t)s.c.N - nwords;
    return hipMemcpy(out, base, sizeof(int32_t) * (size_t)nwords, hipMemcpyDeviceToHost) == hipSuccess ? FSLIC_OK : FSLIC_E_HIP;
}
// lab build 4: `nwords` words from the start of frame `frame`'s candidate-area array (phase stamps of the block assign kernel)
int fslic_hip_debug_cand_area_head(fslic_engine* e, int slot, int frame, int nwords, uint32_t* out) {
    if (!e || slot < 0 || slot >= (int)e->slots.size() || !out) return FSLIC_E_INVALID;
    Slot& s = e->slots[slot];
    const uint32_t* base = s.at(s.c.cand_area, frame);
    return hipMemcpy(out, base, sizeof(uint32_t) * (size_t)nwords, hipMemcpyDeviceToHost) == hipSuccess ? FSLIC_OK : FSLIC_E_HIP;
}
#endif

}  // extern "C"
