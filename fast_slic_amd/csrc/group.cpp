// group.cpp -- one launch group of the engine: a group is up to 16 frames of identical geometry that share every
// kernel launch (frame = last grid dimension).  Staging of the caller's clusters, the launch sequence of iterate()
// (src/context.cpp:108-197) enqueued operation by operation or replayed as one hipGraph, completion, the rare host
// steps, and the write-back of the Cluster[K] blocks.  Part of the host engine, see engine_internal.h.
#include "engine_internal.h"
#include "forms.h"

#include <time.h>

#include <algorithm>
#include <cassert>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>

namespace fslic {

double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int validate(const fslic_params* p, int H, int W, int K, int& S) {
    if (!p) return fail(FSLIC_E_INVALID, "params is NULL");
    static_assert(sizeof(fslic_params) == 64 && offsetof(fslic_params, abi) == 40 && offsetof(fslic_params, variant) == 44, "fslic_params layout (include/fslic_hip.h)");
    if (p->abi != FSLIC_PARAMS_ABI) return fail(FSLIC_E_INVALID, "fslic_params.abi != FSLIC_PARAMS_ABI: the caller was built against another layout of the struct (include/fslic_hip.h)");
    if (p->reserved[0] | p->reserved[1] | p->reserved[2] | p->reserved[3]) return fail(FSLIC_E_INVALID, "fslic_params.reserved must be 0");
    if (H <= 0 || W <= 0) return fail(FSLIC_E_INVALID, "H and W must be positive");
    if (H > 32767 || W > 32767) return fail(FSLIC_E_INVALID, "H and W must fit int16 (src/context.cpp:262)");
    if ((long long)H * W >= (1ll << 31)) return fail(FSLIC_E_INVALID, "H*W must fit int32");
    if (K <= 0 || K >= 65534) return fail(FSLIC_E_INVALID, "num_components must be in [1, 65533] (cfast_slic.pyx:24-27)");
    if (p->subsample_stride < 1 || p->subsample_stride > 255) return fail(FSLIC_E_INVALID, "subsample_stride must be in [1, 255]");
    if (p->max_iter < 0) return fail(FSLIC_E_INVALID, "max_iter must be >= 0");
    if (p->preemptive && !std::isfinite(p->preemptive_thres)) return fail(FSLIC_E_INVALID, "preemptive_thres must be finite");
    if (p->variant < FSLIC_VARIANT_SLIC || p->variant > FSLIC_VARIANT_REALDIST_NOQ) return fail(FSLIC_E_UNSUPPORTED, "unknown variant");
    if (!(p->compactness > 0.0f) || !std::isfinite(p->compactness)) return fail(FSLIC_E_INVALID, "compactness must be a positive finite number");
    S = (int)(int16_t)sqrt(H * W / K);   // src/context.h:60
    if (S < 1) return fail(FSLIC_E_INVALID, "num_components exceeds the number of pixels (S == 0)");
    return FSLIC_OK;
}

int fill_job(GroupJob& j, const fslic_params* p, int H, int W, int K, int n,
             const uint8_t* const* d_rgb, fslic_cluster* const* clusters, uint16_t* const* d_out) {
    if (n < 1 || n > (int)kMaxGroup || !d_rgb || !clusters || !d_out) return fail(FSLIC_E_INVALID, "bad group arguments");
    if (!p) return fail(FSLIC_E_INVALID, "params is NULL");
    // a label map is uint16_t[H * W]: an odd address cannot hold one (include/fslic_hip.h; the frames themselves may lie anywhere)
    for (int i = 0; i < n; i++)
        if (reinterpret_cast<uintptr_t>(d_out[i]) & 1) return fail(FSLIC_E_INVALID, "d_labels[" + std::to_string(i) + "] is not 2-byte aligned");
    j.p = *p; j.H = H; j.W = W; j.K = K; j.n = n;
    for (int i = 0; i < n; i++) { j.d_rgb[i] = d_rgb[i]; j.clusters[i] = clusters[i]; j.d_out[i] = d_out[i]; }
    return FSLIC_OK;
}

int check_job(const GroupJob& j, int& S) {
    if (j.n < 1 || j.n > (int)kMaxGroup) return fail(FSLIC_E_INVALID, "bad group arguments");
    const int rc = validate(&j.p, j.H, j.W, j.K, S);
    if (rc) return rc;
    for (int i = 0; i < j.n; i++)
        if (!j.clusters[i] || !j.d_rgb[i] || !j.d_out[i]) return fail(FSLIC_E_INVALID, "NULL pointer argument");
    return FSLIC_OK;
}

// ---- the top-K / ranking step of ConnectivityEnforcer::execute (src/cca.cpp:205-237) on the host ----
// Input: candidates (components with area >= threshold) in ASCENDING LEADER order, which is ascending component
// number, the order the reference hands to std::partial_sort.  libstdc++'s std::partial_sort decides ties at
// the cut exactly as it does for the reference (same library, same input order).  Output: kept leaders in
// ascending order; label = position (src/cca.cpp:229-237).
void select_kept_sorted(const int32_t* leader, const uint32_t* area, uint32_t M, int K,
                        int32_t* keep_leader, uint16_t* keep_label, uint32_t& n_keep) {
    if ((size_t)K >= (size_t)M) {
        for (uint32_t i = 0; i < M; i++) { keep_leader[i] = leader[i]; keep_label[i] = (uint16_t)i; }
        n_keep = M;
        return;
    }
    std::vector<uint32_t> order(M);
    std::iota(order.begin(), order.end(), 0u);
    // src/cca.cpp:225-228 calls std::partial_sort; on an area tie at the cut the survivors depend on the library's heap
    // mechanics, so the same call is made here (the device path replays libstdc++'s __heap_select, see k_cca_select;
    // this host path only serves frames with more candidates than the device sorts).
    auto by_area = [&](uint32_t a, uint32_t b) { return area[a] > area[b]; };
    std::partial_sort(order.begin(), order.begin() + K, order.end(), by_area);
    std::vector<uint8_t> kept(M, 0);
    for (int i = 0; i < K; i++) kept[order[i]] = 1;
    uint32_t n = 0;
    for (uint32_t i = 0; i < M; i++)
        if (kept[i]) { keep_leader[n] = leader[i]; keep_label[n] = (uint16_t)n; n++; }
    n_keep = n;
}

// The per-frame output pointers must already be in s.d_ptrs[kMaxGroup + i] (upload_ptrs).
CcaDev cca_view(const Slot& s, int i0, const uint16_t* d_in0, size_t in_stride, int K, int min_threshold) {
    CcaDev c = s.c;
    c.in = d_in0; c.in_stride = in_stride; c.K = K; c.min_threshold = min_threshold;
    c.outs = nullptr;
    c.out = nullptr;
    // host-side advance to frame i0 (CcaDev::select dereferences the device array, so spell it out here)
    FrameDev::adv(c.in, (size_t)i0 * in_stride);
    const size_t d = (size_t)i0 * c.frame_bytes;
    FrameDev::adv(c.lid, d); FrameDev::adv(c.nrec, d); FrameDev::adv(c.narea, d);
    FrameDev::adv(c.nfinal, d); FrameDev::adv(c.vedge, d); FrameDev::adv(c.roots, d);
    FrameDev::adv(c.counters, d);
    FrameDev::adv(c.cand_leader, d); FrameDev::adv(c.cand_area, d);
    c.outs = reinterpret_cast<uint16_t* const*>(s.d_ptrs + kMaxGroup + i0);
    return c;
}

// Caller's per-frame buffers of the group, and the pinned blocks of the slot's current set -> device pointer table.
int upload_ptrs(Slot& s, int n, const uint8_t* const* d_rgb, uint16_t* const* d_out) {
    PinnedSet& ps = s.pin();
    for (int i = 0; i < kMaxGroup; i++) {
        ps.h_ptrs[i] = (i < n && d_rgb) ? const_cast<uint8_t*>(d_rgb[i]) : nullptr;
        ps.h_ptrs[kMaxGroup + i] = (i < n && d_out) ? d_out[i] : nullptr;
    }
    ps.h_ptrs[kPtrStage] = ps.h_cl.get();
    ps.h_ptrs[kPtrExport] = ps.h_cl.get();
    ps.h_ptrs[kPtrStatus] = ps.h_misc.get();
    HIPCHK(hipMemcpyAsync(s.d_ptrs, ps.h_ptrs, sizeof(void*) * kPtrTable, hipMemcpyHostToDevice, s.st));
    return FSLIC_OK;
}

// Connectivity pass, fully asynchronous on the slot's stream: tile CCL, seams, compress, collect, device
// top-K + ranking, chain, relabel, for frames [i0, i0+n) (c = cca_view(s, i0, ...)).  The select status of every
// frame ends up in its misc words; cca_finish_group() serves the frames whose status is not 0.
void cca_enqueue(Slot& s, const CcaDev& c, int i0, int n, const ExportDev* ex) {
    (void)i0;
    launch_cca_phase1(c, n, s.st);
    launch_cca_select(c, n, s.st);
    launch_cca_phase2(c, n, s.st, ex);
}

// After the stream has been synchronised and h_misc refreshed.  The select kernel resolves the top-K step on the
// device, including an area tie at the cut (it replays libstdc++'s __heap_select).  Status 2 (more candidates than the
// device sorts): gather + sort on the host, frame by frame, then chain + relabel again for that frame.
int cca_finish_group(Slot& s, int first, int n, const uint16_t* d_in0, size_t in_stride, int K, int thres) {
    int n_slow = 0;
    for (int i = first; i < first + n; i++) n_slow += status(s, i)[kStSelect] == kSelectHost;
    if (n_slow == 0) return FSLIC_OK;
    for (int i = first; i < first + n && n_slow; i++) {
        const uint32_t* hm = status(s, i);
        if (hm[kStSelect] != kSelectHost) continue;
        const CcaDev c1 = cca_view(s, i, d_in0, in_stride, K, thres);
        int32_t* d_dl = s.at(s.c.cand_leader, i);      // dense (appended by k_cca_compress), unordered
        uint32_t* d_da = s.at(s.c.cand_area, i);
        const uint32_t M = hm[kStCands];
        const size_t cap = std::max<size_t>((size_t)M * 2, 16384);      // (two halves: the gathered list, then the same in leader order)
        int rc;
        if ((rc = s.h_cand_leader.reserve(cap)) || (rc = s.h_cand_area.reserve(cap))) return rc;
        launch_cca_gather_area(c1, s.st);
        HIPCHK(hipMemcpyAsync(s.h_cand_leader, d_dl, sizeof(int32_t) * M, hipMemcpyDeviceToHost, s.st));
        HIPCHK(hipMemcpyAsync(s.h_cand_area, d_da, sizeof(uint32_t) * M, hipMemcpyDeviceToHost, s.st));
        HIPCHK(hipStreamSynchronize(s.st));
        // ascending-leader order first (the device gathered tile by tile)
        std::vector<uint32_t> order(M);
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return s.h_cand_leader[a] < s.h_cand_leader[b]; });
        int32_t* sl = s.h_cand_leader + M;       // second half of the (2M-entry) host buffers
        uint32_t* sa = s.h_cand_area + M;
        for (uint32_t q = 0; q < M; q++) { sl[q] = s.h_cand_leader[order[q]]; sa[q] = s.h_cand_area[order[q]]; }
        // the kept list goes into the first halves of the pinned buffers (their content was moved to the second halves above)
        // and from there to the device on the slot's OWN stream: a copy on the default stream fails while another slot
        // of the engine was capturing its graph (stream capture is gone since: launch.h)
        int32_t* kl = s.h_cand_leader;
        uint16_t* kb = reinterpret_cast<uint16_t*>(s.h_cand_area.get());
        uint32_t n_keep = 0;
        select_kept_sorted(sl, sa, M, K, kl, kb, n_keep);
        int32_t* d_kl = s.at(s.d_keep_leader, i);
        uint16_t* d_kb = s.at(s.d_keep_label, i);
        if (n_keep) {
            HIPCHK(hipMemcpyAsync(d_kl, kl, sizeof(int32_t) * n_keep, hipMemcpyHostToDevice, s.st));
            HIPCHK(hipMemcpyAsync(d_kb, kb, sizeof(uint16_t) * n_keep, hipMemcpyHostToDevice, s.st));
        }
        launch_cca_set_kept(c1, d_kl, d_kb, (int)n_keep, s.st);
        launch_cca_phase2(c1, 1, s.st);
    }
    HIPCHK(hipStreamSynchronize(s.st));
    return FSLIC_OK;
}

// Host half of a group start: the integer part of the clamped centres (src/context.cpp:129-131,208-211,262) into the
// pinned staging block, and what the launch-timing events of this call will cover.  Nothing here touches the stream, so
// it runs on every call whether the device half below is enqueued directly or replayed as a graph.
void stage_group(fslic_engine* e, Slot& s, int i0, int n, bool timed) {
    const int H = s.H, W = s.W, K = s.K;
    for (int z = 0; z < n; z++) {
        const fslic_cluster* cl = s.clusters[i0 + z];
        uint32_t* h = s.pin().h_cl + (size_t)(i0 + z) * 4 * K;
        for (int k = 0; k < K; k++) {
            const int y = clampi((int)cl[k].y, 0, H - 1), x = clampi((int)cl[k].x, 0, W - 1);
            h[k] = ((uint32_t)y << 16) | (uint32_t)x;
        }
    }
    if (s.p.variant == FSLIC_VARIANT_REALDIST_NOQ) {      // assign()'s safeguard on the float position, src/context.cpp:208-211
        for (int z = 0; z < n; z++) {
            const fslic_cluster* cl = s.clusters[i0 + z];
            float* h = s.h_clf + (size_t)(i0 + z) * 8 * K;
            for (int k = 0; k < K; k++) {
                h[8 * k + 0] = clampf(cl[k].y, 0.0f, (float)(H - 1));
                h[8 * k + 1] = clampf(cl[k].x, 0.0f, (float)(W - 1));
                for (int q = 2; q < 8; q++) h[8 * k + q] = 0.0f;
            }
        }
    }
    if (timed) {
        s.n_timed_iters = 0; s.assign_loop_px = 0;
        const int stride = s.p.subsample_stride;
        int rem = 0;
        for (int it = 0; it < s.p.max_iter && s.launch_timing && it < Slot::kMaxTimedIters; it++) {
            s.n_timed_iters = it + 1;
            s.assign_loop_px += (double)visited_rows(H, rem, stride) * W * n;
            rem = (rem + 1) % stride;
        }
    }
}

// Whether a launch of `n` frames wants its cluster passes inside its assign launches (the per-cluster fused form, assign.hip:
// k_assign_bin): launches that do not fill the chip (FSLIC_FUSEBIN=1, the default) or all of them (=2), where every pass has rows.
static bool cluster_pass_fused(const Slot& s, int n) {
    const int stride = s.p.subsample_stride;
    const int assign_blocks = assign_blocks8(s.W, visited_rows(s.H, 0, stride), n);      // (the first pass's: launch_assign_fused_bin's own count)
#if defined(FSLIC_LAB) && FSLIC_LAB == 3
    // lab build 3 turns st_stream into plain stores; the fused cluster pass hands partial sums from block to block through
    // written-through (sc1) stores and agent-scope loads and would read stale lines of another XCD's L2: never fused there
    const bool fuse_wanted = false;
    (void)assign_blocks;
#else
    const bool fuse_wanted = knobs().fuse_bin == 2 || (knobs().fuse_bin == 1 && assign_blocks <= kBlocksFuseBin);
#endif
    // (H < stride: the passes of the residues >= H visit no row at all and launch nothing -- src/context.cpp:158-175 still runs update()
    // for them: every cluster's num_members becomes 0, positions stay; a cluster pass that rides on the assign blocks would not happen.
    // Found on a 71x1 frame, tests/fuzz_parity.py FUZZ_SHAPES=tiny seed 5 case 3100.)
    const bool every_pass_has_rows = s.H >= stride;
    return fuse_wanted && every_pass_has_rows;
}

// Whether the slot's current work may take the label-free passes at all: not under the sticky fallback of a slot that has had to redo a
// frame of this work (Slot::store_labels).
static bool label_free_allowed(const Slot& s) { return !s.store_labels; }

// What a launch asks of choose_passes beyond the slot's current work.  The defaults are a group's own launch; a frame redone because
// of a kernel flag asks for the conservative passes (group_complete).
struct ChoiceRequest {
    int count = 0;                   // frames of the launch: what the fusing rule is judged by
    bool force_generic = false;      // the generic kernel whatever the slot's geometry allows (a candidate list overflowed)
    bool allow_fused = true;         // false: the separate cluster pass
    bool allow_label_free = true;    // false: storing passes
};

// The ONE place where the passes of a launch are decided, from the slot's current work (geometry, parameters, Slot::generic,
// Slot::recording, the sticky fallback) and the request.  Everything here that no launch argument shows reaches the graph key with the
// value (launch_group).
static PassChoice choose_passes(const Slot& s, const ChoiceRequest& rq) {
    const fslic_params& p = s.p;
    const bool slic = p.variant == FSLIC_VARIANT_SLIC;
    const bool blk = blk_kernel_applies(s.f, p.subsample_stride);
    PassChoice c{};
    c.generic = s.generic || rq.force_generic;
    c.rec = s.recording && rq.count == 1;
    c.pre = p.preemptive != 0;
    c.lsc = p.variant == FSLIC_VARIANT_LSC;
    c.noq = p.variant == FSLIC_VARIANT_REALDIST_NOQ;
    c.rd_l2 = p.variant == FSLIC_VARIANT_REALDIST_L2;
    c.rd = p.variant == FSLIC_VARIANT_REALDIST || c.rd_l2 || c.noq;
    // the patch also where a preemptive Slic group falls back to the generic kernel for its subsampled passes (geometries outside the
    // block kernel: launch_assign_pre returns false)
    c.need_patch = c.generic || (c.pre && slic && !blk);
    // the cluster pass rides on the assign blocks of the integer SLIC path on the block kernel only
    c.fused = rq.allow_fused && slic && !c.pre && !c.generic && blk && cluster_pass_fused(s, rq.count);
    // The integer SLIC path on the block / 32-bit kernels resets the assignment plane lazily (FrameDev::fv_mod): the LAB kernel then
    // writes 4 B/px instead of 6; every other path -- variants, generic kernel, preemptive mode -- has the plane filled by the LAB kernel.
    // ... except under the fused cluster pass (launches that do not fill the chip: one or two frames per group): there every block drains
    // its label stores before it counts itself in, and stores into a plane the LAB kernel has just written find their lines in the
    // memory-side cache -- without the fill each of the ten launches of a one-frame group takes 0.35 us longer (8.54 against 8.18 us,
    // same-box A/B, profiles/r06_experiments.txt) for the 0.6 us the LAB kernel saves once.
    c.lazy_labels = slic && !c.generic && !c.pre && !c.fused;
    // Label-free group (DESIGN.md "Deferred labels"; FrameDev::fv_mod): the subsampled passes store no labels, the full pass defines the
    // whole plane.
    c.label_free = c.lazy_labels && rq.allow_label_free && label_free_allowed(s) && p.max_iter >= 1 && !s.recording && blk;
    assert(!(c.fused && c.lazy_labels));      // (the fused loop knows no first visits: first_visit_rule)
    return c;
}

// enforce_connectivity's minimum component size of the slot's current call, src/context.cpp:14-20
static int min_size_threshold(const Slot& s) { return (int)round((double)(s.S * s.S) * (double)s.p.min_size_factor); }

// ---- debug_mode: the recording path ----
// A call with debug_mode set (fslic_hip_iterate / fslic_hip_iterate_device; one frame) is enqueued directly, never as a graph, on the
// generic / unfused kernels with the label plane reset eagerly, and records what src/context.cpp:155-174 hands to its Recorder
// (src/recorder.h): snapshot -1 after the colour fetch, then one after every assign + update.  The assign launches of the loop take
// their recording forms, which write every visited pixel's minimum distance straight into the snapshot's distance plane (filled
// with the type's maximum beforehand: the reference resets min_dists over the whole frame in every assign(), src/context.cpp:199-205;
// snapshot -1's plane is the zeroed allocation of the reference, src/simd-helper.hpp:62-70).  After every cluster pass async copies
// put the label plane and the cluster state into the ring; the host reads the ring back once and formats the JSON.
// Ring: labels[nsnap][N] u16 | dists[nsnap][N] (u16 for Slic, f32 for the variants) | cluster state[nsnap][kRecWords * K] u32, the
// state as SoA: [0,K) position, [K,2K) colour, [2K,3K) num_members, [3K,4K) moved, [4K,5K) is_updatable, [5K,6K) is_active (preemptive
// mode), [6K,14K) the float centroids ('noq').
constexpr int kRecWords = 16;
struct RecLayout {
    size_t N, K, nsnap, dsize, dist_off, cl_off, bytes;
};
static RecLayout rec_layout(const Slot& s) {
    RecLayout L{};
    L.N = (size_t)s.H * s.W; L.K = (size_t)s.K; L.nsnap = (size_t)s.p.max_iter + 1;
    L.dsize = s.p.variant == FSLIC_VARIANT_SLIC ? 2 : 4;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L.dist_off = up(L.nsnap * L.N * 2);
    L.cl_off = L.dist_off + up(L.nsnap * L.N * L.dsize);
    L.bytes = L.cl_off + up(L.nsnap * kRecWords * L.K * 4);
    return L;
}

// ---- the device half of a group: enqueue_frames and its steps ----
#define FSLIC_TRY(expr) do { const int rc__ = (expr); if (rc__) return rc__; } while (0)

// Which frames of the slot's current group a call of enqueue_frames serves, and whether it brackets the phases with event records.
struct FramesRequest {
    int first = 0, count = 0;
    bool timed = false;
};
static FramesRequest frames(int first, int count) { FramesRequest rq; rq.first = first; rq.count = count; return rq; }
static FramesRequest timed_frames(int first, int count) { FramesRequest rq = frames(first, count); rq.timed = true; return rq; }

// What the steps of one enqueue_frames call share.
struct Enqueue {
    Slot& s;
    const PassChoice c;
    const int i0, n;
    const bool timed;
    FrameDev f;                      // the working copy every launch takes by value: frame i0's pointers, the pass's buffers and stamps
    LscDev l;
    // positions: the uploaded centres are in yx_up (s.f.cl_yx); every cluster pass reads one buffer and writes the other
    uint32_t *yx_up = nullptr, *yx_a = nullptr, *yx_b = nullptr;   // this frame's cl_yx, d_yx_alt[0], d_yx_alt[1]
    uint32_t* yx_cur = nullptr;      // where the last cluster pass put them
    int rem = 0;                     // the residue of the next subsampled pass's rows
    RecLayout rl{};                  // debug_mode: the snapshot ring
    float noq_coef = 0.0f, pre_l1_thres = 0.0f;
};

// FrameDev::fv_mod's rule (kernels.h) for a pass of the integer SLIC path on the block / 32-bit kernels: subsampled pass `it`, or the
// full pass (kFullPass).  The fused loop and the other families keep (0, 0): their plane is filled by the LAB kernel.
constexpr int kFullPass = -1;
static void first_visit_rule(FrameDev& f, const PassChoice& c, const fslic_params& p, int it) {
    const int stride = p.subsample_stride;
    if (it != kFullPass) {
        f.fv_mod = c.lazy_labels && it < stride ? 1 : 0; f.fv_from = 0;       // all of its rows, while the residues are new
    } else if (c.label_free) {
        // no pass has written the plane, EVERY row is a first visit; an uncovered pixel gets its 0xFFFF -- the plane is defined before the
        // connectivity kernels run -- and flags the frame
        f.fv_mod = 1; f.fv_from = 0;
    } else {
        // the rows of the residues no subsampled pass came to are first looked at by the full pass
        f.fv_mod = c.lazy_labels && p.max_iter < stride ? stride : 0; f.fv_from = p.max_iter < stride ? std::max(p.max_iter, 0) : 0;
    }
    f.fv_rcp = f.fv_mod > 1 ? 0xFFFFFFFFu / (uint32_t)f.fv_mod : 0u;
}

// debug_mode: snapshot `idx` (iteration idx - 1) of the label plane and the cluster state into the ring; rec_dist(idx) is the
// snapshot's distance plane, which the recording assign kernels write
static void* rec_dist(const Enqueue& q, int idx) { return q.c.rec ? q.s.d_rec + q.rl.dist_off + (size_t)idx * q.rl.N * q.rl.dsize : nullptr; }
static int snapshot(const Enqueue& q, int idx, const uint32_t* yx) {
    Slot& s = q.s;
    const FrameDev& f = q.f;
    const RecLayout& rl = q.rl;
    const int K = s.K;
    HIPCHK(hipMemcpyAsync(s.d_rec + (size_t)idx * rl.N * 2, f.labels, rl.N * 2, hipMemcpyDeviceToDevice, s.st));
    uint32_t* c = reinterpret_cast<uint32_t*>(s.d_rec + rl.cl_off) + (size_t)idx * kRecWords * K;
    const size_t kb = sizeof(uint32_t) * (size_t)K;
    HIPCHK(hipMemcpyAsync(c, yx, kb, hipMemcpyDeviceToDevice, s.st));
    HIPCHK(hipMemcpyAsync(c + K, f.cl_lab, kb, hipMemcpyDeviceToDevice, s.st));
    HIPCHK(hipMemcpyAsync(c + 2 * (size_t)K, f.cl_n, kb, hipMemcpyDeviceToDevice, s.st));
    HIPCHK(hipMemcpyAsync(c + 3 * (size_t)K, f.cl_moved, kb, hipMemcpyDeviceToDevice, s.st));
    if (q.c.pre) {
        HIPCHK(hipMemcpyAsync(c + 4 * (size_t)K, f.cl_upd, kb, hipMemcpyDeviceToDevice, s.st));
        HIPCHK(hipMemcpyAsync(c + 5 * (size_t)K, f.cl_act, kb, hipMemcpyDeviceToDevice, s.st));
    }
    if (q.c.noq) HIPCHK(hipMemcpyAsync(c + 6 * (size_t)K, f.cl_f, 8 * kb, hipMemcpyDeviceToDevice, s.st));
    return FSLIC_OK;
}

// The scaffolding of a subsampled pass, the same in the four loops.  assign_mark: per-launch timing, the event before (edge 0) and
// after (edge 1) the assign launch of pass `it`.  flip_positions: the coming cluster pass reads the current buffer and writes the other.
// end_pass: the cluster pass has been enqueued -- its output is current, the recorder takes its snapshot, the next pass's rows.
static int assign_mark(const Enqueue& q, int it, int edge) {
    if (q.timed && q.s.launch_timing && it < Slot::kMaxTimedIters) HIPCHK(hipEventRecord(q.s.ev_it[2 * it + edge], q.s.st));
    return FSLIC_OK;
}
static void flip_positions(Enqueue& q) { q.f.cl_yx = q.yx_cur; q.f.cl_yx_out = (q.yx_cur == q.yx_a) ? q.yx_b : q.yx_a; }
static int end_pass(Enqueue& q, int it) {
    q.yx_cur = q.f.cl_yx_out;
    if (q.c.rec) FSLIC_TRY(snapshot(q, it + 1, q.yx_cur));
    q.rem = (q.rem + 1) % q.s.p.subsample_stride;
    return FSLIC_OK;
}

// Patch upload, the preemptive and 'noq' initial state, LAB, the first cluster pass (reads the staged centres), the LSC prepare and the
// recorder's first snapshot.
static int prologue(fslic_engine* e, Enqueue& q) {
    Slot& s = q.s;
    const PassChoice& c = q.c;
    const fslic_params& p = s.p;
    FrameDev& f = q.f;
    const int K = s.K, S = s.S, i0 = q.i0, n = q.n;
    hipEvent_t* const ev = s.pin().ev;
    if (c.need_patch && !s.sp_patch_uploaded) {
        HIPCHK(hipMemcpyAsync(s.d_patch, s.h_patch, (size_t)(2 * S + 1) * (2 * S + 1) * sizeof(uint16_t), hipMemcpyHostToDevice, s.st));
        s.sp_patch_uploaded = true;
    }
    // cluster centres: staged by stage_group() into the pinned block the first cluster pass reads (no copy command)
    if (c.pre) {
        // PreemptiveGrid::initialize, src/preemptive.h:59-67: every counter = cooldown, everything active
        uint32_t* base = s.at(s.d_pre, i0);
        f.cl_upd = base; f.cl_act = base + K; f.cell_act = base + 2 * (size_t)K; f.pre_flags = f.cell_act + (size_t)f.pre_cw * f.pre_ch;
        for (int z = 0; z < n; z++) {
            uint32_t* bz = s.at(s.d_pre, i0 + z);
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)bz, 2, (size_t)K, s.st));                                   // cooldown
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(bz + 2 * (size_t)K + (size_t)f.pre_cw * f.pre_ch), 1, 1, s.st));   // all_active
        }
    }
    if (c.noq) {
        f.cl_f = s.at(s.d_clf, i0);
        HIPCHK(hipMemcpy2DAsync(f.cl_f, s.frame_bytes, s.h_clf + (size_t)i0 * 8 * K, sizeof(float) * 8 * (size_t)K,
                                sizeof(float) * 8 * (size_t)K, (size_t)n, hipMemcpyHostToDevice, s.st));
    }
    // sums, bin counters, flags and cl_n / cl_moved start from zero: cleared by the LAB kernel below (two memset launches less)

    if (q.timed) HIPCHK(hipEventRecord(ev[0], s.st));
    // + labels <- 0xFFFF (src/context.cpp:138-145) unless they are reset lazily; + a fresh range of bin generation stamps for this group's passes
    f.gen_base = s.d_gen;
    launch_rgb_to_lab(f, n, p.convert_to_lab, e->tables, !c.lazy_labels, s.st, s.gen_step,
                      s.at(s.zero_block, i0), s.zero_bytes, f.cl_n, 2 * (size_t)K,
                      reinterpret_cast<const uint32_t* const*>(s.d_ptrs + kPtrStage), (size_t)i0 * 4 * K, 4 * (size_t)K);      // (+ the staged centres -> cl_yx)
    if (q.timed) HIPCHK(hipEventRecord(ev[1], s.st));
    f.gen_off = 1;
    f.cl_yx = q.yx_up; f.cl_yx_out = q.yx_a;
    launch_bin_clusters(f, n, 0, 0, 0, PassGeom{}, s.st);      // (the centres are in cl_yx: copied from the host's staging block by the LAB kernel)
    q.yx_cur = q.yx_a;
    if (c.lsc) {
        q.l.select(i0);
        HIPCHK(clear_rows(s.lsc_zero + (size_t)i0 * s.lsc_frame_bytes, s.lsc_frame_bytes, s.lsc_zero_bytes, (size_t)n, s.st));
        launch_lsc_prepare(f, q.l, n, s.st);                      // before_iteration, src/lsc.cpp:12-15
    }
    if (c.rec) {
        // distance planes: -1 zero, 0 .. max_iter-1 the type's maximum; cluster state zero
        const RecLayout& rl = q.rl;
        HIPCHK(hipMemsetAsync(s.d_rec + rl.dist_off, 0, rl.N * rl.dsize, s.st));
        if (p.max_iter > 0) {
            if (rl.dsize == 2) HIPCHK(hipMemsetAsync(rec_dist(q, 1), 0xFF, (size_t)p.max_iter * rl.N * 2, s.st));
            else HIPCHK(hipMemsetD32Async((hipDeviceptr_t)rec_dist(q, 1), 0x7F7FFFFFu, (size_t)p.max_iter * rl.N, s.st));     // FLT_MAX
        }
        HIPCHK(hipMemsetAsync(s.d_rec + rl.cl_off, 0, rl.nsnap * kRecWords * rl.K * 4, s.st));
        FSLIC_TRY(snapshot(q, 0, q.yx_up));             // after the colour fetch, the label reset and before_iteration()
    }
    return FSLIC_OK;
}

// src/context.cpp:158-175, BaseContext<float>
static int float_distance_loop(Enqueue& q) {
    Slot& s = q.s;
    const PassChoice& c = q.c;
    const fslic_params& p = s.p;
    FrameDev& f = q.f;
    const int n = q.n, stride = p.subsample_stride;
    for (int it = 0; it < p.max_iter; it++) {
        flip_positions(q);
        FSLIC_TRY(assign_mark(q, it, 0));
        float* const dist = static_cast<float*>(rec_dist(q, it + 1));
        if (c.noq) launch_noq_assign(f, q.noq_coef, p.manhattan_spatial_dist != 0, n, q.rem, stride, it & 1, it & 1, true, s.st, dist);
        else launch_rd_assign(f, s.d_patchf, c.rd_l2, n, q.rem, stride, it & 1, it & 1, true, s.st, dist);
        FSLIC_TRY(assign_mark(q, it, 1));
        launch_member_sums(f, n, q.rem, stride, it & 1, c.noq ? 1 : 0, s.st);
        f.gen_off++;
        if (c.pre) launch_preempt_update(f, n, (it + 1) & 1, it & 1, false, q.pre_l1_thres, s.st);      // update() + set_new_clusters(), src/context.cpp:356-387
        else launch_bin_clusters(f, n, 1, (it + 1) & 1, it & 1, PassGeom{}, s.st);
        FSLIC_TRY(end_pass(q, it));
    }
    return FSLIC_OK;
}

// src/context.cpp:158-175 with ContextLSC's hooks
static int lsc_loop(Enqueue& q) {
    Slot& s = q.s;
    const PassChoice& c = q.c;
    FrameDev& f = q.f;
    const int n = q.n, stride = s.p.subsample_stride;
    for (int it = 0; it < s.p.max_iter; it++) {
        flip_positions(q);
        FSLIC_TRY(assign_mark(q, it, 0));
        launch_lsc_assign(f, q.l, n, q.rem, stride, it & 1, it & 1, !c.pre, s.st, static_cast<float*>(rec_dist(q, it + 1)));      // (preemptive: the assignment alone, the sums follow)
        FSLIC_TRY(assign_mark(q, it, 1));
        if (c.pre) {
            // update() under the activity state the pass started with, set_new_clusters(), then after_update() under the new one
            // (src/context.cpp:301-387, src/preemptive.h:114-178, src/lsc.cpp:226-307): lsc.hip, "preemptive mode"
            launch_lsc_pre_sums(f, n, q.rem, stride, it & 1, s.st);
            f.gen_off++;
            launch_preempt_update(f, n, (it + 1) & 1, it & 1, false, q.pre_l1_thres, s.st);
            launch_lsc_pre_feats(f, q.l, n, q.rem, stride, s.st);
        } else {
            f.gen_off++;
            launch_bin_clusters_lsc(f, q.l, n, (it + 1) & 1, it & 1, s.st);   // update() sums + after_update(), re-binning: one launch (everything is in FrameDev::sums)
        }
        FSLIC_TRY(end_pass(q, it));
    }
    return FSLIC_OK;
}

// The cluster pass between two assign passes (centroids from the sums, re-binning) is done by the assign kernel itself where
// the block kernel applies: its last block to deliver sums of a cluster finalises it (launch_assign_fused_bin), so the loop is
// max_iter launches instead of 2 * max_iter.  Positions then live in ONE buffer (yx_a, where the first cluster pass put them).
// Measured (profiles/r03_fused_cluster_pass.txt): one 1280x720 frame per group 168 instead of 183 us (the loop is ten launches
// of 9.9 us instead of twenty of 6.7 + 4.9), eight frames 315 instead of 333 us -- but the pipelined rate of 16-frame groups
// drops from 51.8 to 45.3 GP/s: the finaliser is a chain of dependent memory round trips at the end of every block and
// vector work a 1600-thread cluster pass does once.  So: fused where a launch does not fill the chip (latency-bound: the
// reference's own one-frame-per-call pattern), separate where it does.  FSLIC_FUSEBIN=0 / 2: never / always.
// Pass `it` reads spill list it % 3 and appends to (it + 1) % 3, which is the list the full pass reads (full_pass).
static int fused_slic_loop(Enqueue& q) {
    Slot& s = q.s;
    FrameDev& f = q.f;
    for (int it = 0; it < s.p.max_iter; it++) {
        f.cl_yx = q.yx_a; f.cl_yx_out = q.yx_a;
        FSLIC_TRY(assign_mark(q, it, 0));
        launch_assign_fused_bin(f, q.n, q.rem, s.p.subsample_stride, it, s.st);
        FSLIC_TRY(assign_mark(q, it, 1));
        f.gen_off++;
        FSLIC_TRY(end_pass(q, it));
    }
    return FSLIC_OK;
}

// src/context.cpp:158-175: the assign launch (which still sees the previous pass's buffers in f), then the flip and the cluster pass
static int slic_loop(Enqueue& q) {
    Slot& s = q.s;
    const PassChoice& c = q.c;
    FrameDev& f = q.f;
    const int n = q.n, stride = s.p.subsample_stride;
    for (int it = 0; it < s.p.max_iter; it++) {
        PassGeom pg{};
        FSLIC_TRY(assign_mark(q, it, 0));
        // (preemptive mode: the block kernel on the bins of the active clusters where the geometry takes it, round 5; until then the
        // generic kernel served every preemptive frame)
        first_visit_rule(f, c, s.p, it);
        if (c.rec) launch_assign_generic(f, n, q.rem, stride, it & 1, it & 1, true, s.st, static_cast<uint16_t*>(rec_dist(q, it + 1)));     // (rec: generic)
        else if (c.generic || (c.pre && !launch_assign_pre(f, n, q.rem, stride, it & 1, it & 1, s.st))) launch_assign_generic(f, n, q.rem, stride, it & 1, it & 1, true, s.st);
        else if (!c.pre) pg = launch_assign(f, n, q.rem, stride, it & 1, it & 1, true, s.st, -1, c.label_free);
        FSLIC_TRY(assign_mark(q, it, 1));
        f.gen_off++;
        flip_positions(q);
        if (c.pre) launch_preempt_update(f, n, (it + 1) & 1, it & 1, false, q.pre_l1_thres, s.st);     // update() + set_new_clusters()
        else launch_bin_clusters(f, n, 1, (it + 1) & 1, it & 1, pg, s.st);
        FSLIC_TRY(end_pass(q, it));
    }
    return FSLIC_OK;
}

// PreemptiveGrid::finalize (src/preemptive.h:69-74): every cluster takes part in the full assignment
static void preemptive_finalise(Enqueue& q) {
    q.f.gen_off++;
    q.f.cl_yx = q.yx_cur;
    launch_preempt_update(q.f, q.n, (q.s.p.max_iter + 1) & 1, 0, true, q.pre_l1_thres, q.s.st);
}

// full_assign: stride 1, rem 0, no update afterwards (src/context.cpp:246-256)
static void full_pass(Enqueue& q) {
    Slot& s = q.s;
    const PassChoice& c = q.c;
    const fslic_params& p = s.p;
    FrameDev& f = q.f;
    const int n = q.n;
    const int full_buf = (p.max_iter + (c.pre ? 1 : 0)) & 1;      // the bins of all clusters: the finalise has written one set more
    const int full_obuf = c.fused ? p.max_iter % 3 : -1;          // the spill list the fused loop's last pass appended to
    first_visit_rule(f, c, p, kFullPass);
    if (c.lsc) { f.cl_yx = q.yx_cur; launch_lsc_assign(f, q.l, n, 0, 1, full_buf, 0, false, s.st); }
    else if (c.noq) { f.cl_yx = q.yx_cur; launch_noq_assign(f, q.noq_coef, p.manhattan_spatial_dist != 0, n, 0, 1, full_buf, 0, false, s.st); }
    else if (c.rd) { f.cl_yx = q.yx_cur; launch_rd_assign(f, s.d_patchf, c.rd_l2, n, 0, 1, full_buf, 0, false, s.st); }
    else if (c.generic) launch_assign_generic(f, n, 0, 1, full_buf, 0, false, s.st);
    else (void)launch_assign(f, n, 0, 1, full_buf, 0, false, s.st, full_obuf, c.label_free);
}

// Connectivity, with the cluster state, overflow flag and connectivity status back to the host: the last kernel of the connectivity
// pass writes them into the pinned blocks of the group's set, which it finds in the pointer table (three 2-D copy commands per group
// before: blit kernels with their own barriers).  The status words are final once the select kernel has run, the cluster state
// since the loop ended.  Then the copies back of the variants' own state.
static int connectivity_and_export(Enqueue& q) {
    Slot& s = q.s;
    const int K = s.K, i0 = q.i0, n = q.n;
    const size_t fb = s.frame_bytes;
    const CcaDev c = cca_view(s, i0, s.f.labels, fb, K, min_size_threshold(s));
    ExportDev ex{};
    ex.frame_bytes = fb; ex.K = K; ex.yx_cur = q.yx_cur; ex.lab_n_moved = q.yx_up + K; ex.misc0 = s.at(s.d_misc, i0);
    ex.tab = reinterpret_cast<uint32_t* const*>(s.d_ptrs + kPtrExport);      // [0] kPtrExport, [1] kPtrStatus
    ex.h_off = (size_t)i0 * 4 * K; ex.h_stride = 4 * (size_t)K; ex.misc_off = (size_t)kStatusWords * i0;
    cca_enqueue(s, c, i0, n, &ex);
    if (q.timed) HIPCHK(hipEventRecord(s.pin().ev[4], s.st));
    if (q.c.pre) HIPCHK(hipMemcpy2DAsync(s.h_upd + (size_t)i0 * K, sizeof(uint32_t) * (size_t)K, q.f.cl_upd, fb,
                                         sizeof(uint32_t) * (size_t)K, (size_t)n, hipMemcpyDeviceToHost, s.st));
    if (q.c.noq) HIPCHK(hipMemcpy2DAsync(s.h_clf + (size_t)i0 * 8 * K, sizeof(float) * 8 * (size_t)K, q.f.cl_f, fb,
                                         sizeof(float) * 8 * (size_t)K, (size_t)n, hipMemcpyDeviceToHost, s.st));
    return FSLIC_OK;
}

// Device half: everything of iterate() for the frames `rq` names of the slot's current group, on the passes `c` (choose_passes),
// enqueued asynchronously on the slot's stream.  Pure stream work with no per-call values in any launch argument (caller pointers sit
// in the device pointer table, bin generations come from device memory), so the same sequence can be recorded once as a graph and
// replayed (launch_group).
static int enqueue_frames(fslic_engine* e, Slot& s, const PassChoice& c, const FramesRequest& rq) {
    const fslic_params& p = s.p;
    // copies the graph recorder has no node for (launch.h): such a group is always enqueued directly
    if ((c.pre || c.noq || (c.need_patch && !s.sp_patch_uploaded)) && recording_unsupported()) return FSLIC_OK;
    Enqueue q{s, c, rq.first, rq.count, rq.timed, s.f, s.l};
    if (c.rec) q.rl = rec_layout(s);
    q.f.rgbs = nullptr;
    q.f.select(rq.first);                          // host-side: pointers of frame `first`
    q.f.rgbs = reinterpret_cast<const uint8_t* const*>(s.d_ptrs + rq.first);
    q.yx_up = q.f.cl_yx;
    q.yx_a = q.yx_up + 6 * (size_t)s.K;
    q.yx_b = q.yx_up + 7 * (size_t)s.K;
    q.noq_coef = 1.0f / ((float)s.S / p.compactness);        // src/context.cpp:463-464
    q.noq_coef *= (1 << (p.convert_to_lab ? 1 : 0));
    q.pre_l1_thres = std::max(roundf(2 * s.S * p.preemptive_thres), 1.0f);      // src/preemptive.h:129
    hipEvent_t* const ev = s.pin().ev;

    FSLIC_TRY(prologue(e, q));
    if (c.rd) FSLIC_TRY(float_distance_loop(q));
    else if (c.lsc) FSLIC_TRY(lsc_loop(q));
    else if (c.fused) FSLIC_TRY(fused_slic_loop(q));
    else FSLIC_TRY(slic_loop(q));
    if (c.pre) preemptive_finalise(q);
    if (rq.timed) HIPCHK(hipEventRecord(ev[2], s.st));
    full_pass(q);
    if (rq.timed) HIPCHK(hipEventRecord(ev[3], s.st));
    return connectivity_and_export(q);
}

GraphRecorder*& current_recorder() {
    static thread_local GraphRecorder* rec = nullptr;
    return rec;
}

// The device half of a group start, replayed from a graph when this exact sequence has been seen before.  `c`: the passes it chose.
static int launch_group(fslic_engine* e, Slot& s, int n, PassChoice& c) {
    s.last_launch_mode = 0;
    ChoiceRequest want;
    want.count = n;
    c = choose_passes(s, want);
    {   // Bin slots are validated by a u32 generation stamp; a group uses max_iter + 3 consecutive values above the base
        // (device word *d_gen, mirrored here).  Long before it could wrap, start over: stamps and base back to zero.
        // The base moves past the stamps of the PREVIOUS group at the start of this one (a group of fewer iterations after one
        // of more would otherwise meet the earlier group's stamps inside its own range and take stale bin slots for live).
        const uint64_t span = (uint64_t)s.p.max_iter + 3u;
        if (s.gen_host + 2 * (s.gen_span_prev + span) >= 0xC0000000ull) {
            HIPCHK(hipMemsetAsync(s.d_gen, 0, 256, s.st));
            HIPCHK(hipMemset2DAsync(s.stamp_block, s.frame_bytes, 0, s.stamp_bytes, (size_t)s.cap_frames, s.st));
            s.gen_host = 0;
        }
        s.gen_step = s.gen_span_prev ? s.gen_span_prev : (uint32_t)span;     // (first group of the slot: any step does)
        s.gen_span_prev = (uint32_t)span;
        s.gen_host += s.gen_step;
    }
    // Per-launch timing wants real event records between the launches; events replayed inside a graph keep the time
    // stamps of an earlier execution.  Timed groups therefore take the direct path.
    // (debug_mode: the recording path, always direct)
    if (s.recording || !knobs().use_graphs || s.launch_timing) return enqueue_frames(e, s, c, timed_frames(0, n));
    // everything a launch argument can depend on, and the choice of the passes itself
    std::vector<unsigned char> key;
    auto put = [&](const void* p, size_t bytes) { const unsigned char* b = (const unsigned char*)p; key.insert(key.end(), b, b + bytes); };
    const int hdr[7] = {s.H, s.W, s.K, s.S, n, (int)s.gen_step, s.sp_patch_uploaded ? 1 : 0};
    // (the pinned blocks of the group's set are not among them: the kernels read their addresses from the pointer table, one sequence serves both sets)
    const void* const ptrs[7] = {s.d_ptrs, s.h_patch, s.d_gen, s.lsc_zero, s.d_patchf, s.h_clf, s.h_upd};   // baked into copy nodes / arguments
    put(hdr, sizeof hdr); put(&c, sizeof c); put(ptrs, sizeof ptrs); put(&s.p, sizeof s.p); put(&s.f, sizeof s.f); put(&s.c, sizeof s.c);
    if (s.p.variant == FSLIC_VARIANT_LSC) put(&s.l, sizeof s.l);
    Slot::GraphEntry* ge = nullptr;
    for (auto& g : s.graphs) if (g.key == key) { ge = &g; break; }
    if (!ge) {
        if (s.graphs.size() >= 8) {                  // keep the cache small: drop the oldest entry
            if (s.graphs.front().exec) hipGraphExecDestroy(s.graphs.front().exec);
            if (s.graphs.front().graph) hipGraphDestroy(s.graphs.front().graph);
            s.graphs.erase(s.graphs.begin());
        }
        s.graphs.emplace_back();
        ge = &s.graphs.back();
        ge->key = key;
        // The sticky fallback of the label-free passes changes the key.  The group that caused it was enqueued directly and its flagged
        // frames were redone with the storing kernels, which is all a first sighting is for: the storing sequence of the same work is
        // recorded on its first group, not on its second (a slot that serves three groups of such a work still reaches the replay).
        if (s.store_seen_credit && s.store_labels) ge->seen = 1;
        s.store_seen_credit = false;
    }
    if (!ge->exec) {
        if (ge->failed || ge->seen++ == 0) return enqueue_frames(e, s, c, timed_frames(0, n));   // first sighting: direct (also warms one-time setup)
        // second sighting: the same calls with a recorder current on this thread build the graph, node by node (launch.h)
        GraphRecorder rec;
        if (hipGraphCreate(&rec.graph, 0) != hipSuccess) { ge->failed = true; (void)hipGetLastError(); return enqueue_frames(e, s, c, timed_frames(0, n)); }
        current_recorder() = &rec;
        const int rc = enqueue_frames(e, s, c, frames(0, n));     // no event records inside the graph
        current_recorder() = nullptr;
        if (rc != FSLIC_OK || rec.err != hipSuccess || rec.nodes == 0 || hipGraphInstantiate(&ge->exec, rec.graph, nullptr, nullptr, 0) != hipSuccess) {
            hipGraphDestroy(rec.graph);
            ge->exec = nullptr; ge->failed = true;
            (void)hipGetLastError();
            if (rc != FSLIC_OK) return rc;
            return enqueue_frames(e, s, c, timed_frames(0, n));
        }
        ge->graph = rec.graph;
        s.last_launch_mode = 1;
    } else {
        s.last_launch_mode = 2;
    }
    // the whole group between two real event records: total device time stays available, the per-phase split does not
    HIPCHK(hipEventRecord(s.pin().ev[0], s.st));
    HIPCHK(hipGraphLaunch(ge->exec, s.st));
    HIPCHK(hipEventRecord(s.pin().ev[4], s.st));
    return FSLIC_OK;
}

// testing aid (fslic_hip_debug_fail_group): whether this passage of point `what` by a slot thread's group is the one that fails
static bool debug_fail_here(fslic_engine* e, const Slot& s, int what) {
    if (!s.nap_wait || e->debug_fail_what.load(std::memory_order_relaxed) != what) return false;
    if (e->debug_fail_after.fetch_sub(1) != 0) return false;
    e->debug_fail_what.store(-1);
    return true;
}

int group_begin(fslic_engine* e, Slot& s, const GroupJob& job, bool record) {
    const double t_begin = now_us();
    const fslic_params* p = &job.p;
    const int H = job.H, W = job.W, K = job.K, n = job.n;
    int S = 0;
    s.recording = false;
    int rc = check_job(job, S);
    if (rc) return rc;
    if (record && n != 1) return fail(FSLIC_E_INTERNAL, "a recording group holds one frame");
    if (debug_fail_here(e, s, 0)) return fail(FSLIC_E_INTERNAL, "testing aid: group_begin failed before it touched the slot");
    rc = ensure_prepared(e, s, H, W, K, S, n);           // (carves for at least the engine's batching reserve)
    if (rc) return rc;
    const int cap_frames = s.cap_frames;
    s.par ^= 1;                      // the other set: the previous group may still be running on its own (a slot thread's successor)
    s.H = H; s.W = W; s.K = K; s.S = S; s.p = *p; s.nframes = n;
    // the sticky fallback of the label-free passes belongs to one work
    if (s.store_labels && !same_work(s.store_work, job)) { s.store_labels = false; s.store_seen_credit = false; }
    std::copy(job.clusters, job.clusters + n, s.clusters);
    rc = configure_spatial(s, S, p);
    if (rc) return rc;
    if (p->variant == FSLIC_VARIANT_LSC) {
        rc = prepare_lsc(s, H, W, K, S, cap_frames, p->compactness);
        if (rc) return rc;
    }
    if (p->variant == FSLIC_VARIANT_REALDIST || p->variant == FSLIC_VARIANT_REALDIST_L2) {
        rc = configure_patchf(s, S, p);
        if (rc) return rc;
    }
    if (p->variant == FSLIC_VARIANT_REALDIST_NOQ && (rc = s.h_clf.reserve((size_t)s.cap_frames * K * 8))) return rc;
    rc = upload_ptrs(s, n, job.d_rgb, job.d_out);
    if (rc) return rc;
    if (record) {
        s.rec_clusters.assign(job.clusters[0], job.clusters[0] + K);
        s.recording = true;       // (before rec_layout: it reads s.H, s.W, s.K, s.p)
        const size_t need = rec_layout(s).bytes;
        if (s.d_rec.reserve(need)) {
            (void)hipGetLastError();
            s.recording = false;
            return fail(FSLIC_E_HIP, "debug_mode: hipMalloc of the snapshot ring (" + std::to_string(need) + " bytes) failed");
        }
    }
    s.generic = p->variant == FSLIC_VARIANT_SLIC && (e->lab_force_generic.load() != 0 || !s.sp_tiled_ok || record);
    if (p->preemptive && (rc = s.h_upd.reserve((size_t)s.cap_frames * K))) return rc;
    stage_group(e, s, 0, n, true);
    PassChoice choice{};
    rc = launch_group(e, s, n, choice);
    if (rc) return rc;
    if (debug_fail_here(e, s, 1)) return fail(FSLIC_E_INTERNAL, "testing aid: group_begin failed after it enqueued the group");
    s.have_pre = true;
    s.last_path = s.generic ? 1 : 0;
    InFlight& g = s.fl[s.par];
    g.job = job; g.S = S; g.par = s.par; g.choice = choice; g.launch_mode = s.last_launch_mode;
    g.t_begun_us = now_us();
    if (knobs().host_timing) {
        fprintf(stderr, "[fslic host] group_begin n=%d: %.1f us | slot %d begin %.1f .. %.1f\n", n, now_us() - t_begin, (int)(&s - e->slots.data()), t_begin, now_us());
        s.t_begun_us = now_us();
    }
    return FSLIC_OK;
}

// The shortest of the slot thread's last four flight times (from the return of group_begin to the group's completion) for the
// workload of `g`; 1e30: none yet.  The history belongs to ONE workload: after a switch from long groups (16 x 4K: ~10 ms) to short ones
// (0.15 ms) the first short groups would otherwise sleep 5, 2.5, 1.25 .. ms before the minimum converged.
static double shortest_flight(Slot& s, const InFlight& g) {
    const GroupJob& j = g.job;
    const unsigned long long key = ((unsigned long long)(uint32_t)j.H << 48) ^ ((unsigned long long)(uint32_t)j.W << 32) ^ ((unsigned long long)(uint32_t)j.K << 16) ^
                                   ((unsigned long long)(uint32_t)j.n << 8) ^ ((unsigned long long)(uint32_t)j.p.max_iter << 4) ^ (unsigned long long)(uint32_t)j.p.variant ^
                                   ((unsigned long long)(uint32_t)j.p.preemptive << 60) ^ ((unsigned long long)(uint32_t)j.p.subsample_stride << 56);
    if (key != s.recent_wait_key) {
        s.recent_wait_key = key;
        for (double& w : s.recent_wait_us) w = 1e30;
    }
    double shortest = 1e30;
    for (double w : s.recent_wait_us) shortest = std::min(shortest, w);
    return shortest;
}

// Sleep through the first half of the shortest flight, then look at `ev` every ten microseconds until it is complete or `deadline_us` has passed.
static int nap_poll(const InFlight& g, hipEvent_t ev, double shortest, double deadline_us, bool& done) {
    auto nap = [](double us) { struct timespec ts; ts.tv_sec = 0; ts.tv_nsec = (long)(us * 1000.0); nanosleep(&ts, nullptr); };
    if (shortest < 1e29 && shortest * 0.5 > 30.0) {
        const double rest = std::min(g.t_begun_us + std::min(shortest * 0.5, 20000.0), deadline_us) - now_us();
        if (rest > 1.0) nap(rest);
    }
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        done = q == hipSuccess;
        if (done) return FSLIC_OK;
        if (q != hipErrorNotReady) return fail(FSLIC_E_HIP, std::string("hipEventQuery: ") + hipGetErrorString(q));
        if (now_us() >= deadline_us) return FSLIC_OK;
        nap(10.0);
    }
}

// Completion of everything enqueued on the slot's stream, for a slot's OWN host thread (the submit / drain pipeline): hipStreamSynchronize
// spins, and six slot threads spinning cost a rank 0.77 ms of CPU per 0.153 ms step (five cores; forty on an 8-GPU node).  Here the
// thread sleeps through the first half of the wait -- half of the SHORTEST of its last four flights, so that a group that finishes
// sooner than its predecessors (the pipeline draining) is not slept past -- and then looks at an event behind the stream's work every
// ten microseconds (the slot threads run with a timer slack of 1 us, pipeline.cpp).  A synchronous caller's thread keeps the spin:
// its timer slack is its own, and one frame per call is a latency measurement.
// (`successor`: the slot's thread has already enqueued the group's successor.  The event is then the group's OWN end event: one recorded
// at the stream's tail, or a stream synchronisation, would wait for the successor as well.)
static int nap_wait(Slot& s, const InFlight& g, bool successor) {
    const hipEvent_t ev = s.set[g.par].ev[successor ? 4 : 5];
    if (!successor) HIPCHK(hipEventRecord(ev, s.st));
    bool done = false;
    const int rc = nap_poll(g, ev, shortest_flight(s, g), 1e300, done);
    if (rc) return rc;
    s.recent_wait_us[s.recent_wait_i++ & 3] = now_us() - g.t_begun_us;
    return FSLIC_OK;
}

constexpr double kOverlapMaxFlightUs = 4000.0;
// How long before the expected end of the running group its thread looks for a successor: the host's part of a group start (~100 us)
// with room to spare.  The same for every slot, NOT a share of the flight: streams that share a hardware queue fly twice as long as
// those that have one to themselves, and with a proportional lead their threads looked -- and took the last submissions of a burst --
// before the threads of the faster slots did.
constexpr double kSuccessorLeadUs = 200.0;

// For a slot thread with `g` running and nothing behind it: waits -- in nap_wait's manner, on the group's own end event -- until the group
// is complete or only the last part of its expected flight is left, which is when the thread looks for a successor.  Committing a
// submission to this slot's stream any earlier would take it from a slot that becomes free sooner (the end of a burst: the slots that
// finish first take what is left, as they do without overlap); any later and the stream runs dry.  false: no history of this workload
// yet, the group is finished without a successor.
bool group_prewait(Slot& s, const InFlight& g, int& rc) {
    rc = FSLIC_OK;
    const double shortest = shortest_flight(s, g);
    if (shortest > 1e29) return false;
    // What a successor saves is the host's part between two groups, some 100 us.  Beside a flight of several milliseconds that is below
    // what a measurement resolves, and two such groups queued on every stream cost more than it: 16 x 3840x2160 per group (flights of
    // ~9 ms) ran 1 % slower with successors than without (profiles/r15_overlapped_groups.txt).  Such groups are finished one by one.
    if (shortest > kOverlapMaxFlightUs) return false;
    bool done = false;
    rc = nap_poll(g, s.set[g.par].ev[4], shortest, g.t_begun_us + shortest - kSuccessorLeadUs, done);
    return rc == FSLIC_OK;
}

int group_wait(Slot& s, InFlight& g, bool successor) {
    PinnedSet& ps = s.set[g.par];
    if (successor) {
        const int rc = nap_wait(s, g, true);
        if (rc) return rc;
        HIPCHK(hipEventSynchronize(ps.ev[4]));      // (complete: returns at once)
    } else {
        if (s.nap_wait) { const int rc = nap_wait(s, g, false); if (rc) return rc; }
        HIPCHK(hipStreamSynchronize(s.st));
    }
    auto elapsed = [](float& ms, hipEvent_t a, hipEvent_t b) { if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { ms = 0; (void)hipGetLastError(); } };
    elapsed(s.total_ms, ps.ev[0], ps.ev[4]);
    g.total_ms = s.total_ms;
    if (g.launch_mode == 0) {
        elapsed(s.lab_ms, ps.ev[0], ps.ev[1]);
        elapsed(s.loop_ms, ps.ev[1], ps.ev[2]);
        elapsed(s.fa_ms, ps.ev[2], ps.ev[3]);
        elapsed(s.cca_ms, ps.ev[3], ps.ev[4]);
    } else {
        s.lab_ms = s.loop_ms = s.fa_ms = s.cca_ms = 0;       // graph replay: only the group total is event-timed
    }
    s.assign_loop_ms = 0;
    for (int it = 0; it < s.n_timed_iters; it++) {           // (per-launch timing: never with a successor enqueued)
        float ms = 0;
        elapsed(ms, s.ev_it[2 * it], s.ev_it[2 * it + 1]);
        s.assign_loop_ms += ms;
    }
    return FSLIC_OK;
}

bool group_needs_host(const Slot& s, const InFlight& g) {
    for (int i = 0; i < g.job.n; i++) {
        const uint32_t* hm = status(s, g.par, i);
        if (hm[kStSelect] == kSelectHost || (!g.choice.generic && hm[kStFlags] != 0)) return true;
    }
    return false;
}

// After a successor has been finished and collected: the slot's per-call state, its current set and the device pointer table are
// those of `g` again, so that frames of `g` can be enqueued once more (same work, same prepared buffers: what group_begin set up
// beyond these still stands).
int make_current(Slot& s, const InFlight& g) {
    const GroupJob& j = g.job;
    s.par = g.par;
    s.H = j.H; s.W = j.W; s.K = j.K; s.S = g.S; s.p = j.p; s.nframes = j.n;
    s.generic = g.choice.generic; s.recording = false;
    std::copy(j.clusters, j.clusters + j.n, s.clusters);
    return upload_ptrs(s, j.n, j.d_rgb, j.d_out);
}

// Frame `i` of the slot's current group once more, alone and to completion, on the passes `c`: from the caller's Cluster[K] block, with
// generation stamps past those of the pass just made (same span).
static int redo_frame(fslic_engine* e, Slot& s, int i, const PassChoice& c) {
    stage_group(e, s, i, 1, false);
    s.gen_step = s.gen_span_prev;
    s.gen_host += s.gen_step;
    const int rc = enqueue_frames(e, s, c, frames(i, 1));
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s.st));
    return FSLIC_OK;
}

int group_complete(fslic_engine* e, Slot& s, InFlight& g, bool from_scratch) {
    if (debug_fail_here(e, s, 2)) return fail(FSLIC_E_INTERNAL, "testing aid: group_complete failed before the write-back");
    const double t_ev = now_us();
    const GroupJob& job = g.job;
    const fslic_params& p = job.p;
    const int n = job.n, K = job.K, H = job.H, W = job.W;
    const PinnedSet& ps = s.set[g.par];
    int n_host_topk = 0;
    for (int i = 0; i < n; i++) n_host_topk += status(s, g.par, i)[kStSelect] == kSelectHost;
    // The host steps work on the slot's current group (stage_group, enqueue_frames, cca_finish_group read the slot): a caller with a
    // successor on the stream has finished that one first and made `g` current again (make_current).
    const bool host_steps = group_needs_host(s, g);
    if (host_steps && s.par != g.par) return fail(FSLIC_E_INTERNAL, "host steps of a group that is not the slot's current one");
    const int thres = min_size_threshold(s);
    for (int i = 0; host_steps && i < n; i++) {
        const uint32_t* hm = status(s, i);
        // A successor's kernels have run over the device state of this group.  A frame that only wants the host's top-K step has no
        // candidate lists left to gather: it is computed again the way the group ran it, and takes the steps below from there.
        if (from_scratch && hm[kStSelect] == kSelectHost && (s.generic || hm[kStFlags] == 0)) {
            const int rc = redo_frame(e, s, i, g.choice);      // (the group's own choice, not a one-frame launch's)
            if (rc) return rc;
        }
        // Flags of the tiled kernels.  kFlagStalePixel: a visited pixel that no window covered kept its label while the cluster pass was
        // fused into the assign kernel (its sums reached the owner through global atomics that nothing orders before the owner's
        // finaliser): that frame alone is redone with the separate cluster pass.  kFlagListOverflow: a block's candidate list overflowed: that
        // frame alone is redone with the generic kernel.  kFlagUncoveredPixel: a pass of a label-free group met a visited pixel no window
        // covered (the one place where an earlier pass's label is needed): that frame alone is redone with storing passes, and the slot keeps
        // to them for this work.  (Every redo starts from the caller's Cluster[K] block, which is written only below: it serves a group
        // whose device state is gone just as well.)
        for (int attempt = 0; attempt < 2 && !s.generic && hm[kStFlags] != 0; attempt++) {
            const bool overflow = (hm[kStFlags] & kFlagListOverflow) != 0;
            const bool uncovered = (hm[kStFlags] & kFlagUncoveredPixel) != 0;
            // (an overflowing block assigns nothing, so later passes of that attempt work on centres that may well leave pixels uncovered:
            // the flag then is a by-product, the redo is the generic one, and neither the counter nor the slot's fallback is concerned)
            if (uncovered && !overflow) {
                if (!s.store_labels) s.store_seen_credit = true;
                s.store_labels = true; s.store_work = job;
                __atomic_fetch_add(&s.n_uncovered_redo, 1, __ATOMIC_RELAXED);      // (read by fslic_hip_uncovered_redos without the engine lock)
            }
            if (knobs().host_timing) fprintf(stderr, "[fslic host] frame %d redone with %s\n", i, overflow ? "the generic kernel (candidate-list overflow)" : uncovered ? "storing assign passes (uncovered pixel)" : "the separate cluster pass (stale pixel)");
            // the conservative passes: separate cluster pass, storing, generic where the candidate list overflowed
            ChoiceRequest want;
            want.count = 1; want.force_generic = overflow; want.allow_fused = false; want.allow_label_free = false;
            const int rc = redo_frame(e, s, i, choose_passes(s, want));
            if (rc) return rc;
            if (overflow) {
                if (hm[kStFlags] != 0) return fail(FSLIC_E_INTERNAL, "generic path reported a candidate overflow");
                s.last_path = 1;
            } else if (!uncovered) {
                __atomic_fetch_add(&s.n_separate_redo, 1, __ATOMIC_RELAXED);      // (read by fslic_hip_separate_pass_redos without the engine lock)
            }
        }
        if (!s.generic && hm[kStFlags] != 0) return fail(FSLIC_E_INTERNAL, "a redone frame still carries a kernel flag");
    }
    if (host_steps) {
        int rc = cca_finish_group(s, 0, n, s.f.labels, s.frame_bytes, K, thres);
        if (rc) return rc;
    }
    s.n_host_topk = g.n_host_topk = n_host_topk;
    const double t_cca = now_us();
    // write the cluster state back the way the reference leaves it
    const bool noq = p.variant == FSLIC_VARIANT_REALDIST_NOQ;
    for (int i = 0; i < n; i++) {
        const uint32_t* yx = ps.h_cl + (size_t)i * 4 * K;
        const uint32_t* lab = yx + K;
        const uint32_t* nm = yx + 2 * (size_t)K;
        const uint32_t* moved = yx + 3 * (size_t)K;
        fslic_cluster* cl = job.clusters[i];
        for (int k = 0; k < K; k++) {
            cl[k].r = (float)(lab[k] & 255u);                 // src/context.cpp:132-134 / :370-372
            cl[k].g = (float)((lab[k] >> 8) & 255u);
            cl[k].b = (float)((lab[k] >> 16) & 255u);
            const float* c = noq ? s.h_clf + ((size_t)i * K + k) * 8 : nullptr;
            if (moved[k] && c) { cl[k].r = c[2]; cl[k].g = c[3]; cl[k].b = c[4]; }      // src/context.cpp:374-380
            cluster_position(moved[k] != 0, yx[k], c, cl[k], H, W, cl[k].y, cl[k].x);
            if (p.max_iter > 0) cl[k].num_members = nm[k];  // src/context.cpp:362
            cl[k].is_updatable = p.preemptive ? (uint8_t)s.h_upd[(size_t)i * K + k] : 2;   // src/preemptive.h:59-67, :131-139
            cl[k].is_active = 1;                               // src/preemptive.h:69-74
        }
    }
    if (knobs().host_timing)
        fprintf(stderr, "[fslic host] group_complete n=%d slot %d .. %.1f: host steps (%d frames for top-K) %.1f us, write-back %.1f us (device %.1f us)\n",
                n, (int)(&s - e->slots.data()), now_us(), n_host_topk, t_cca - t_ev, now_us() - t_cca, s.total_ms * 1e3);
    return FSLIC_OK;
}

// Wait for the slot's current group, serve the rare host-side steps frame by frame (candidate-list overflow -> generic redo, more
// connectivity candidates than the device sorts -> std::partial_sort on the host), then write the cluster state back.
int group_finish(fslic_engine* e, Slot& s) {
    const double t_begin = now_us();
    InFlight& g = s.fl[s.par];
    int rc = group_wait(s, g, false);
    if (rc) return rc;
    if (knobs().host_timing) fprintf(stderr, "[fslic host] group_finish n=%d slot %d at %.1f: wait + events %.1f us\n", g.job.n, (int)(&s - e->slots.data()), t_begin, now_us() - t_begin);
    return group_complete(e, s, g, false);
}

void drain_failed(Slot& s) {
    const std::string msg = last_error();
    (void)hipStreamSynchronize(s.st);
    (void)hipGetLastError();
    set_last_error(msg);
}

int run_group(fslic_engine* e, Slot& s, const GroupJob& job, bool record) {
    int rc = group_begin(e, s, job, record);
    if (rc == FSLIC_OK) rc = group_finish(e, s);
    if (rc != FSLIC_OK) drain_failed(s);
    return rc;
}

// BaseContext::get_timing_report (src/context.h:74) in the fstimer schema (src/timer.cpp:4-18), durations from the
// HIP events of the slot's last group.  The report belongs to the calling thread, like the reference's thread_local
// timer (src/timer.cpp:45): concurrent iterate() calls on different models do not overwrite each other's report.
std::string make_timing_report(const Slot& s) {
    char buf[1024];
    auto us = [](float ms) { return (long long)(ms * 1000.0f); };
    snprintf(buf, sizeof buf,
             "{\"name\": \"iterate\", \"duration\": %lld, \"children\": ["
             "{\"name\": \"cielab_conversion\", \"duration\": %lld, \"children\": []},"
             "{\"name\": \"assign_update_loop\", \"duration\": %lld, \"children\": []},"
             "{\"name\": \"full_assign\", \"duration\": %lld, \"children\": []},"
             "{\"name\": \"enforce_connectivity\", \"duration\": %lld, \"children\": []}]}",
             us(s.total_ms), us(s.lab_ms), us(s.loop_ms), us(s.fa_ms), us(s.cca_ms));
    return buf;
}

namespace {
thread_local std::string t_timing;
thread_local std::string t_recorder;

// Numbers as std::stringstream << prints them (src/recorder.h): integers in decimal, floats as printf's %g at precision 6 (what
// to_chars does with chars_format::general and a precision).  Every call has room for the longest form.
inline char* put_u(char* o, uint64_t v) { return std::to_chars(o, o + 24, v).ptr; }
inline char* put_i(char* o, int64_t v) { return std::to_chars(o, o + 24, v).ptr; }
inline char* put_f(char* o, float v) { return std::to_chars(o, o + 32, (double)v, std::chars_format::general, 6).ptr; }
inline char* put_s(char* o, const char* s) { const size_t n = strlen(s); memcpy(o, s, n); return o + n; }
inline char* header(char* o, int H, int W) {
    o = put_s(o, "{\"height\": "); o = put_i(o, H);
    o = put_s(o, ", \"width\": "); o = put_i(o, W);
    return put_s(o, ", \"snapshots\": [");
}
}  // namespace

void set_thread_timing_report(const std::string& json) { t_timing = json; }
const std::string& thread_timing_report() { return t_timing; }
void set_thread_recorder_report(std::string&& json) { t_recorder = std::move(json); }
const std::string& thread_recorder_report() { return t_recorder; }

// RecorderSnapshot::gen / Recorder::gen (src/recorder.h) over the ring of the slot's last call, after group_finish.  The Cluster view of
// a snapshot is the reference's Cluster[K] at that moment: snapshot -1 holds the caller's block with the fetched colours and
// is_updatable = cooldown (PreemptiveGrid::initialize, src/preemptive.h:59-66); after an update a cluster sits where cluster_position()
// says, as in the write-back of group_finish.
int make_recorder_report(Slot& s, std::string& out) {
    const int H = s.H, W = s.W, K = s.K;
    if (!s.recording) {
        char buf[96];
        char* o = header(buf, H, W);
        o = put_s(o, "]}");
        out.assign(buf, o);
        return FSLIC_OK;
    }
    const RecLayout L = rec_layout(s);
    std::vector<char> ring(L.bytes);
    HIPCHK(hipMemcpyAsync(ring.data(), s.d_rec, L.bytes, hipMemcpyDeviceToHost, s.st));
    HIPCHK(hipStreamSynchronize(s.st));
    const bool pre = s.p.preemptive != 0, noq = s.p.variant == FSLIC_VARIANT_REALDIST_NOQ;
    const size_t per_dist = L.dsize == 2 ? 6 : 16;       // ",65535" / ",3.40282e+38"
    out.resize(96 + L.nsnap * (96 + L.K * 320 + L.N * (6 + per_dist)));
    char* const o0 = &out[0];
    char* o = header(o0, H, W);
    const fslic_cluster* const cin = s.rec_clusters.data();
    for (size_t i = 0; i < L.nsnap; i++) {
        if (i) *o++ = ',';
        o = put_s(o, "{\"iteration\": "); o = put_i(o, (int64_t)i - 1);
        o = put_s(o, ", \"clusters\": [");
        const uint32_t* c = reinterpret_cast<const uint32_t*>(ring.data() + L.cl_off) + i * kRecWords * L.K;
        for (int k = 0; k < K; k++) {
            const fslic_cluster& a = cin[k];
            const uint32_t lab = c[K + k];
            float y = a.y, x = a.x, r = (float)(lab & 255u), g = (float)((lab >> 8) & 255u), b = (float)((lab >> 16) & 255u);
            uint32_t upd = 2, act = a.is_active, nm = a.num_members;
            if (i > 0) {
                const bool moved = c[3 * (size_t)K + k] != 0;
                const float* cf = noq ? reinterpret_cast<const float*>(c + 6 * (size_t)K) + 8 * (size_t)k : nullptr;
                if (moved && cf) { r = cf[2]; g = cf[3]; b = cf[4]; }
                cluster_position(moved, c[k], cf, a, H, W, y, x);
                nm = c[2 * (size_t)K + k];
                if (pre) { upd = c[4 * (size_t)K + k]; act = c[5 * (size_t)K + k]; }
            }
            if (k) *o++ = ',';
            o = put_s(o, "{\"yx\": ["); o = put_f(o, y); *o++ = ','; o = put_f(o, x);
            o = put_s(o, "], \"color\": ["); o = put_f(o, r); *o++ = ','; o = put_f(o, g); *o++ = ','; o = put_f(o, b);
            o = put_s(o, "], \"is_updatable\": "); o = put_u(o, (uint8_t)upd);
            o = put_s(o, ", \"is_active\": "); o = put_u(o, (uint8_t)act);
            o = put_s(o, ", \"number\": "); o = put_u(o, a.number);
            o = put_s(o, ", \"num_members\": "); o = put_u(o, nm);
            *o++ = '}';
        }
        o = put_s(o, "], \"assignment\": [");
        const uint16_t* lb = reinterpret_cast<const uint16_t*>(ring.data()) + i * L.N;
        for (size_t q = 0; q < L.N; q++) {
            if (q) *o++ = ',';
            o = put_u(o, lb[q]);
        }
        o = put_s(o, "], \"min_dists\": [");
        if (L.dsize == 2) {
            const uint16_t* d = reinterpret_cast<const uint16_t*>(ring.data() + L.dist_off) + i * L.N;
            for (size_t q = 0; q < L.N; q++) {
                if (q) *o++ = ',';
                o = put_u(o, d[q]);
            }
        } else {
            const float* d = reinterpret_cast<const float*>(ring.data() + L.dist_off) + i * L.N;
            for (size_t q = 0; q < L.N; q++) {
                if (q) *o++ = ',';
                o = put_f(o, d[q]);
            }
        }
        o = put_s(o, "]}");
    }
    o = put_s(o, "]}");
    out.resize((size_t)(o - o0));
    return FSLIC_OK;
}

}  // namespace fslic
