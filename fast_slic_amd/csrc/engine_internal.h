// engine_internal.h -- shared declarations of the host engine's translation units (internal to the library).
//
//   tables.cpp      RGB->LAB tables, spatial patch and its device encodings (src/cielab.h, src/context.cpp:22-40)
//   arena.cpp       per-slot device / pinned buffers: allocation, carving, release
//   group.cpp       one launch group: staging, the launch sequence (direct or as a hipGraph), completion, write-back
//   pipeline.cpp    slot ownership (synchronous calls, asynchronous groups, the submit/drain pipeline), slot threads
//   capi.cpp        the C ABI of include/fslic_hip.h for iterate() and friends
//   host_utils.cpp  O(K) host functions and the stage / superpixel-graph entry points
//
// The engine replaces, for the arch "hip/gfx950", what SlicModel.iterate builds per call in the reference: a Context
// (src/context.h:59-66), initialize_state(), iterate() (src/context.cpp:108-197) and its teardown
// (cfast_slic.pyx:171-197).  Device and pinned buffers are owned here and cached across calls; the only state that
// carries over between calls is the caller's Cluster[K].
#pragma once
#include "kernels.h"
#include "launch.h"
#include "../../include/fslic_hip.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace fslic {

// ---- errors: thread-local message, integer status (no exception crosses the ABI) ----
int fail(int code, const std::string& msg);
const std::string& last_error();
void set_last_error(const std::string& msg);

#define HIPCHK(expr)                                                                            \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return ::fslic::fail(FSLIC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
inline float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
double now_us();

// ---- buffers that own themselves: pinned host (Pinned<T>) or device (Device<T>) memory that grows on demand, is released with its
// owner and reads as the T* it holds.  Move-only. ----
template <class T, bool kDevice>
class Buffer {
    T* p_ = nullptr;
    size_t cap_ = 0;                 // elements
public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buffer& operator=(Buffer&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
    ~Buffer() { release(); }
    operator T*() const { return p_; }
    T* get() const { return p_; }
    void release() {
        if (p_) (void)(kDevice ? hipFree(p_) : hipHostFree(p_));
        p_ = nullptr; cap_ = 0;
    }
    // room for `count` elements (never shrinks; the content is NOT kept when it grows; at least 16 bytes, so that a held buffer is never NULL)
    int reserve(size_t count) {
        if (p_ && cap_ >= count) return FSLIC_OK;
        release();
        const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
        const hipError_t err = kDevice ? hipMalloc((void**)&p_, bytes) : hipHostMalloc((void**)&p_, bytes);
        if (err != hipSuccess) {
            p_ = nullptr;
            return fail(FSLIC_E_HIP, std::string(kDevice ? "hipMalloc(" : "hipHostMalloc(") + std::to_string(bytes) + " bytes): " + hipGetErrorString(err));
        }
        cap_ = count;
        return FSLIC_OK;
    }
};
template <class T> using Pinned = Buffer<T, false>;
template <class T> using Device = Buffer<T, true>;

// One work: a geometry under one parameter set.  Frames of the same work share launch groups (pipeline.cpp), a running group may be
// followed by one of the same work (may_follow), and the sticky fallback of the label-free passes belongs to one (Slot::store_work).
struct Work {
    fslic_params p{};
    int H = 0, W = 0, K = 0;
};
inline bool same_work(const Work& a, const Work& b) {
    return a.H == b.H && a.W == b.W && a.K == b.K && memcmp(&a.p, &b.p, sizeof(fslic_params)) == 0;
}

// One group request as the C entry points receive it: up to kMaxGroup frames of one work.
struct GroupJob : Work {
    int n = 0;
    const uint8_t* d_rgb[kMaxGroup] = {};
    fslic_cluster* clusters[kMaxGroup] = {};
    uint16_t* d_out[kMaxGroup] = {};
    // the frames of `j` behind this job's (the caller has made sure that they fit and ask for the same work)
    void append(const GroupJob& j) {
        for (int i = 0; i < j.n; i++) { d_rgb[n + i] = j.d_rgb[i]; clusters[n + i] = j.clusters[i]; d_out[n + i] = j.d_out[i]; }
        n += j.n;
    }
};

// Environment switches, read ONCE when the library is loaded (never on a call path).
//   FSLIC_GROUP        frames per launch group of fslic_hip_iterate_batch (default 8, at most 16)
//   FSLIC_GRAPH=0      enqueue every group operation by operation instead of replaying a recorded hipGraph
//   FSLIC_POISON       testing aid: fill a freshly carved arena with 0xA5 (reads of never-written memory show up)
//   FSLIC_HOST_TIMING  one stderr line per group start / completion with host-side durations
//   FSLIC_FUSEBIN      the cluster pass between two assign passes: 1 (default) fused into the assign kernel for launches that do
//                      not fill the chip and a separate launch (k_bin_clusters<1>) otherwise; 0 always separate (round 2; also what
//                      a frame with a stale pixel is redone with); 2 always fused (A/B measurements)
//   FSLIC_BLOCKS_SCALE testing aid: an integer >= 1 (default 1) that multiplies assign_blocks8 (kernels.h), the launch size every
//                      rows-per-wavefront and fusing rule is compared with, and nothing else: a small frame then takes the kernel
//                      forms of a chip-filling launch (tests/test_gpu_assign_forms.py)
struct Knobs {
    int group_size;
    bool use_graphs, poison, host_timing;
    int fuse_bin;
    int blocks_scale;
};
const Knobs& knobs();

constexpr int kDenseCap = 8192;          // candidates the select kernel resolves on the device (== its LDS sort capacity)
constexpr size_t kTabMaxBytes = 40960;   // LDS budget of the packed kernel's spatial table (row-vector mode: per table)
constexpr size_t kLutMaxWords = 12288;   // 48 KB of LDS for the spatial table at most

// Host copies of the RGB->LAB tables (src/cielab.h:296-305), built once per process.
struct HostTables {
    uint16_t gamma[256];
    uint16_t lab[8194];
    int cb[9];
};
const HostTables& host_tables();

// The device pointer table of a group (Slot::d_ptrs, copied per group by upload_ptrs): the callers' frame buffers, then the pinned blocks
// of the group's set -- where its first kernel finds the staged centres and its last kernel puts the cluster state and the status words.
constexpr int kPtrStage = 2 * kMaxGroup, kPtrExport = kPtrStage + 1, kPtrStatus = kPtrStage + 2, kPtrTable = kPtrStage + 3;

// What a group owns on the host from its begin to its finish, twice per slot: while group N of a slot is still running, the slot's thread
// stages and enqueues N + 1 on the other set (pipeline.cpp).  Nothing recorded in a graph names a set: the kernels take the blocks from
// the pointer table.
struct PinnedSet {
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // 0..4 bracket the phases (4: the group's end), 5: nap_wait's
    // pinned host (device-accessible: the first kernel reads the centres from it, the export blocks of the last kernel write the
    // results into it -- no copy commands in a group's launch sequence)
    Pinned<uint32_t> h_cl;           // per frame 4K words: in [0,K) yx; out (yx, lab, n, moved)
    Pinned<uint32_t> h_misc;         // per frame its status words as the export left them: status(s, frame)
    Pinned<void*> h_ptrs;            // the source of the pointer table's asynchronous copy
};

// What enqueue_frames runs for a launch beyond the values of its launch arguments: decided once per launch by choose_passes (group.cpp),
// part of the graph key byte by byte (all members are bool: no padding), and kept by the group (InFlight::choice).
struct PassChoice {
    // the family: which assign loop runs, and on which kernels
    bool generic;                    // the brute-force gather kernel (k_assign_generic) for the integer SLIC path
    bool rec;                        // debug_mode: the recording forms and a snapshot after every cluster pass
    bool pre;                        // preemptive mode
    bool lsc;                        // the LSC loop
    bool rd, rd_l2, noq;             // the float-distance loop (RealDist, RealDistL2, RealDistNoQ), and which of its kinds
    bool need_patch;                 // the (2S+1)^2 patch of the generic kernel has to be on the device
    bool fused;                      // the cluster passes run inside the assign launches (launch_assign_fused_bin)
    bool lazy_labels;                // the LAB kernel leaves the label plane alone, first visits reset it (FrameDev::fv_mod)
    bool label_free;                 // the subsampled passes store no labels at all (DESIGN.md "Deferred labels")
};

// A group between group_begin and its completion: everything the finish needs, so that the slot's per-call state may already be that
// of the next group.
struct InFlight {
    GroupJob job;                    // geometry, parameters, frames, the callers' buffers and Cluster[K] blocks
    int S = 0;
    int par = 0;                     // its PinnedSet
    PassChoice choice{};             // what its begin chose: a frame computed again from scratch runs the same passes
    int launch_mode = 0;             // Slot::last_launch_mode of its begin
    double t_begun_us = 0;           // when group_begin returned (nap_wait's history counts from here)
    // what its finish found, for whoever collects it (the slot's own fields of the same names belong to the group finished LAST)
    float total_ms = 0;
    int n_host_topk = 0;
};

struct Slot {
    hipStream_t st = nullptr;
    PinnedSet set[2];
    int par = 0;                     // the set of the current (last begun) group; group_begin takes the other one
    InFlight fl[2];                  // by set
    PinnedSet& pin() { return set[par]; }
    const PinnedSet& pin() const { return set[par]; }
    // HIP events bracketing every subsampled assign launch of the loop (the roofline figure of bench.py sums them)
    static constexpr int kMaxTimedIters = 16;
    hipEvent_t ev_it[2 * kMaxTimedIters] = {};
    int n_timed_iters = 0;
    float assign_loop_ms = 0;        // sum of the fused assign launches' durations of the last group
    double assign_loop_px = 0;       // pixels those launches visited (all frames of the group)
    // device: one arena = [shared spatial tables][frame 0][frame 1]...; f / c hold frame 0's pointers
    Device<char> arena;
    int cap_frames = 0;              // frames the arena is carved for
    size_t frame_bytes = 0;
    FrameDev f{};
    CcaDev c{};
    // per-frame regions, given as frame 0's pointers (frame i: + i * frame_bytes)
    char* zero_block = nullptr;
    size_t zero_bytes = 0;
    char* stamp_block = nullptr;     // the bin slots' generation stamps (cleared when carved and when the stamps wrap)
    size_t stamp_bytes = 0;
    uint32_t* d_misc = nullptr;      // frame 0's status words (kernels.h, StatusWord)
    uint32_t* d_yx_alt[2] = {nullptr, nullptr};   // the cluster pass's alternating position buffers (frame 0)
    uint8_t* d_rgb_stage = nullptr;
    uint16_t* d_out_stage = nullptr;
    int32_t* d_keep_leader = nullptr;
    uint16_t* d_keep_label = nullptr;
    // per-frame caller pointers of the current group: [0, kMaxGroup) inputs, [kMaxGroup, 2*kMaxGroup) outputs
    Device<void*> d_ptrs;            // device copy, kPtrTable entries (allocated with the slot; pinned staging: PinnedSet::h_ptrs)
    // shared tables
    uint16_t* d_patch = nullptr;
    uint32_t* d_lut = nullptr;
    Pinned<uint32_t> h_lut;
    uint16_t* d_tab = nullptr;
    Pinned<uint16_t> h_tab;
    Pinned<uint16_t> h_patch;
    Pinned<int32_t> h_cand_leader;   // the host top-K step's candidates (cca_finish_group)
    Pinned<uint32_t> h_cand_area;
    Device<uint32_t> d_gen;          // device word: base of the bin generation stamps (FrameDev::gen_base)
    uint64_t gen_host = 0;           // host mirror of *d_gen
    uint32_t gen_span_prev = 0;      // stamps the previous group used above its base (max_iter + 3): what the next group's first kernel adds to *d_gen
    uint32_t gen_step = 0;           // ... for the group being enqueued
    int keyH = 0, keyW = 0, keyK = 0;
    // Recorded launch sequences (hipGraph, launch.h), one per distinct (geometry, options, group size, arena carving): a group
    // start is ~45 stream operations at ~3 us of host time each when enqueued one by one, ~8 us as one graph launch
    // (scripts/microbench/graph_launch.hip).  A key is recorded the second time it is seen.
    struct GraphEntry {
        std::vector<unsigned char> key;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        int seen = 0;
        bool failed = false;
    };
    std::vector<GraphEntry> graphs;
    int last_launch_mode = 0;        // 0 direct, 1 recorded this call, 2 replayed
    bool launch_timing = false;      // the engine's flag as it stood when this slot's current group was submitted
    double t_begun_us = 0;           // FSLIC_HOST_TIMING: when group_begin returned
    // the slot's own host thread waits for a group by sleeping and polling instead of spinning (group.cpp, nap_wait)
    bool nap_wait = false;           // set for groups served by the slot thread
    double recent_wait_us[4] = {1e30, 1e30, 1e30, 1e30};   // its last four flights: group_begin's return to completion (1e30: none yet)
    unsigned recent_wait_i = 0;
    unsigned long long recent_wait_key = 0;   // the workload those waits belong to (geometry, group size, iterations, variant): another one starts a new history
    // per-call state
    int H = 0, W = 0, K = 0, S = 0;
    int nframes = 0;
    bool generic = false;
    fslic_params p{};
    fslic_cluster* clusters[kMaxGroup] = {};      // the group's Cluster[K] blocks (its frame buffers live in the device pointer table)
    float total_ms = 0, fa_ms = 0, lab_ms = 0, loop_ms = 0, cca_ms = 0;
    int last_path = 0;
    int n_host_topk = 0;             // frames of the last group whose top-K step ran on the host
    int n_separate_redo = 0;         // (accessed with __atomic builtins) frames (since the slot was created) redone with the separate cluster pass because of a stale pixel
    // Label-free passes (group.cpp, choose_passes): once a frame of this slot had to be redone because a visited pixel lay outside every
    // window, the slot keeps to the storing passes for that work (same_work) -- a stream of scattered warm starts pays the redo once,
    // not in every group; another work starts afresh.
    int n_uncovered_redo = 0;        // (accessed with __atomic builtins) frames (since the slot was created) redone with storing passes because of kFlagUncoveredPixel
    bool store_labels = false;       // the sticky fallback is in force for store_work
    bool store_seen_credit = false;  // the fallback has just begun: the group that caused it counts as the first sighting of the storing sequence (launch_group)
    Work store_work;
    bool have_pre = false;
    // Ownership (guarded by fslic_engine::mu): `busy` while a synchronous call or a stage utility runs on the slot,
    // `pending` from the submission of an asynchronous group until it has been collected.
    bool busy = false;
    bool pending = false;
    int wanted = 0;                  // synchronous callers waiting for THIS slot (fslic_hip_iterate_device with a slot number): its thread leaves the submit queue alone meanwhile
    // asynchronous groups run on the slot's own host thread (launches, stream sync, cluster write-back), so the host
    // work of one slot overlaps that of the others
    struct Async {
        std::thread worker;
        bool has_job = false, done = false, quit = false;      // guarded by fslic_engine::mu
        GroupJob job;
        int rc = 0;
        std::string err;
        bool from_queue = false;      // the job was taken from the engine's submit queue (the thread collects it itself)
        int jobs = 0;                 // ... and is this many submissions in one group
    };
    std::unique_ptr<Async> async;
    uint32_t* d_pre = nullptr;       // frame 0's preemptive state: is_updatable[K], is_active[K], cells, flags
    Pinned<uint32_t> h_upd;          // is_updatable counters back from the device, per frame K words
    float* d_clf = nullptr;          // frame 0's float centroids ('noq')
    Pinned<float> h_clf;             // per frame K * 8 floats: upload (y, x) / download (y, x, r, g, b)
    // float-distance variants: f32 spatial patch (shared region of the arena) and its pinned staging
    float* d_patchf = nullptr;
    Pinned<float> h_patchf;
    int pf_S = 0, pf_shift = -1, pf_variant = -1;
    float pf_compactness = -1.0f;
    bool pf_manhattan = true;
    // LSC variant: own arena = [shared tables][frame 0][frame 1]...; l holds frame 0's pointers
    Device<char> lsc_arena;
    size_t lsc_frame_bytes = 0, lsc_zero_bytes = 0;
    char* lsc_zero = nullptr;
    LscDev l{};
    Pinned<float> h_lsc_lut;         // staging of the tables: [4][256] colour, [2][W], [2][H]
    int lsc_H = 0, lsc_W = 0, lsc_K = 0, lsc_G = 0, lsc_S = 0;
    float lsc_compactness = -1.0f;
    // cached spatial configuration (configure_spatial)
    bool sp_valid = false, sp_tiled_ok = false, sp_manhattan = true, sp_patch_uploaded = false;
    int sp_S = 0, sp_shift = 0, sp_stride = 0;
    float sp_compactness = 0.0f;
    // debug_mode (group.cpp, "the recording path"): the snapshot ring of the current call (RecLayout), grown on demand and kept
    bool recording = false;          // the current group is a recording one-frame call
    Device<char> d_rec;
    std::vector<fslic_cluster> rec_clusters;   // the caller's Cluster block as it came in (snapshot -1, the unmoved positions)

    template <class T> T* at(T* p, int frame) const { return reinterpret_cast<T*>(reinterpret_cast<char*>(p) + (size_t)frame * frame_bytes); }
};

// the status words of frame `frame` of the slot's current group, or of the group that owns set `par` (host copy)
inline uint32_t* status(const Slot& s, int frame) { return s.pin().h_misc + (size_t)kStatusWords * frame; }
inline uint32_t* status(const Slot& s, int par, int frame) { return s.set[par].h_misc + (size_t)kStatusWords * frame; }

// Where the reference leaves a cluster after an update (src/context.cpp:368-380): one that has moved (an update with members) at its
// integer centre `yx` (y << 16 | x) or, for 'noq', at its float centroid (y, x; NULL otherwise); one that has not at the caller's
// position `in`, clamped by assign()'s safeguard (src/context.cpp:208-211).
inline void cluster_position(bool moved, uint32_t yx, const float* centroid, const fslic_cluster& in, int H, int W, float& y, float& x) {
    if (moved && centroid) { y = centroid[0]; x = centroid[1]; }
    else if (moved) { y = (float)(yx >> 16); x = (float)(yx & 0xFFFFu); }
    else { x = clampf(in.x, 0.0f, (float)(W - 1)); y = clampf(in.y, 0.0f, (float)(H - 1)); }
}

}  // namespace fslic

struct fslic_engine {
    int device = 0;
    int group_size = 8;              // frames per launch group of iterate_batch (FSLIC_GROUP)
    bool launch_timing = false;      // bracket every subsampled assign launch with HIP events (fslic_hip_set_launch_timing)
    std::vector<fslic::Slot> slots;
    fslic::Device<uint16_t> d_gamma, d_labtbl;
    fslic::LabTables tables{};
    // slot ownership and the completion of asynchronous groups
    std::mutex mu;
    std::condition_variable cv;        // callers: a slot has become free, a group is complete, the queue has room, everything has drained
    std::condition_variable cv_work;   // the slot threads: a job has been handed over, the queue has work, a slot may serve the queue again, quit
                                       // (two variables so that a submission does not wake the callers and a completion does not wake the idle slot threads)
    // the submit / drain pipeline (fslic_hip_pipeline_*): first error of a collected group, totals since the last drain
    int pipe_rc = 0;
    std::string pipe_err;
    double pipe_device_ms = 0;
    long long pipe_groups = 0, pipe_frames = 0, pipe_host_topk = 0;
    // Submissions wait here for a slot thread (guarded by mu).  With batching on (fslic_hip_pipeline_batching), a thread
    // that finds several compatible submissions waiting serves them as ONE group: fewer, fuller launches when the
    // caller submits faster than the device finishes.
    std::deque<fslic::GroupJob> pipe_q;
    int pipe_inflight = 0;           // groups taken from the queue and not yet collected
    int pipe_batch_frames = 0;       // 0: one submission per group; otherwise the most frames a group may gather
    bool pipe_gathering = false;     // a slot thread is waiting briefly for a companion of the submission it took
    double pipe_last_submit_us = 0;  // (mu) when the last submission arrived: a companion is only waited for while submissions are arriving
    std::atomic<int> reserve_frames{0};   // arenas are carved for at least this many frames per group
    int sync_waiters = 0;                    // (mu) synchronous callers waiting for ANY slot (or all of them): the slot threads leave the submit queue alone meanwhile
    std::atomic<bool> pipe_overlap{true};          // fslic_hip_pipeline_overlap: off, the slot threads finish every group before they begin the next one (the serial loop)
    std::atomic<long long> overlapped_groups{0};   // groups begun while their slot's previous group had not been collected (fslic_hip_overlapped_groups)
    std::atomic<int> lab_force_generic{0};
    // testing aid (fslic_hip_debug_fail_group): the slot threads' groups pass point `debug_fail_what` (-1: none) `debug_fail_after` more times, then one fails there
    std::atomic<int> debug_fail_what{-1}, debug_fail_after{0};   // testing aid (fslic_hip_lab_force_generic): the brute-force gather kernels instead of the tiled ones
};

// Testing aid, exported but deliberately NOT part of include/fslic_hip.h: every following group of the Slic variant on this engine
// runs the brute-force gather kernel (k_assign_generic) instead of the tiled one -- the tests' independent cross-check.
extern "C" int fslic_hip_lab_force_generic(fslic_engine* e, int on);
// Testing aid, exported and NOT part of include/fslic_hip.h either: after `after` more groups of the slot threads have passed the point
// `what`, the next one fails there with FSLIC_E_INTERNAL, once.  0: group_begin before it touches the slot; 1: group_begin after the group
// has been enqueued (its kernels run; the slot's current set is the failed group's); 2: group_complete before the host steps and the
// write-back.  Nothing on the device goes wrong: the error paths of the submit / drain pipeline run without a fault.  -1: disarm.
extern "C" int fslic_hip_debug_fail_group(fslic_engine* e, int what, int after);

namespace fslic {

// ---- tables.cpp ----
int configure_spatial(Slot& s, int S, const fslic_params* p);
int configure_patchf(Slot& s, int S, const fslic_params* p);

// ---- arena.cpp ----
void free_slot(Slot& s);
int prepare(fslic_engine* e, Slot& s, int H, int W, int K, int S, int G);
int ensure_prepared(fslic_engine* e, Slot& s, int H, int W, int K, int S, int G);
// whether ensure_prepared would leave the slot's buffers as they are
bool prepared_for(const fslic_engine* e, const Slot& s, int H, int W, int K, int G);
int prepare_lsc(Slot& s, int H, int W, int K, int S, int G, float compactness);

// ---- group.cpp ----
int validate(const fslic_params* p, int H, int W, int K, int& S);
// An entry point's arguments as a job (what cannot be copied -- a missing array or parameter block -- is refused here), and what every
// group is checked for: its size, validate(), no frame pointer NULL.  Both run on the caller's thread.
int fill_job(GroupJob& j, const fslic_params* p, int H, int W, int K, int n,
             const uint8_t* const* d_rgb, fslic_cluster* const* clusters, uint16_t* const* d_out);
int check_job(const GroupJob& j, int& S);
int upload_ptrs(Slot& s, int n, const uint8_t* const* d_rgb, uint16_t* const* d_out);
CcaDev cca_view(const Slot& s, int i0, const uint16_t* d_in0, size_t in_stride, int K, int min_threshold);
void cca_enqueue(Slot& s, const CcaDev& c, int i0, int n, const ExportDev* ex = nullptr);
int cca_finish_group(Slot& s, int first, int n, const uint16_t* d_in0, size_t in_stride, int K, int thres);
// record: the recording path of debug_mode (one frame; only fslic_hip_iterate / fslic_hip_iterate_device ask for it)
int group_begin(fslic_engine* e, Slot& s, const GroupJob& job, bool record = false);
int group_finish(fslic_engine* e, Slot& s);
// The halves of group_finish, for a slot thread that has already begun the group's successor (pipeline.cpp).  group_wait: the group's
// completion and its event times; with `successor` it waits for the group's own end event and leaves the stream alone.
// group_needs_host: a frame came back with a kernel flag or for the host's top-K step.  group_complete: those host steps, then the
// write-back of the Cluster[K] blocks; `from_scratch`: the device state of the group is gone (a successor has run over it), the frames
// concerned are computed again first.  The host steps need the group to be the slot's current one (make_current) and the stream idle.
int group_wait(Slot& s, InFlight& g, bool successor);
bool group_prewait(Slot& s, const InFlight& g, int& rc);      // (group.cpp: when a slot thread looks for a successor)
bool group_needs_host(const Slot& s, const InFlight& g);
int make_current(Slot& s, const InFlight& g);
int group_complete(fslic_engine* e, Slot& s, InFlight& g, bool from_scratch);
// After a failure on the slot's stream: waits until nothing touches the caller's buffers any more; the error message survives.
void drain_failed(Slot& s);
// One group from start to completion: group_begin, group_finish, and drain_failed if either fails.
int run_group(fslic_engine* e, Slot& s, const GroupJob& job, bool record = false);
std::string make_timing_report(const Slot& s);
void set_thread_timing_report(const std::string& json);
const std::string& thread_timing_report();
// The recorder report of a completed call (src/recorder.h): the ring of a recording call read back and formatted, the header
// alone otherwise.  Kept per calling thread like the timing report.
int make_recorder_report(Slot& s, std::string& out);
void set_thread_recorder_report(std::string&& json);
const std::string& thread_recorder_report();

// ---- pipeline.cpp ----
// Synchronous calls take a slot for their duration (they wait while every slot is taken; a slot with an uncollected
// asynchronous group is never handed out).  `want` >= 0 asks for that slot.
int acquire_slot(fslic_engine* e, int want, int& slot);
int acquire_all_slots(fslic_engine* e);
void release_slot(fslic_engine* e, int slot);
void release_all_slots(fslic_engine* e);
void stop_slot_thread(fslic_engine* e, Slot& s);
struct SlotLease {               // RAII: one slot for the length of a scope
    fslic_engine* e;
    int slot = -1;
    explicit SlotLease(fslic_engine* e_) : e(e_) {}
    int take(int want = -1) { return acquire_slot(e, want, slot); }
    ~SlotLease() { if (slot >= 0) release_slot(e, slot); }
};

}  // namespace fslic
