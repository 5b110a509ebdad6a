/* fslic_hip.h -- C ABI of the MI355X (gfx950) SLIC superpixel engine.
 *
 * This is the drop-in boundary for ONE hot path of Algy/fast-slic: fast_slic.Slic.iterate()
 * (RGB->CIELAB prepass, subsampled assign/update loop, full assign, connectivity/min-size pass).
 * Every entry point names the reference interface it replaces; paths are relative to the
 * reference repository root.  Plain C types only: no C++ or torch types cross this boundary.
 *
 * Threading (cfast_slic.pyx:188-193 releases the GIL around the calls replaced here, and the reference's
 * per-call Context makes concurrent iterate() calls on different models legal): every entry point may be
 * called from any thread at any time.  A call needs one of the engine's n_slots slots (a HIP stream and
 * its buffers); synchronous calls take a free slot for their duration and wait while all are taken, so
 * up to n_slots calls run concurrently on one engine and further ones queue.  A slot that owns a group
 * submitted with fslic_hip_submit_group is handed to nobody until fslic_hip_wait_group has collected it.
 * The timing report and the error message are per calling thread.  The library never calls into Python.
 *
 * All functions returning int return 0 on success and a non-zero FSLIC_E_* code on failure;
 * fslic_hip_last_error() then returns a thread-local human-readable message.  No exception
 * crosses the ABI (the reference maps C++ exceptions through Cython `except +`, cfast_slic.pxd:47,51).
 */
#ifndef FSLIC_HIP_H
#define FSLIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSLIC_HIP_ARCH_NAME "hip/gfx950"   /* new entry for archtbl[], src/context-impl.cpp:15-24 */

enum {
    FSLIC_OK = 0,
    FSLIC_E_INVALID = 1,       /* bad argument (maps to ValueError in the binding)             */
    FSLIC_E_UNSUPPORTED = 2,   /* option outside the implemented surface (NotImplementedError) */
    FSLIC_E_HIP = 3,           /* HIP runtime failure: no device, OOM, launch error            */
    FSLIC_E_INTERNAL = 4
};

/* Bit-compatible with `Cluster`, src/fast-slic-common.h:10-23 (32 bytes; Cython mirror
 * cfast_slic.pxd:8-18).  r,g,b hold L,a,b when convert_to_lab is set.  `a` is never written. */
typedef struct fslic_cluster {
    float y, x, r, g, b, a;
    uint16_t number;
    uint8_t is_active;
    uint8_t is_updatable;
    uint32_t num_members;
} fslic_cluster;

/* The public configuration fields of BaseContext (src/context.h:26-36) as set by
 * SlicModel.iterate (cfast_slic.pyx:179-187), plus max_iter (context.iterate's argument). */
typedef struct fslic_params {
    int32_t max_iter;              /* BaseContext::iterate(assignment, max_iter), src/context.cpp:108 */
    float compactness;             /* src/context.h:28 */
    float min_size_factor;         /* src/context.h:29 */
    int32_t subsample_stride;      /* subsample_stride_config, src/context.h:26 (>= 1) */
    int32_t convert_to_lab;        /* src/context.h:30 */
    int32_t manhattan_spatial_dist;/* src/context.h:35; 0 (hypotf patch) takes the generic kernel */
    int32_t preemptive;            /* src/context.h:32, src/preemptive.h; every variant (BaseContext<DistType>::iterate, src/context.cpp:152-181) */
    float preemptive_thres;        /* src/context.h:33; ignored while preemptive == 0 */
    int32_t num_threads;           /* src/context.h:27; ignored on the GPU */
    int32_t debug_mode;            /* src/context.h:36; fslic_hip_iterate / fslic_hip_iterate_device record the reference's per-iteration
                                    * report (fslic_hip_last_recorder_report); the group and pipeline entries ignore it */
    int32_t abi;                   /* must be FSLIC_PARAMS_ABI: the layout of this struct has changed between library versions (a testing
                                    * flag lived in this slot in 0.2 and `variant` in the header of 0.2+); a caller built against
                                    * another layout is refused with FSLIC_E_INVALID instead of being misread */
    int32_t variant;               /* FSLIC_VARIANT_SLIC: Context (src/context.h:127); FSLIC_VARIANT_LSC: ContextLSC
                                    * (src/lsc.h:6-26), picked by cfast_slic.pyx:199-216 from real_dist_type */
    int32_t reserved[4];           /* must be 0 */
} fslic_params;
#define FSLIC_PARAMS_ABI 0x46533033  /* "FS03" */

enum {
    FSLIC_VARIANT_SLIC = 0,          /* Context, uint16 distances */
    FSLIC_VARIANT_LSC = 1,           /* ContextLSC, real_dist_type 'lsc' */
    FSLIC_VARIANT_REALDIST = 2,      /* ContextRealDist, real_dist_type 'standard' (src/context.h:100-103) */
    FSLIC_VARIANT_REALDIST_L2 = 3,   /* ContextRealDistL2, real_dist_type 'l2' (src/context.h:105-111) */
    FSLIC_VARIANT_REALDIST_NOQ = 4   /* ContextRealDistNoQ, real_dist_type 'noq' (src/context.h:113-125): float centroids */
};

typedef struct fslic_engine fslic_engine;

/* Number of visible HIP devices (0 when none / runtime unusable). */
int fslic_hip_device_count(void);

/* Create / destroy an engine bound to one GPU.  The engine owns every device and pinned-host
 * buffer and caches them across calls keyed by (H, W, K); the reference re-allocates per call
 * (BaseContext ctor, src/context.h:59-66, invoked from cfast_slic.pyx:171-177).
 * n_slots >= 1 is the number of frames that may be in flight at once (one HIP stream each). */
int fslic_hip_create(int device, int n_slots, fslic_engine** out);
void fslic_hip_destroy(fslic_engine* e);

/* Replaces BaseContext::initialize_clusters (src/context.cpp:42-97) as called by
 * SlicModel.initialize (cfast_slic.pyx:124-147).  Pure host code, O(K); `rgb` is a host pointer
 * to C-contiguous uint8[H][W][3]. */
int fslic_hip_initialize_clusters(int H, int W, int K, const uint8_t* rgb, fslic_cluster* clusters);
/* The part of it that needs no image (NEW surface): the seed grid, `number`, the flags and num_members = 0, with r, g, b set to 0.
 * fslic_hip_initialize_clusters is this call plus the colours of the K seed pixels; a caller whose frames live in device memory
 * reads those pixels there, at byte 3 * (W * (int)y + (int)x) + c of a frame (fast_slic_amd/frames.py). */
int fslic_hip_seed_positions(int H, int W, int K, fslic_cluster* clusters);

/* Replaces Context construction + initialize_state() + iterate() + delete for the integer SLIC path
 * (cfast_slic.pyx:171-197 -> src/context.cpp:108-197).
 *   rgb      : HOST pointer, borrowed, C-contiguous uint8[H][W][3]
 *   clusters : HOST pointer to K clusters, updated in place exactly like the reference does
 *   labels   : HOST pointer to uint16[H][W]; all H*W entries are written (0xFFFF possible);
 *              the caller applies astype(int16) / 0xFFFF -> -1 (cfast_slic.pyx:258-260). */
int fslic_hip_iterate(fslic_engine* e, const fslic_params* p, int H, int W, int K,
                      const uint8_t* rgb, fslic_cluster* clusters, uint16_t* labels);

/* Same computation with the frame already resident in HBM (NEW surface, absent in the reference;
 * SURVEY.md section 8f-4).  d_rgb / d_labels are DEVICE pointers on the engine's GPU; clusters stays a
 * host pointer (K*32 bytes).  `slot` selects the in-flight slot / stream (0 <= slot < n_slots).
 * The call returns after the slot's stream has been synchronised.
 * Alignment of the device buffers, here and in every entry point below that takes d_rgb / d_labels (the kernels read and write the
 * caller's memory in place, e.g. frame i of one stacked tensor):
 *   d_rgb    : any address.  A frame at a 4-byte-aligned address is read three dwords per four pixels; any other frame is read byte
 *              by byte (same results, slower).  Frames of one group may differ.
 *   d_labels : 2-byte aligned (it holds uint16_t); an odd address is refused with FSLIC_E_INVALID before any device work.  A map at an
 *              8-byte-aligned address with W % 4 == 0 is written with 8-byte stores; any other map two bytes at a time (same
 *              results, slower).  Maps of one group may differ.
 * Exactly H*W*3 bytes are read from d_rgb and exactly H*W*2 bytes are written to d_labels: nothing before or behind them is touched. */
int fslic_hip_iterate_device(fslic_engine* e, int slot, const fslic_params* p, int H, int W, int K,
                             const uint8_t* d_rgb, fslic_cluster* clusters, uint16_t* d_labels);

/* Independent frames of identical geometry (NEW surface; BASELINE.json config 4).  The frames are cut into
 * groups of up to 8 (FSLIC_GROUP, at most 16); every kernel launch of a group covers all of its frames (frame =
 * last grid dimension), groups rotate over the engine's slots (one stream each).
 * rgb[i] / labels[i] are host pointers when device_ptrs == 0 and device pointers otherwise;
 * clusters[i] are host pointers, each K clusters. */
int fslic_hip_iterate_batch(fslic_engine* e, const fslic_params* p, int H, int W, int K, int n_frames,
                            const uint8_t* const* rgb, fslic_cluster* const* clusters,
                            uint16_t* const* labels, int device_ptrs);

/* Asynchronous form for pipelining groups across calls (NEW surface): submit enqueues ONE group of n_frames
 * (1..16) device-resident frames on `slot` and returns without waiting; wait blocks until that group is complete,
 * serves its host-side steps and writes the clusters back.  The pointer arrays are copied; clusters[i] and the
 * device buffers must stay valid until the wait.  With two slots the host work of one group (cluster upload and
 * write-back) overlaps the kernels of the other. */
int fslic_hip_submit_group(fslic_engine* e, int slot, const fslic_params* p, int H, int W, int K, int n_frames,
                           const uint8_t* const* d_rgb, fslic_cluster* const* clusters, uint16_t* const* d_labels);
int fslic_hip_wait_group(fslic_engine* e, int slot);
/* Non-blocking: 1 when the group submitted on `slot` is complete (fslic_hip_wait_group will not block) or the slot is
 * idle, 0 while it is in flight, -1 on a bad argument.  Lets a caller with several slots collect groups in completion
 * order instead of submission order (groups with a top-K tie take longer than the others). */
int fslic_hip_group_done(fslic_engine* e, int slot);

/* The same, with the engine choosing the slot (NEW surface): submit puts one submission of n_frames (1..16)
 * device-resident frames into the engine's queue and returns; it blocks only while the queue is full (two submissions
 * per slot).  The slot threads serve the queue; the clusters of a submission are written back when its group is complete.
 * drain waits for everything submitted so far and returns the first error of any group since the previous drain (a
 * submit after a failed group returns that error as well); the optional outputs receive the totals over those groups:
 * device time (ms, HIP events per group), groups (launch groups: with batching on, fewer than submissions), frames, and
 * the number of frames whose top-K step fell back to the host.  A video pipeline calls submit once per batch of frames
 * and drain at the end.  (A slot that is serving the queue counts as owning an unfinished group: drain before addressing
 * slots by number with fslic_hip_submit_group.) */
int fslic_hip_pipeline_submit(fslic_engine* e, const fslic_params* p, int H, int W, int K, int n_frames,
                              const uint8_t* const* d_rgb, fslic_cluster* const* clusters, uint16_t* const* d_labels);
int fslic_hip_pipeline_drain(fslic_engine* e, double* device_ms, long long* groups, long long* frames,
                             long long* host_topk_frames);
/* Dynamic batching of the pipeline (off by default: max_frames_per_group = 0): a slot thread that finds several
 * submissions of identical geometry and options waiting serves them as ONE group of up to max_frames_per_group (<= 16)
 * frames -- every launch of the group then covers all of them.  Frames are independent, so results do not change; a
 * caller that submits faster than the device finishes gets fewer, fuller launches (1280x720: +10 %).  Arenas are carved
 * for max_frames_per_group frames from then on.  Call it before the first submit. */
int fslic_hip_pipeline_batching(fslic_engine* e, int max_frames_per_group);

/* Stage entry points (used by the parity tests; each mirrors one stage of iterate()). */

/* rgb_to_cielab, src/cielab.h:337-353 (convert != 0) or the raw copy of src/context.cpp:117-127
 * (convert == 0).  Host pointers; lab4 is uint8[H][W][4] = (L, a, b, 0). */
int fslic_hip_rgb_to_lab(fslic_engine* e, int H, int W, const uint8_t* rgb, int convert, uint8_t* lab4);

/* cca::ConnectivityEnforcer(labels,H,W,K,min_threshold).execute(labels), src/cca.cpp:178-265, as
 * exposed by cfast_slic.enforce_connectivity (cfast_slic.pyx:371-396).  In place, host pointer. */
int fslic_hip_enforce_connectivity(fslic_engine* e, uint16_t* labels, int H, int W, int K, int min_threshold);
/* The same pass; *n_nodes receives the number of union-find nodes the device pass kept for the frame (the components of
 * the 64x32 tiles minus the closed small ones): a testing aid, the tests restate the count on the CPU. */
int fslic_hip_enforce_connectivity_nodes(fslic_engine* e, uint16_t* labels, int H, int W, int K, int min_threshold, uint32_t* n_nodes);

/* ---- Superpixel-graph utilities on a finished label map (src/fast-slic.h:13-17, src/fast-slic.cpp; reached from
 * SlicModel.get_connectivity / get_knn_connectivity / get_mask_density / broadcast_density_to_mask,
 * cfast_slic.pyx:262-324).  `labels` (H*W uint16), `mask` (H*W uint8) and `result` (H*W uint8) may be host pointers or
 * device pointers (a label map left in HBM by fslic_hip_iterate_device needs no copy); the per-cluster arrays are host
 * arrays.  Device planes are read and written in place, one element at a time: `labels` 2-byte aligned, `mask` and `result` at any
 * address, and no byte outside the H*W elements is touched.The reference returns a heap-allocated Connectivity (src/fast-slic-common.h:25-29); here the same content is
 * written into caller arrays: num_neighbors[K] and neighbors[K][stride] (unused entries 0). */

/* fast_slic_get_connectivity(H, W, K, assignment), src/fast-slic.cpp:16-78: for every cluster its adjacent clusters
 * (right / down / down-right scan) in the order the raster scan meets them, at most 12 per cluster with the
 * reference's order-dependent cut-off.  stride = 12. */
int fslic_hip_get_connectivity(fslic_engine* e, int H, int W, int K, const uint16_t* labels,
                               int* num_neighbors, uint32_t* neighbors);

/* fast_slic_knn_connectivity(H, W, K, clusters, num_neighbors), src/fast-slic.cpp:80-130.  Host only (O(K)); the
 * neighbour order is the reference's heap order.  stride = n_neighbors. */
int fslic_hip_knn_connectivity(int H, int W, int K, const fslic_cluster* clusters, size_t n_neighbors,
                               int* num_neighbors, uint32_t* neighbors);

/* fast_slic_get_mask_density(H, W, K, clusters, assignment, mask, cluster_densities), src/fast-slic.cpp:141-154:
 * densities[k] = min(255, sum of mask over the pixels labelled k / max(num_members[k], 1)). */
int fslic_hip_get_mask_density(fslic_engine* e, int H, int W, int K, const fslic_cluster* clusters,
                               const uint16_t* labels, const uint8_t* mask, uint8_t* densities);

/* fast_slic_cluster_density_to_mask(H, W, K, clusters, assignment, cluster_densities, result), src/fast-slic.cpp:156-168
 * (the reference's `clusters` argument is unused and not taken): result[p] = densities[labels[p]], 0 for labels >= K. */
int fslic_hip_cluster_density_to_mask(fslic_engine* e, int H, int W, int K, const uint16_t* labels,
                                      const uint8_t* densities, uint8_t* result);

/* Labels after full_assign and before the connectivity pass (BaseContext::assignment,
 * src/context.cpp:182-190) of the last fslic_hip_iterate*() call on `slot`; host pointer, H*W. */
int fslic_hip_last_prelabels(fslic_engine* e, int slot, uint16_t* prelabels);

/* Debug entry, for tests only (read-only): the LSC state of frame `z` of the last group on `slot`, read back once the slot is idle --
 * the ten feature means (src/lsc.cpp:143-149) into means10[10] and the K feature-space centroids as they stand behind the last update
 * (the seed centroids with max_iter = 0) into cfeat[K * 10], ten floats per cluster, NaN for a cluster without a member.  Host
 * pointers.  FSLIC_E_INVALID when the slot's last group was not of FSLIC_VARIANT_LSC, `z` is not one of its frames or K is not its K. */
int fslic_hip_debug_lsc_state(fslic_engine* e, int slot, int z, int K, float* means10, float* cfeat);

/* Replaces BaseContext::get_timing_report (src/context.h:74): JSON with the fstimer schema
 * {"name","duration"(us),"children"} (src/timer.cpp:4-18), durations from HIP events of the CALLING THREAD's last
 * fslic_hip_iterate* / fslic_hip_wait_group (thread-local like the reference's timer, src/timer.cpp:45).  Pointer
 * valid until that thread's next call. */
const char* fslic_hip_last_timing_report(fslic_engine* e);

/* Replaces BaseContext::get_recorder_report (src/context.h; the JSON of src/recorder.h, as cfast_slic.pyx:196 / :256 store it in
 * SlicModel.last_recorder_report): the report of the CALLING THREAD's last successful fslic_hip_iterate / fslic_hip_iterate_device.
 * With fslic_params.debug_mode set it holds snapshot -1 and one snapshot per iteration (labels before connectivity, min_dists, the
 * Cluster[K] block of that moment), byte for byte what the reference prints; otherwise the header alone,
 * {"height": H, "width": W, "snapshots": []}.  Such a call runs the recording path (one frame, direct launches, the generic / unfused
 * kernels; same results, slower).  fslic_hip_iterate_batch, fslic_hip_submit_group and fslic_hip_pipeline_submit ignore debug_mode
 * and leave the report alone.  *report is NUL-terminated, *length its size; it stays valid until the thread's next iterate call. */
int fslic_hip_last_recorder_report(fslic_engine* e, const char** report, size_t* length);

/* Device time (ms, HIP events on the slot's stream) of the last frame GROUP on `slot`: whole pipeline, and
 * the full-assign launch alone (the roofline kernel; it covers every frame of the group).  */
int fslic_hip_last_device_times(fslic_engine* e, int slot, float* total_ms, float* full_assign_ms);

/* Per-launch timing of the subsampled (fused assign + update) launches: when on, groups submitted afterwards bracket
 * each of those launches with HIP events on the slot's stream (about 1 us of stream time per launch, hence opt-in).
 * last_assign_loop: sum of their durations (ms), pixels they visited over all frames, number of launches timed
 * (0 when the group was submitted with timing off). */
int fslic_hip_set_launch_timing(fslic_engine* e, int on);
int fslic_hip_last_assign_loop(fslic_engine* e, int slot, float* sum_ms, double* visited_px, int* launches);

/* Number of frames in the last group on `slot` (1 for iterate / iterate_device). */
int fslic_hip_last_group_frames(fslic_engine* e, int slot);

/* How the last group on `slot` reached the GPU: 0 = operations enqueued one by one, 1 = recorded as a hipGraph during
 * this call and launched, 2 = replay of a recorded graph.  (The engine records a launch sequence the second time it
 * sees the same geometry / options / group size; the environment variable FSLIC_GRAPH=0, read when the library is
 * loaded, disables that.)  Testing / diagnostics aid. */
int fslic_hip_last_launch_mode(fslic_engine* e, int slot);

/* Which kernel family served the last call on `slot`: 0 = tiled (LDS candidate lists), 1 = generic. */
int fslic_hip_last_path(fslic_engine* e, int slot);

/* Frames of the last group on `slot` whose top-K step of the connectivity pass ran on the host (more candidate
 * components than the device sorts in one block; an area tie at the cut is resolved on the device). */
int fslic_hip_last_host_topk_frames(fslic_engine* e, int slot);

/* Frames redone on `slot` since it was created because a visited pixel that no cluster window covered kept its label
 * (src/context.cpp:138-145 resets the assignment plane once per call, not per iteration) while the cluster pass
 * (src/context.cpp:356-373) ran fused into the assign kernel: such a frame is recomputed with the separate cluster pass,
 * the results are those of the reference either way.  Cost: such a frame is computed TWICE (about 2 x the latency of that call);
 * it only arises in groups small enough to take the fused cluster pass (one or two 1280x720 frames per call), with warm starts whose
 * centres have drifted far enough apart to leave visited pixels uncovered.  A caller that sees this counter grow on a stream can set
 * FSLIC_FUSEBIN=0 (the separate cluster pass everywhere: +8 % latency per one-frame call, no redo).  Diagnostics aid. */
int fslic_hip_separate_pass_redos(fslic_engine* e, int slot);

/* Frames redone on `slot` since it was created because a visited pixel lay outside every cluster window while the group's subsampled
 * assign passes ran in their label-free form (they store no labels: the full pass at the end overwrites every covered pixel, and only an
 * uncovered pixel ever needs the label of an earlier pass).  Such a frame is recomputed with storing passes, the results are those of
 * the reference either way, and the slot keeps to the storing passes for that work (H, W, K, params) from then on, so a stream of such
 * inputs pays the redo once.  Grid-seeded and warm-started centres never leave a pixel uncovered; arbitrary caller-supplied centres
 * can.  Diagnostics aid. */
int fslic_hip_uncovered_redos(fslic_engine* e, int slot);

/* Groups of the submit / drain pipeline, since the engine was created, that a slot's thread began while the slot's previous group had not
 * been collected yet: the slot's stream received the next group's kernels behind those of the running one, and the running group was
 * waited for, written back and collected afterwards.  A slot thread does this when the submission at the head of the queue asks for the
 * same work (H, W, K, params) as the group it has running, the slot's buffers serve it as they are, no other slot is free to take it, and
 * neither per-launch timing, preemptive mode nor the 'noq' variant is involved; never for fslic_hip_submit_group or the synchronous
 * entry points.  Results do not depend on it.  -1: no engine.  Diagnostics aid. */
long long fslic_hip_overlapped_groups(fslic_engine* e);

/* on == 0: the slot threads of this engine finish every group before they begin the next one (the serial loop: depth one, as for
 * fslic_hip_submit_group), and fslic_hip_overlapped_groups stops counting; on != 0 (the default): as described above.  Takes effect
 * with the next submission a slot thread takes from the queue.  For A/B measurements and tests. */
int fslic_hip_pipeline_overlap(fslic_engine* e, int on);

/* Debug entries, for tests only: the record of kernel FORMS.  The assign pass is a family of template instantiations picked by the
 * spatial table, the stride, the launch size and the mode, and the preemptive update has two forms; every launch site notes a code for the
 * instantiation it chose when it enqueues the launch or records it into a graph (a replay adds nothing).  The record is the process-wide
 * set of distinct codes, thread-safe, host side only.  A code is
 *   bits 0-3 family (1 blk, 2 bin, 3 pre, 4 k32, 5 generic, 6 generic_rec, 7 preempt_update) | bits 4-9 rows per wavefront |
 *   bit 10 fused | bits 11-13 stride template (0: run-time argument) | bits 14-16 table (0 none, 1 row-vector, 2 the full pass's 16-row
 *   row-vector table, 3 2-D, 4 2-D for 16 rows, 5 LUT) | bit 17 label-free | bit 18 all-pairs (preempt_update; 0: per-cell lists).
 * forms_seen: up to `cap` recorded codes into `codes` (may be NULL with cap 0); returns how many are recorded, -2 when the record
 * overflowed; `clear` != 0 empties the record afterwards.  forms_all: the complete list of codes the dispatch can produce (a static table
 * next to the launch functions), up to `cap` into `codes`; returns its length.  -1: cap < 0, or codes NULL with cap > 0. */
int fslic_hip_debug_forms_seen(uint32_t* codes, int cap, int clear);
int fslic_hip_debug_forms_all(uint32_t* codes, int cap);

/* Measurement aid (no counterpart in the reference): bytes read + written per second, in GB/s, of a plain streaming copy of
 * `bytes` on the engine's GPU (best of `reps` launches, HIP events) -- the measured HBM rate that bench.py prints next to the 8 TB/s of
 * the specification.  Allocates and frees 2 x `bytes` of device memory. */
int fslic_hip_copy_bandwidth(fslic_engine* e, size_t bytes, int reps, double* gb_per_s);

/* ---- SimpleCRF (src/simple-crf.h, src/simple-crf.{hpp,cpp}; Python: csimple_crf.pyx, fast_slic/crf.py) ----
 * Mean-field inference of a Potts CRF over the superpixel graph: spatial edges inside a frame (the neighbour lists, typically from
 * fslic_hip_get_connectivity) and temporal edges between consecutive frames (node i of frame t to node i of t-1 and t+1).  The
 * state lives on the host (every entry but fslic_hip_crf_inference and fslic_hip_crf_expf_device works without a GPU); inference
 * runs on the engine's GPU and leaves q there until it is read.  Results are bit-identical to the reference's.
 * Handles: a frame handle stays valid until its frame is popped or its CRF freed.  Every entry point may be called from any thread;
 * calls on one CRF (and its frames) are serialised by the CRF, fslic_hip_crf_inference takes one engine slot.
 * Deliberate differences, each refused with FSLIC_E_INVALID where the reference has undefined behaviour:
 *   - num_classes or num_nodes 0, num_classes * num_nodes >= 2^31 (new); frames * classes * nodes or the total number of
 *     neighbour entries of the window >= 2^31 (inference);
 *   - neighbour indices >= num_nodes (set_connectivity: the reference indexes q with them unchecked), more rows than nodes;
 *   - a class outside [0, num_classes) (set_mask, get/set_compat), a node outside [0, num_nodes) (the energies);
 *   - inference with max_iter > 0 and no frame (the reference dereferences a missing frame);
 *   - a missing time (fslic_hip_crf_frame; the reference throws std::out_of_range through its C API).
 * copy is a deep copy (the reference's copy constructor shares its frames' time map and parent with the original). */
typedef struct fslic_crf fslic_crf;
typedef struct fslic_crf_frame fslic_crf_frame;
typedef struct fslic_crf_params {  /* SimpleCRFParams, src/simple-crf.h:11-19; defaults src/simple-crf.hpp:81-87 */
    float spatial_w, temporal_w, spatial_srgb, temporal_srgb, spatial_sxy, spatial_smooth_w, spatial_smooth_sxy;
} fslic_crf_params;

int fslic_hip_crf_new(size_t num_classes, size_t num_nodes, fslic_crf** out);          /* simple_crf_new,  simple-crf.h:29 */
void fslic_hip_crf_free(fslic_crf* crf);                                               /* simple_crf_free, simple-crf.h:31 */
int fslic_hip_crf_copy(fslic_crf* crf, fslic_crf** out);                               /* simple_crf_copy, simple-crf.h:97 */
int fslic_hip_crf_get_params(fslic_crf* crf, fslic_crf_params* out);                   /* simple-crf.h:33 */
int fslic_hip_crf_set_params(fslic_crf* crf, const fslic_crf_params* params);          /* simple-crf.h:34 */
int fslic_hip_crf_set_compat(fslic_crf* crf, int cls, float compat_value);             /* simple-crf.h:35 */
int fslic_hip_crf_get_compat(fslic_crf* crf, int cls, float* out);                     /* simple-crf.h:36 */
int fslic_hip_crf_num_classes(fslic_crf* crf, size_t* num_classes, size_t* num_nodes);  /* the sizes given to new */
/* Times: -1 when there is no frame (simple-crf.h:38-39); pop returns the popped time or -1 (:41). */
int fslic_hip_crf_first_time(fslic_crf* crf);
int fslic_hip_crf_last_time(fslic_crf* crf);
size_t fslic_hip_crf_num_frames(fslic_crf* crf);                                       /* simple-crf.h:40 */
int fslic_hip_crf_pop_frame(fslic_crf* crf);
int fslic_hip_crf_push_frame(fslic_crf* crf, fslic_crf_frame** out);                   /* simple-crf.h:42 */
int fslic_hip_crf_frame(fslic_crf* crf, int time, fslic_crf_frame** out);              /* simple-crf.h:43 */
int fslic_hip_crf_frame_time(fslic_crf_frame* frame);                                  /* simple-crf.h:44 */
/* clusters: num_nodes fslic_cluster (simple-crf.h:51); get returns them as set (no counterpart in the C API: the pyx reads them). */
int fslic_hip_crf_frame_set_clusters(fslic_crf_frame* frame, const fslic_cluster* clusters);
int fslic_hip_crf_frame_get_clusters(fslic_crf_frame* frame, fslic_cluster* clusters);
/* Neighbour lists (simple-crf.h:52, Connectivity of src/fast-slic-common.h:25-29): rows [0, num_rows) are replaced, others kept.
 * Table form: row i is neighbors[i * stride + k], k < num_neighbors[i] (what fslic_hip_get_connectivity writes, stride 12);
 * CSR form: row i is indices[offsets[i] .. offsets[i+1]).  Lists may be empty, longer than 12, hold duplicates and self-loops. */
int fslic_hip_crf_frame_set_connectivity(fslic_crf_frame* frame, int num_rows, const int* num_neighbors, const uint32_t* neighbors,
                                         size_t stride);
int fslic_hip_crf_frame_set_connectivity_csr(fslic_crf_frame* frame, int num_rows, const int64_t* offsets, const uint32_t* indices);
/* The lists as CSR: offsets[num_nodes + 1]; indices may be NULL to ask for the size only (offsets[num_nodes]). */
int fslic_hip_crf_frame_get_connectivity(fslic_crf_frame* frame, int64_t* offsets, uint32_t* indices);
/* Unaries, [num_classes][num_nodes] float (simple-crf.h:59-66). */
int fslic_hip_crf_frame_set_mask(fslic_crf_frame* frame, const int32_t* classes, float confidence);
int fslic_hip_crf_frame_set_proba(fslic_crf_frame* frame, const float* probas);
int fslic_hip_crf_frame_set_unbiased(fslic_crf_frame* frame);
int fslic_hip_crf_frame_set_unary(fslic_crf_frame* frame, const float* unary_energies);
int fslic_hip_crf_frame_get_unary(fslic_crf_frame* frame, float* unary_energies);
/* simple-crf.h:77-78.  The temporal energy is taken towards `other_frame` (any frame, of any CRF; 0 for the frame itself) as
 * SimpleCRFFrame::calc_temporal_pairwise_energy does -- the reference's C wrapper passes the frame itself instead (always 0). */
int fslic_hip_crf_frame_spatial_energy(fslic_crf_frame* frame, int node_i, int node_j, float* out);
int fslic_hip_crf_frame_temporal_energy(fslic_crf_frame* frame, fslic_crf_frame* other_frame, int node_i, float* out);
/* q, [num_classes][num_nodes] float (simple-crf.h:84-85); initialize resets every frame (simple-crf.h:30). */
int fslic_hip_crf_frame_get_inferred(fslic_crf_frame* frame, float* probas);
int fslic_hip_crf_frame_reset_inferred(fslic_crf_frame* frame);
int fslic_hip_crf_initialize(fslic_crf* crf);
/* simple_crf_inference (simple-crf.h:92): max_iter Jacobi sweeps over every frame, on the engine's GPU (one slot).  max_iter == 0
 * does nothing and needs no engine.  A CRF keeps its device buffers on the engine of its last inference. */
int fslic_hip_crf_inference(fslic_crf* crf, fslic_engine* e, size_t max_iter);
/* Testing aids: the exponential the CRF uses (a copy of the host libm's expf, crf.h) over a batch of host floats, on the host
 * (use_libm != 0: the host libm's expf itself, for comparison) or on the engine's GPU. */
int fslic_hip_crf_expf_host(const float* in, float* out, size_t n, int use_libm);
int fslic_hip_crf_expf_device(fslic_engine* e, const float* in, float* out, size_t n);

/* ---- Superpixel pooling (NEW surface, no counterpart in the reference; Python: fast_slic_amd/pool.py) ----
 * Pooling of float feature planes over a label map, and the inverse broadcast, on device memory the caller owns.  No engine: each
 * entry takes a device index and a stream (a hipStream_t; NULL is the default stream), enqueues its work on that stream and returns
 * without synchronising and without allocating.  The calling thread's current device is restored.  Every argument is checked before
 * the first HIP call (FSLIC_E_INVALID).
 *   features : float [N][C][H][W], contiguous          labels : [N][H][W] of label_type; values outside [0, K) belong to no segment
 *   values   : float [N][C][K]                          counts : int32 [N][K]              argmax : int32 [N][C][K]
 * Results are bitwise reproducible: per-tile float partials in a fixed order (a tile is 16 rows x 64 columns, aligned at the frame's
 * origin), combined in a fixed-point accumulator with integer atomics and rounded once (sum within 4e-6 of the sum of |x|).  Every
 * partial enters the accumulator truncated towards zero to a multiple of 2^-96, so partials (and inputs) below 2^-96 in magnitude,
 * subnormal ones included, vanish; the truncated partials are added exactly and the total is rounded once to f32, nearest with ties
 * to even.  Hence the sum is the correctly rounded sum of the partials when every partial is a multiple of 2^-96 (any f32 of
 * magnitude 2^-73 or more is), and the correctly rounded sum of the pixels when in addition every partial is exact in f32.  A
 * total of zero is +0.0; a total of magnitude 2^128 - 2^103 or more (FLT_MAX plus half an ulp) is +-inf, while partials that
 * pass 2^128 on the way and cancel again do no harm.  An in-tile f32 partial that overflows leaves its segment's entry unspecified,
 * like an Inf input.
 * The workspace holds N * C * K * 56 bytes (sum, mean) or N * C * K * 8 bytes (max), plus N * K * 4 bytes of counts (rounded up to 8). */
enum { FSLIC_POOL_SUM = 0, FSLIC_POOL_MEAN = 1, FSLIC_POOL_MAX = 2 };
enum { FSLIC_LABEL_U16 = 0 /* the int16 map of iterate(), -1 = 0xFFFF */, FSLIC_LABEL_I32 = 1, FSLIC_LABEL_I64 = 2 };
int fslic_hip_pool_workspace_size(int N, int C, int K, int reduce, size_t* bytes);
/* Clears the workspace and accumulates into it (K in 1 .. 65534). */
int fslic_hip_pool(int device, void* stream, int N, int C, int H, int W, int K, int reduce, const float* features,
                   const void* labels, int label_type, void* workspace, size_t workspace_bytes);
/* The workspace of a completed fslic_hip_pool (same stream, same N, C, K, reduce) -> values: the sum; the sum / count (0 for an empty
 * segment); the maximum (-0.0 below +0.0; 0 for an empty segment).  counts (optional) the pixels per segment; argmax (optional, max
 * only) the lowest flat index h * W + w holding the maximum, -1 for an empty segment.  NaN / Inf in a segment leave that segment's
 * entries unspecified. */
int fslic_hip_pool_finalize(int device, void* stream, int N, int C, int K, int reduce, const void* workspace, size_t workspace_bytes,
                            float* values, int32_t* counts, int32_t* argmax);
/* out[n][c][p] = values[n][c][labels[n][p]], `fill` where the label is not in [0, K).  With argmax (the max backward):
 * out[n][c][p] = values[n][c][l] where argmax[n][c][l] == p, `fill` everywhere else. */
int fslic_hip_unpool(int device, void* stream, int N, int C, int H, int W, int K, const float* values, const void* labels,
                     int label_type, const int32_t* argmax, float fill, float* out);

/* ---- Frames of any tensor layout into the engine's form (NEW surface, no counterpart in the reference; Python: fast_slic_amd/frames.py) ----
 * N frames of 3 channels -> uint8 [H][W][3] interleaved, what fslic_hip_iterate_batch and the other device entries read.  Entry as for
 * pooling: a device index and a stream, no synchronisation, no allocation, the caller's device restored, every argument checked before
 * the first HIP call (FSLIC_E_INVALID).
 *   src     : element (n, c, y, x) at src + n * strides[0] + c * strides[1] + y * strides[2] + x * strides[3], strides in ELEMENTS of
 *             src_type (FSLIC_PACK_*), any value, 0 included; src is aligned to its element type; H * W < 2^31
 *   out     : frame n at out + n * pitch; pitch >= 3 H W, a multiple of 16 and at most 2^33; out is 4-byte aligned.  The bytes
 *             [3 H W, pitch) of every frame are written as 0; nothing outside [out, out + N * pitch) is touched.
 * A float source, per element, in float32 (float16 and bfloat16 widen exactly): v = x * scale, one rounding; NaN -> 0; clamp to
 * [0, 255]; round to nearest, ties to even.  scale is finite.  A uint8 source is copied and scale ignored.  One launch (in slices
 * past 2^24 - 1 blocks of 1024 pixels: N * ceil(ceil(pitch / 12) / 256) is admitted up to 2^31 - 1). */
enum { FSLIC_PACK_U8 = 0, FSLIC_PACK_F16 = 1, FSLIC_PACK_BF16 = 2, FSLIC_PACK_F32 = 3 };
int fslic_hip_pack_rgb(int device, void* stream, int N, int H, int W, const void* src, int src_type, const long long strides[4],
                       float scale, uint8_t* out, size_t pitch);

/* ---- Region adjacency graph of a label map (NEW surface, no counterpart in the reference; Python: fast_slic_amd/rag.py) ----
 * Every unordered pair of labels that touch, with the number of neighbouring pixel pairs across their boundary and, with an image, per
 * channel the sum of |difference| over those pixel pairs.  connectivity 4 looks at every pixel's right and down neighbour, 8 also
 * down-right and down-left: every pixel pair of the whole plane once.  A pixel whose label is outside [0, K) is in no pair.  Entries
 * as for pooling: a device index and a stream, no synchronisation, no allocation, the caller's device restored, every argument checked
 * before the first HIP call (FSLIC_E_INVALID).
 *   labels : [N][H][W] of label_type (FSLIC_LABEL_*), H * W < 2^29        image : uint8 [N][H][W][C], C in 1 .. 4, or NULL with C == 0
 * Pairs are collected per frame in an open-addressing table of `capacity` slots (a power of two in [64, 2^31]); the workspace holds a
 * header of 16 + 4 N bytes (rounded up to 16) and N * capacity * (8 + 8 C) bytes of tables.  Header: uint32 overflow flag, uint32
 * unused, uint64 used by compact, then uint32 [N]: the distinct pairs of each frame.  The flag is set when a frame's table got more
 * than half full or a probe run exceeded its bound; the tables are then incomplete and the caller starts over with a larger capacity
 * (2 * min(K (K - 1) / 2, 4 H W) pairs rounded up to a power of two always suffice for the load).  All integer arithmetic: the
 * result does not depend on the capacity or on the order of execution. */
int fslic_hip_rag_workspace_size(int N, int K, int C, long long capacity, size_t* bytes);
/* Clears the workspace, then fills the tables and the header. */
int fslic_hip_rag_accumulate(int device, void* stream, int N, int H, int W, int K, int connectivity, const void* labels, int label_type,
                             const uint8_t* image, int C, long long capacity, void* workspace, size_t workspace_bytes);
/* The occupied slots of the workspace of a completed fslic_hip_rag_accumulate (same stream, same N, C, capacity), densely and in NO
 * specified order: keys[i] = frame << 32 | lo << 16 | hi (lo < hi), boundary[i] its pixel pairs, contrast[i][C] (optional) its channel
 * sums.  At most max_edges rows are written (the sum of the header's counts is what there is). */
int fslic_hip_rag_compact(int device, void* stream, int N, int C, long long capacity, void* workspace, size_t workspace_bytes,
                          int64_t* keys, int32_t* boundary, int64_t* contrast, long long max_edges);

/* ---- Two label maps against each other (NEW surface, no counterpart in the reference; Python: fast_slic_amd/compare.py) ----
 * The overlap table: every pair (a, b) = (labels[p], other[p]) that shares a pixel, with the number of its pixels.  A pixel takes part
 * when 0 <= labels[p] < K and 0 <= other[p] < M, decided on the value at its own width; K and M in [1, 65534].  Entries as for the
 * graph: a device index and a stream, no synchronisation, no allocation, the caller's device restored, every argument checked before
 * the first HIP call (FSLIC_E_INVALID).
 *   labels, other : [N][H][W] of label_type / other_type (FSLIC_LABEL_*, they may differ), H * W < 2^31
 * Pairs are collected per frame in an open-addressing table of `capacity` slots (a power of two in [64, 2^31]); the workspace holds a
 * header of 16 + 4 N bytes (rounded up to 16) and N * capacity * 8 bytes of tables: uint32 keys [N][capacity], (a << 16 | b) + 1 and 0
 * for an empty slot, then uint32 pixels [N][capacity].  Header: uint32 overflow flag, uint32 unused, uint64 used by compact, then
 * uint32 [N]: the distinct pairs of each frame.  The flag is set when a frame's table got more than half full or a probe run exceeded
 * its bound; the tables are then incomplete and the caller starts over with a larger capacity (2 * min(K M, H W) pairs rounded up to
 * a power of two always suffice for the load).  All integer arithmetic: the result does not depend on the capacity or on the order
 * of execution. */
int fslic_hip_overlap_workspace_size(int N, long long capacity, size_t* bytes);
/* Clears the workspace, then fills the tables and the header. */
int fslic_hip_overlap_accumulate(int device, void* stream, int N, int H, int W, int K, int M, const void* labels, int label_type,
                                 const void* other, int other_type, long long capacity, void* workspace, size_t workspace_bytes);
/* The occupied slots of the workspace of a completed fslic_hip_overlap_accumulate (same stream, same N, capacity), densely and in NO
 * specified order: keys[i] = frame << 32 | a << 16 | b, count[i] its pixels.  At most max_pairs rows are written (the sum of the
 * header's counts is what there is). */
int fslic_hip_overlap_compact(int device, void* stream, int N, long long capacity, void* workspace, size_t workspace_bytes,
                              int64_t* keys, int32_t* count, long long max_pairs);
/* The boundary match.  A boundary pixel of a map is one whose value differs from its right or its lower neighbour's, where the image
 * has that neighbour (values compared as stored: no K).  counts[n] = { boundary pixels of other[n] that have a boundary pixel of
 * labels[n] within Chebyshev distance `tolerance` (0 .. 15), boundary pixels of other[n], boundary pixels of labels[n] }.  Clears
 * counts (int64 [N][3], device memory), then adds into it with integer atomics: exact whatever the order.  No workspace. */
int fslic_hip_boundary_match(int device, void* stream, int N, int H, int W, const void* labels, int label_type,
                             const void* other, int other_type, int tolerance, int64_t* counts);

/* ---- Connectivity on label tensors (NEW surface; Python: fast_slic_amd/connect.py, which states the rules) ----
 * The 4-connected components of equal labels of every frame, and the merge of the components below a minimum area: the reference's
 * ConnectivityEnforcer::execute (src/cca.cpp:178-265) without its cut at K labels, on device memory.  Entries as for pooling: a device
 * index and a stream, no synchronisation, no allocation, no copy to the host, no host path for any input, the caller's device
 * restored, every argument checked before the first HIP call (FSLIC_E_INVALID).
 *   labels : [N][H][W] of label_type (FSLIC_LABEL_*), N * H * W < 2^31; values are compared for equality only, at their own width
 *   out    : int32 [N][H][W], overlaps neither the labels nor the workspace        counts : int32 [N]
 * A component's leader is its first pixel in raster order; components are numbered 0, 1, ... in ascending leader order.
 * The workspace holds 8 bytes per pixel (two uint32 planes, each rounded up to 16 bytes: the leader of every pixel; the area, then the
 * label, of every leader) and 4 bytes per 1024 pixels of a frame (rounded up likewise).  It needs no clearing.  All integer
 * arithmetic; a component's root is always its smallest raster index, so the result does not depend on the order of execution. */
int fslic_hip_connect_workspace_size(int N, int H, int W, size_t* bytes);
/* components[n][p] = the number of p's component, counts[n] = the components of frame n. */
int fslic_hip_connected_components(int device, void* stream, int N, int H, int W, const void* labels, int label_type,
                                   int32_t* components, int32_t* counts, void* workspace, size_t workspace_bytes);
/* The components of at least min_size (>= 0) pixels are kept and take the labels 0, 1, ... in ascending leader order.  Component 0,
 * when it is not kept, takes label 0; every other component that is not kept takes the final label of the component of the pixel
 * left of its leader (above it for a leader in column 0).  counts[n] = the kept components of frame n, 1 when there are none: the
 * labels 0 .. counts[n] - 1 all occur, and counts[n] <= H * W / min_size for min_size >= 1. */
int fslic_hip_connect_enforce(int device, void* stream, int N, int H, int W, const void* labels, int label_type, long long min_size,
                              int32_t* out, int32_t* counts, void* workspace, size_t workspace_bytes);

/* ---- Merging on the region adjacency graph (NEW surface; Python: fast_slic_amd/merge.py, which states the rules) ----
 * A graph is what fslic_hip_rag_compact delivers once sorted: N frames of K nodes (K in [1, 65534], N * K < 2^31) and E < 2^31 edges,
 *   edge_index : int64 [2][E], row 0 the node a and row 1 the node b of every edge        offsets : int64 [N + 1]
 * the edges of frame f at [offsets[f], offsets[f + 1]); the position of an edge is its index minus offsets[f].  Entries as for
 * pooling: a device index and a stream, no synchronisation, no allocation, no copy to the host, the caller's device restored, every
 * argument checked before the first HIP call (FSLIC_E_INVALID).  What the device arrays hold is checked by the kernels before it
 * becomes an index: an edge with a node outside [0, K) takes part in nothing, and the frame of an edge is found by a search in
 * offsets[1 .. N] whose result is a frame whatever they hold.  All integer arithmetic and comparison: exact, the same from run to run.
 *
 * Best edges.  weight : float [E], >= 0 (-0.0 counts as +0.0; NaN or negative values leave the result unspecified).  An edge is
 * eligible if has_threshold == 0 or weight < threshold; a node's best edge is the eligible edge at it with the smallest
 * (weight, position); join[e] (uint8, 0 or 1) says whether e is the best edge of at least one of its nodes.  The workspace holds
 * 8 N K bytes (one 64-bit key per node) and needs no clearing.  E == 0: nothing is launched. */
int fslic_hip_merge_best_workspace_size(int N, int K, size_t* bytes);
int fslic_hip_merge_best_edges(int device, void* stream, int N, int K, long long E, const int64_t* edge_index, const int64_t* offsets,
                               const float* weight, int has_threshold, double threshold, uint8_t* join, void* workspace,
                               size_t workspace_bytes);
/* Components.  A node is present if members is NULL or members[n][v] > 0 (members_type FSLIC_LABEL_I32 or FSLIC_LABEL_I64).  Groups
 * are the connected components of a frame's present nodes under the edges with join[e] != 0 whose two nodes are present; a group's
 * leader is its smallest node; groups are numbered 0, 1, ... in ascending leader order.  mapping[n][v] (int32 [N][K]) = the number of
 * v's group, -1 for an absent node; counts[n] (int32 [N]) = the groups of frame n.  The workspace holds two uint32 planes of N K words
 * and 4 bytes per 256 nodes of a frame (each part rounded up to 16 bytes) and needs no clearing.  Six launches whatever the graph. */
int fslic_hip_merge_components_workspace_size(int N, int K, size_t* bytes);
int fslic_hip_merge_components(int device, void* stream, int N, int K, long long E, const int64_t* edge_index, const int64_t* offsets,
                               const uint8_t* join, const void* members, int members_type, int32_t* mapping, int32_t* counts,
                               void* workspace, size_t workspace_bytes);
/* Labels.  out[n][p] (int32 [N][H][W], 4-byte aligned, overlapping nothing) = mapping[n][labels[n][p]] for a label in [0, K), -1 for
 * any other.  labels : [N][H][W] of label_type (FSLIC_LABEL_*), N * H * W < 2^31, at any alignment of its type. */
int fslic_hip_merge_labels(int device, void* stream, int N, int H, int W, int K, const void* labels, int label_type,
                           const int32_t* mapping, int32_t* out);
/* Contraction.  Clears the workspace of a label pair table (the graph's: fslic_hip_rag_workspace_size(N, K2, C, capacity)), then for
 * every edge (a, b) of frame n with a' = mapping[n][a] and b' = mapping[n][b] both in [0, K2) and different adds boundary[e] (int32)
 * and the row contrast[e][C] (int64; NULL with C == 0) to the pair (min(a', b'), max(a', b')).  The header is the graph's, and so is
 * the way out: fslic_hip_rag_compact on the same stream, and a larger capacity after an overflow (2 * min(K2 (K2 - 1) / 2, E) pairs
 * rounded up to a power of two always suffice for the load). */
int fslic_hip_merge_contract_accumulate(int device, void* stream, int N, int K, int K2, long long E, const int64_t* edge_index,
                                        const int64_t* offsets, const int32_t* boundary, const int64_t* contrast, int C,
                                        const int32_t* mapping, long long capacity, void* workspace, size_t workspace_bytes);

/* ---- The features of merged regions (NEW surface; Python: fast_slic_amd/regions.py, which states the rules) ----
 * Entries as for merging: a device index and a stream, no synchronisation, no allocation, no copy to the host, the caller's device
 * restored, every argument checked before the first HIP call (FSLIC_E_INVALID); what the device arrays hold is checked by the kernels
 * before it becomes an index.  N frames, C >= 1 channels, K and K2 in [1, 65534], N * C * K and N * C * K2 below 2^31.
 *
 * Group sums.  sums[n][c][g] (float [N][C][K2]) = the sum of values[n][c][v] (float [N][C][K]) over the nodes v with
 * mapping[n][v] == g (int32 [N][K]); a mapping word outside [0, K2) adds nothing.  Each value is truncated towards zero to a multiple
 * of 2^-96, the values are added exactly (the fixed-point accumulator of fslic_hip_pool, integer atomics), and the total is rounded
 * once to float, ties to even: the same bits whatever the order.  No value, or a zero total: +0.0.  A NaN or Inf value leaves its
 * group's entry unspecified.  counts (NULL, or [N][K] of counts_type FSLIC_LABEL_I32 or FSLIC_LABEL_I64) is added likewise into
 * counts_out ([N][K2] of the same type; NULL exactly when counts is), with wrapping integer atomics.  The workspace holds
 * 56 N C K2 bytes (seven 64-bit words per sum); the entry clears it, and counts_out, itself.  Two launches. */
int fslic_hip_region_sums_workspace_size(int N, int C, int K2, size_t* bytes);
int fslic_hip_region_sums(int device, void* stream, int N, int C, int K, int K2, const float* values, const int32_t* mapping,
                          const void* counts, int counts_type, float* sums, void* counts_out, void* workspace, size_t workspace_bytes);
/* Edge weights of a graph (edge_index, offsets, E as for merging) from sums (float [N][C][K]) and counts ([N][K] of counts_type).
 * For the edge (a, b) of frame n: na = (float)counts[n][a], d_c = sums[n][c][a] / na - sums[n][c][b] / nb, s = the d_c * d_c added in
 * ascending c; mode 0 (mean): weight = sqrt(s); mode 1 (ward): weight = ((na * nb) / (na + nb)) * s.  Every operation is one IEEE
 * float operation rounded on its own, nothing fused, division and square root correctly rounded.  +inf where a or b is outside
 * [0, K) or a count is <= 0.  One launch, no workspace; E == 0: nothing is launched. */
int fslic_hip_region_edge_weights(int device, void* stream, int N, int C, int K, long long E, const int64_t* edge_index,
                                  const int64_t* offsets, const float* sums, const void* counts, int counts_type, int mode, float* weight);

/* ---- Aggregation over neighbour lists (NEW surface; Python: fast_slic_amd/propagate.py, which states the rules) ----
 * Entries as for the regions: a device index and a stream, no synchronisation, no allocation, no workspace, no copy to the host, the
 * caller's device restored, every argument checked before the first HIP call (FSLIC_E_INVALID).  N frames, C >= 1 channels, K in
 * [1, 65534] nodes, N * C * K below 2^31, nnz in [0, 2^31) entries.  The lists are one CSR over the N * K rows (frame, node):
 * offsets int64 [N * K + 1], indices int32 [nnz] (node numbers inside the frame), weight float [nnz] or NULL.  What the device arrays
 * hold is checked by the kernels before it becomes an address: row bounds are clamped into [0, nnz], an end before its start is an
 * empty row, and an entry whose index is outside [0, K) is not valid and contributes nothing.  Every float operation is one IEEE
 * operation rounded on its own, nothing fused, the division correctly rounded; no atomics: the same bits from run to run.
 *
 * Forward.  reduce 0 (sum): out[n][c][i] = the left fold from +0.0 over the valid entries p of row (n, i), ascending, of
 * weight[p] * values[n][c][indices[p]] (values[...] itself without a weight).  reduce 1 (mean): that sum without a weight, divided by
 * (float)d, d = the row's valid entries, +0.0 for d = 0; degree (int32 [N * K], required) receives d.  reduce 2 (max): the largest
 * value over the valid entries, +0.0 for d = 0; argmax (int32 [N][C][K], required) receives the smallest p that attains it, -1 for
 * d = 0; NaN values leave the cell unspecified.  A weight goes with reduce 0 only.  One launch. */
int fslic_hip_aggregate_forward(int device, void* stream, int N, int C, int K, long long nnz, int reduce, const int64_t* offsets,
                                const int32_t* indices, const float* weight, const float* values, float* out, int32_t* argmax, int32_t* degree);
/* Backward to the values over the transposed lists: the entries whose index is node j of frame n are t_entries[t_offsets[n * K + j] ..
 * t_offsets[n * K + j + 1]) (int32 [nnz], ascending), t_rows (int32 [nnz]) the row over (frame, node) of each; an entry outside
 * [0, nnz) or a row outside frame n contributes nothing.  grad_values[n][c][j] = the left fold from +0.0 over them of
 * weight[p] * grad_out[n][c][row(p)] (sum; grad_out[...] itself without a weight), grad_out[n][c][row(p)] / (float)degree[row(p)]
 * (mean; degree as the forward wrote it), or grad_out[n][c][row(p)] where argmax[n][c][row(p)] == p (max).  One launch. */
int fslic_hip_aggregate_backward_values(int device, void* stream, int N, int C, int K, long long nnz, int reduce, const int64_t* t_offsets,
                                        const int32_t* t_entries, const int32_t* t_rows, const float* weight, const int32_t* argmax,
                                        const int32_t* degree, const float* grad_out, float* grad_values);
/* Backward of the sum to the weights: grad_weight[p] = the left fold from +0.0 over c = 0 .. C - 1 of values[n][c][indices[p]] *
 * grad_out[n][c][i], with (n, i) = rows[p] (int32 [nnz], the row over (frame, node) of each entry); +0.0 where rows[p] is outside
 * [0, N * K) or indices[p] outside [0, K).  One thread an entry; one launch, none for nnz == 0. */
int fslic_hip_aggregate_backward_weight(int device, void* stream, int N, int C, int K, long long nnz, const int32_t* rows, const int32_t* indices,
                                        const float* values, const float* grad_out, float* grad_weight);

/* ---- Attention over neighbour lists (NEW surface; Python: fast_slic_amd/attention.py, which states the rules) ----
 * Entries, lists, limits and the treatment of what the device arrays hold as for the aggregation above.  heads >= 1 divides C; D =
 * C / heads channels a head, head h owns the channels h D .. h D + D - 1; a per-entry array is float [heads][nnz], the entries
 * innermost, heads * nnz below 2^31.  An entry p is valid when it lies inside the clamped bounds of a row and indices[p] is inside
 * [0, K).  Every float operation is one IEEE operation rounded on its own, nothing fused, the division correctly rounded, the
 * exponential the one of fslic_hip_crf_expf_host(.., use_libm = 0); no atomics: the same bits from run to run.  No output overlaps an
 * input.
 *
 * Dot.  out[h][p] = the left fold from +0.0 over c = h D .. h D + D - 1 of a[n][c][i] * b[n][c][indices[p]], with (n, i) = rows[p]
 * (int32 [nnz], the row over (frame, node) of each entry); +0.0 where rows[p] is outside [0, N * K) or indices[p] outside [0, K).
 * One thread per (head, entry); one launch, none for nnz == 0. */
int fslic_hip_attend_dot(int device, void* stream, int N, int C, int K, long long nnz, int heads, const int32_t* rows, const int32_t* indices,
                         const float* a, const float* b, float* out);
/* Softmax over the valid entries of each row, per head: m = their largest score, e = expf(scores[h][p] - m), Z = the left fold from
 * +0.0 of e in ascending p, out[h][p] = e / Z; +0.0 for every entry that is not valid.  Defined for rows whose valid scores are
 * finite or -inf with at least one finite; NaN and +inf leave the row unspecified.  One launch, none for nnz == 0. */
int fslic_hip_attend_softmax(int device, void* stream, int N, int K, long long nnz, int heads, const int64_t* offsets, const int32_t* indices,
                             const float* scores, float* out);
/* Its backward from alpha (what the forward wrote): t = the left fold from +0.0 over the row's valid entries of alpha[h][p] *
 * grad_out[h][p]; grad_scores[h][p] = alpha[h][p] * (grad_out[h][p] - t), +0.0 for an entry that is not valid.  One launch. */
int fslic_hip_attend_softmax_backward(int device, void* stream, int N, int K, long long nnz, int heads, const int64_t* offsets,
                                      const int32_t* indices, const float* alpha, const float* grad_out, float* grad_scores);
/* The neighbour sum with one weight per head (weight float [heads][nnz]).  transposed 0: ia = indices, ib is not read; dst[n][c][i] =
 * the left fold from +0.0 over the valid entries p of row (n, i), ascending, of weight[h(c)][p] * src[n][c][indices[p]], h(c) =
 * c / D.  transposed 1: offsets, ia, ib = t_offsets, t_entries, t_rows of the transposed lists as in
 * fslic_hip_aggregate_backward_values; dst[n][c][j] = the fold over them of weight[h(c)][p] * src[n][c][row(p)].  With heads == 1 the
 * bits of fslic_hip_aggregate_forward / _backward_values with reduce 0 and this weight.  The two are the gradients of the dot (to a
 * with src = b, to b with src = a, weight = grad_out) and the dot is the gradient of this sum to its weight.  One launch. */
int fslic_hip_attend_apply(int device, void* stream, int N, int C, int K, long long nnz, int heads, int transposed, const int64_t* offsets,
                           const int32_t* ia, const int32_t* ib, const float* weight, const float* src, float* dst);

/* ---- exact k nearest neighbours in feature space (NEW surface; Python: fast_slic_amd/knn.py) ----
 * For every node i of every frame f of `points` (float [N][D][K], the node innermost) the k nearest nodes j of the same frame of
 * `other` (the same layout; NULL: of `points` itself, and then j != i unless `loop` is not 0) by the squared Euclidean distance
 *     d(i, j) = the left fold from +0.0f over c = 0 .. D - 1 of  t = points[f][c][i] - other[f][c][j],  acc = acc + t * t
 * three separately rounded float operations a channel, nothing fused.  `valid` (one byte per node, [N][K], 0 = invalid; NULL: all
 * valid) describes the nodes of both arrays: an invalid node is no candidate and its own row is all padding.  A NaN distance is no
 * candidate, +inf is an ordinary distance.  indices (int32) and dist (float), both [N * K][k], take the k smallest candidates of
 * every row in the total order (d, j), ascending, and -1 / +inf behind the last one.  The result does not depend on the launch shape
 * and is the same bits from run to run; no atomics, no workspace, one launch.  1 <= k <= 32, N * K * k < 2^31; `loop` together with
 * `other` is refused.  Entries as for pooling: a device index and a stream, no synchronisation, no allocation, every argument checked
 * before the first HIP call (FSLIC_E_INVALID).  No output overlaps an input. */
int fslic_hip_knn_graph(int device, void* stream, int N, int D, int K, int k, int loop, const float* points, const float* other,
                        const uint8_t* valid, int32_t* indices, float* dist);

/* ---- Messages over neighbour lists (NEW surface; Python: fast_slic_amd/messages.py, which states the rules) ----
 * Entries, lists, limits and the treatment of what the device arrays hold as for the aggregation above.  A per-entry array is float
 * [C][nnz], the entries innermost, C * nnz below 2^31; the node side is float [N][C][K].  An entry p is valid when it lies inside the
 * clamped bounds of a row and indices[p] is inside [0, K).  Every float operation is one IEEE operation rounded on its own, nothing
 * fused, the division correctly rounded; no atomics: the same bits from run to run.  No output overlaps an input.
 *
 * Gather, nodes -> entries.  out[c][p] = values[n][c][node] with (n, i) = rows[p] (int32 [nnz], the row over (frame, node) of each
 * entry) and node = i (end 0, the target) or indices[p] (end 1, the source): a copy, NaN and the sign of zero pass through.  +0.0
 * where rows[p] is outside [0, N * K) or indices[p] outside [0, K).  Two optional arrays serve the backward of the reduce below:
 * scale_degree (int32 [N * K], or NULL): the value is divided by (float)scale_degree[n * K + node]; argmax (int32 [N][C][K], or NULL):
 * +0.0 unless argmax[n][c][node] == p.  One thread per (channel, entry); one launch, none for nnz == 0. */
int fslic_hip_message_gather(int device, void* stream, int N, int C, int K, long long nnz, int end, const int32_t* rows, const int32_t* indices,
                             const float* values, const int32_t* scale_degree, const int32_t* argmax, float* out);
/* Reduce, entries -> nodes.  transposed 0: ia = indices, ib is not read; out[n][c][i] folds messages[c][p] over the valid entries p of
 * row (n, i), ascending.  transposed 1: offsets, ia, ib = t_offsets, t_entries, t_rows of the transposed lists as in
 * fslic_hip_aggregate_backward_values; out[n][c][j] folds messages[c][t_entries[q]] over the positions q of target (n, j), ascending
 * (an entry outside [0, nnz) or a row outside frame n contributes nothing).  reduce 0 (sum): the left fold from +0.0.  1 (mean): that
 * sum divided by (float)d, d = the terms of the fold, +0.0 for d = 0; degree (int32 [N * K], required) receives d.  2 (max), 3 (min):
 * the extremum, +0.0 for d = 0; argmax (int32 [N][C][K], required) receives the entry p it was first met at (the smallest such p),
 * -1 for d = 0; NaN leaves the cell unspecified.  The gather above is the gradient of this reduce (of the mean with scale_degree =
 * degree, of the max and min with argmax), and the sum is the gradient of the gather: transposed 0 for end 0, 1 for end 1.  One
 * launch, also for nnz == 0 (zeros, -1, 0). */
int fslic_hip_message_reduce(int device, void* stream, int N, int C, int K, long long nnz, int reduce, int transposed, const int64_t* offsets,
                             const int32_t* ia, const int32_t* ib, const float* messages, float* out, int32_t* argmax, int32_t* degree);

/* ---- Pixels over neighbour lists (NEW surface; Python: fast_slic_amd/pixels.py, which states the rules) ----
 * Entries as for pooling: a device index and a stream, no synchronisation, no allocation, every argument checked before the first HIP
 * call (FSLIC_E_INVALID).  labels: the map of fslic_hip_pool, N x H x W of label_type, a value outside [0, K) is no label; offsets
 * int64 [N * K + 1] and indices int32 [nnz] (NULL only with nnz == 0): the lists of the aggregation above, with its treatment of what
 * the device arrays hold.  Every pixel has S slots, 1 <= S <= 32: slot 0 is its own label i, slot s >= 1 is entry lo + s - 1 of row
 * (n, i), [lo, hi) the row's bounds clamped into [0, nnz]; it is empty unless that entry lies below hi and its index inside [0, K),
 * and every slot of a pixel without a label is empty.  Pixel features are float [N][C][H][W], node features float [N][C][K], a per-slot
 * array float [N][heads][S][H][W]; C % heads == 0, head h owns the channels h D .. h D + D - 1, D = C / heads.  Limits: N * C * K,
 * N * C * H * W, N * heads * S * H * W and nnz below 2^31.  Every float operation is one IEEE operation rounded on its own, nothing
 * fused, the division correctly rounded; no float atomics: the same bits from run to run.  No output overlaps an input.
 *
 * Dot: out[n][h][s][y][x] = the left fold from +0.0 over the head's channels c, ascending, of a[n][c][y][x] * b[n][c][j], j the node of
 * the slot; +0.0 for an empty slot.  One launch. */
int fslic_hip_pixel_dot(int device, void* stream, int N, int C, int H, int W, int K, int S, int heads, long long nnz, int label_type,
                        const void* labels, const int64_t* offsets, const int32_t* indices, const float* a, const float* b, float* out);
/* Mix: out[n][c][y][x] = the left fold from +0.0 over the pixel's non-empty slots s, ascending, of weight[n][h(c)][s][y][x] *
 * values[n][c][j].  One launch. */
int fslic_hip_pixel_mix(int device, void* stream, int N, int C, int H, int W, int K, int S, int heads, long long nnz, int label_type,
                        const void* labels, const int64_t* offsets, const int32_t* indices, const float* values, const float* weight, float* out);
/* Softmax over the non-empty slots of every (pixel, head); C is only checked (pass heads).  backward 0: in = scores; m = their maximum,
 * e = crf_expf(s - m), Z = the left fold of e from +0.0, out = e / Z; grad is not read.  backward 1: in = the alpha of the forward,
 * t = the left fold of alpha * grad, out = alpha * (grad - t).  +0.0 on every empty slot.  NaN or +inf leaves the pixel unspecified.
 * One launch. */
int fslic_hip_pixel_softmax(int device, void* stream, int N, int C, int H, int W, int K, int S, int heads, long long nnz, int label_type,
                            const void* labels, const int64_t* offsets, const int32_t* indices, int backward, const float* in, const float* grad,
                            float* out);
/* Scatter: out[n][c][j] = the sum of weight[n][h(c)][s][y][x] * x[n][c][y][x] over the pixels and slots that name node j, by the
 * contract of fslic_hip_pool's sum: one f32 partial per tile of 16 x 64 pixels, label, slot and channel (each product rounded once,
 * the order inside a tile fixed), truncated towards zero to a multiple of 2^-96; the partials are added exactly in fixed point and
 * the total is rounded once, ties to even, a zero total being +0.0.  Non-finite input leaves the entry unspecified.  The workspace
 * (8-byte aligned, 56 N C K bytes: the accumulator) is zeroed on the stream; three operations on the stream. */
int fslic_hip_pixel_scatter_workspace_size(int N, int C, int K, size_t* bytes);
int fslic_hip_pixel_scatter(int device, void* stream, int N, int C, int H, int W, int K, int S, int heads, long long nnz, int label_type,
                            const void* labels, const int64_t* offsets, const int32_t* indices, const float* x, const float* weight, float* out,
                            void* workspace, size_t workspace_bytes);

/* ---- SimpleCRF inference on device tensors (NEW surface, no counterpart in the reference; Python: fast_slic_amd/crf_torch.py) ----
 * The inference of fslic_hip_crf_inference (same arithmetic, bit for bit) for a caller who holds everything in device memory: no CRF
 * object, no host state.  Entries as for pooling: a device index and a stream, no synchronisation, no allocation, the caller's device
 * restored, every argument checked before the first HIP call (FSLIC_E_INVALID).  Every pointer but `params` is device memory:
 *   unaries, q0, q_out : float [N][C][K] (energies; q0 NULL: crf_expf(-unaries), what fslic_hip_crf_initialize sets; q0 is only read;
 *                        q_out overlaps no input)             compat : float [C]
 *   yxrgb   : float [N][5][K], the Cluster's y, x, r, g, b   members : int32 [N][K], the 32 bits of the Cluster's num_members
 *   offsets : int64 [N * K + 1], indices : int32 [nnz] (NULL only with nnz == 0): one CSR over (frame, node); an index is a node
 *             number inside its frame.  Rows may be empty, of any length, asymmetric, and hold duplicates and self-loops.  An index
 *             outside [0, K) contributes nothing.  Row bounds are clamped into [0, nnz] and to end >= begin before use, so no offset
 *             or index of any value leads to an access out of range (rows that overlap after that give unspecified energies).
 * temporal 0: N independent frames.  temporal 1: N consecutive times of one window, node i of frame n linked to node i of n - 1 and
 * n + 1 as in SimpleCRF.  max_iter Jacobi sweeps; the result is in q_out whatever max_iter is (0: the starting q).
 * Limits: N * C * K, N * K + 1 and nnz below 2^31.  The workspace (16-byte aligned) holds 24 N K + 8 nnz + 4 N C K bytes, and
 * 4 N C K more above 128 classes (each part rounded up to 16): row bounds, temporal and neighbour energies, the second q buffer,
 * and the message plane of the sweeps whose classes do not fit LDS. */
int fslic_hip_crf_tensor_workspace_size(int N, int C, int K, long long nnz, size_t* bytes);
int fslic_hip_crf_tensor_inference(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                   const fslic_crf_params* params, const float* compat, const float* yxrgb, const int32_t* members,
                                   const int64_t* offsets, const int32_t* indices, long long nnz,
                                   const float* unaries, const float* q0 /* NULL: expf(-unaries) */, float* q_out,
                                   void* workspace, size_t workspace_bytes);

/* ---- The backward of that inference (kernels in csrc/crf_tensor_grad.hip; Python: the autograd path of superpixel_crf) ----
 * fslic_hip_crf_tensor_inference_saved is fslic_hip_crf_tensor_inference with every iterate kept: q_all is float
 * [max_iter + 1][N][C][K], plane 0 the starting q, plane t + 1 what sweep t writes (the same kernels: the last plane is bit-equal to
 * q_out of the other entry).  fslic_hip_crf_tensor_backward takes that q_all, the same inputs and grad_q [N][C][K], the gradient of a
 * scalar with respect to the last plane, and writes the gradient with respect to
 *   unaries     -> grad_unaries [N][C][K] (always),
 *   q0          -> grad_q0 [N][C][K]; NULL says that the forward had q0 == NULL, its start crf_expf(-unaries) then adds to grad_unaries,
 *   compat      -> grad_compat [C], or NULL: that pass is skipped.
 * Nothing flows to yxrgb, members or the graph (for params and the energies see the _energies entries below).  One launch per sweep, last sweep first, gathers over the TRANSPOSED lists:
 * t_offsets int64 [N * K + 1] over (frame, target node), and per transposed entry the neighbour entry t_entries int32 [nnz] and its
 * row t_rows int32 [nnz] over (frame, node), in ascending entry order inside one target (both NULL only with nnz == 0).  No float
 * atomics: every output cell has one owner and every sum a fixed order, so two calls give the same bits.  No transposed list of any
 * content leads to an access out of range: bounds are clamped as a row's are, and an entry counts only when its row is a node of the
 * target's frame, its number lies inside that row's clamped bounds, and its index is inside [0, K); lists that are not the transpose
 * of the CSR give unspecified gradients.  Output buffers overlap no input and each other not.
 * The workspace (16-byte aligned parts): 24 N K + 8 nnz bytes of row bounds and energies, and above 128 classes 4 N C K of messages;
 * with backward == 1 also 8 N C K of message gradients, above 128 classes 4 N C K more, and with with_compat == 1 (grad_compat given)
 * 4 C N ceil(K / 64) bytes of per-block sums. */
int fslic_hip_crf_tensor_grad_workspace_size(int N, int C, int K, long long nnz, int backward, int with_compat, size_t* bytes);
int fslic_hip_crf_tensor_inference_saved(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                         const fslic_crf_params* params, const float* compat, const float* yxrgb, const int32_t* members,
                                         const int64_t* offsets, const int32_t* indices, long long nnz,
                                         const float* unaries, const float* q0 /* NULL: expf(-unaries) */, float* q_all,
                                         void* workspace, size_t workspace_bytes);
int fslic_hip_crf_tensor_backward(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                  const fslic_crf_params* params, const float* compat, const float* yxrgb, const int32_t* members,
                                  const int64_t* offsets, const int32_t* indices, long long nnz,
                                  const int64_t* t_offsets, const int32_t* t_entries, const int32_t* t_rows,
                                  const float* unaries, const float* q_all, const float* grad_q,
                                  float* grad_unaries, float* grad_q0, float* grad_compat, void* workspace, size_t workspace_bytes);

/* ---- The energies of that inference as tensors (kernels in csrc/crf_tensor.hip, csrc/crf_tensor_grad.hip; Python: crf_edge_energies
 * and the params tensor and energies arguments of superpixel_crf) ----
 * fslic_hip_crf_tensor_energies writes what the inference above computes for itself: edge float [nnz], the spatial energy of every
 * neighbour entry of the CSR (0.0 for a self-loop, for an index outside [0, K) and for an entry outside every clamped row), and links
 * float [N][2][K], the temporal energy of node i of frame n towards n - 1 (links[n][0][i]) and n + 1 (links[n][1][i]), 0.0 where there
 * is no such frame or temporal is 0.  params is DEVICE memory here: the seven floats of fslic_crf_params in its order; the values are
 * the very floats of the inference with the same params.  edge may be NULL only with nnz == 0.
 * fslic_hip_crf_tensor_energies_backward takes grad_edge [nnz] and grad_links [N][2][K], the gradients of a scalar with respect to
 * those two (either may be NULL: zero), and writes its gradient with respect to the params, grad_params float [7]: every term in
 * double, added in a fixed order (per row in entry order, a fixed tree per block of 256 rows, the blocks in ascending order), rounded
 * once.  Self-loops and dead entries contribute nothing; nothing flows to yxrgb.  Its workspace (16-byte aligned) holds
 * 56 ceil(N K / 256) bytes rounded up to 16.
 * The three _energies entries are fslic_hip_crf_tensor_inference, _inference_saved and _backward with the energies given: edge [nnz]
 * (NULL only with nnz == 0) and links [N][2][K] (NULL: no temporal energy) take the place of params and yxrgb; the weight of entry k
 * is edge[k] times the member factor, also for a self-loop.  Workspaces are those of the entries they mirror
 * (fslic_hip_crf_tensor_workspace_size, fslic_hip_crf_tensor_grad_workspace_size).  The backward also writes, when the pointer is
 * given, grad_edge [nnz] and grad_links [N][2][K]: zeroed on the stream, then behind each sweep's adjoint one launch adds
 *   grad_edge[k] += f_k sum_c dm[row(k)][c] q[j_k][c],   grad_links[n][0][i] += f sum_c dm[n][c][i] q[n - 1][c][i]   ([n][1][i]: n + 1)
 * with dm the gradient of that sweep's messages, q its input iterate and f the member factor (no gradient flows through it); classes
 * in ascending order, sweeps last to first, one owner thread per cell, no atomics.  An index outside [0, K), an entry outside every
 * clamped row, the link cells at the window's ends and all of grad_links with temporal == 0 get 0.0. */
int fslic_hip_crf_tensor_energies(int device, void* stream, int N, int K, int temporal, const float* params /* device, [7] */,
                                  const float* yxrgb, const int32_t* members, const int64_t* offsets, const int32_t* indices,
                                  long long nnz, float* edge, float* links);
int fslic_hip_crf_tensor_energies_backward_workspace_size(int N, int K, size_t* bytes);
int fslic_hip_crf_tensor_energies_backward(int device, void* stream, int N, int K, int temporal, const float* params /* device, [7] */,
                                           const float* yxrgb, const int64_t* offsets, const int32_t* indices, long long nnz,
                                           const float* grad_edge, const float* grad_links, float* grad_params,
                                           void* workspace, size_t workspace_bytes);
int fslic_hip_crf_tensor_inference_energies(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                            const float* compat, const int32_t* members, const int64_t* offsets, const int32_t* indices,
                                            long long nnz, const float* edge, const float* links,
                                            const float* unaries, const float* q0 /* NULL: expf(-unaries) */, float* q_out,
                                            void* workspace, size_t workspace_bytes);
int fslic_hip_crf_tensor_inference_saved_energies(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                                  const float* compat, const int32_t* members, const int64_t* offsets,
                                                  const int32_t* indices, long long nnz, const float* edge, const float* links,
                                                  const float* unaries, const float* q0 /* NULL: expf(-unaries) */, float* q_all,
                                                  void* workspace, size_t workspace_bytes);
int fslic_hip_crf_tensor_backward_energies(int device, void* stream, int N, int C, int K, int temporal, int max_iter,
                                           const float* compat, const int32_t* members, const int64_t* offsets, const int32_t* indices,
                                           long long nnz, const float* edge, const float* links,
                                           const int64_t* t_offsets, const int32_t* t_entries, const int32_t* t_rows,
                                           const float* unaries, const float* q_all, const float* grad_q,
                                           float* grad_unaries, float* grad_q0, float* grad_compat, float* grad_edge, float* grad_links,
                                           void* workspace, size_t workspace_bytes);

/* ---- Soft superpixel assignment on feature planes (NEW surface, no counterpart in the reference; Python: fast_slic_amd/soft.py) ----
 * SLIC's k-means on float feature planes over a regular grid of gh x gw seed cells with soft assignments: every pixel is distributed over
 * the 3 x 3 cells around its own (Superpixel Sampling Networks, Jampani et al. 2018).  Entries as for pooling: a device index and a
 * stream, no synchronisation, no allocation, no workspace, the caller's device restored, every argument checked before the first HIP call
 * (FSLIC_E_INVALID): N, C >= 1, H * W < 2^31, 1 <= gh <= H, 1 <= gw <= W, K = gh * gw <= 65534.
 *   features : float [N][C][H][W]     centres, values, sums : float [N][C][K]     q, grad_q, grad_d : float [N][9][H][W]     weights : float [N][K]
 * Pixel (y, x) lies in cell (cy, cx) = ((y * gh) / H, (x * gw) / W) (integers).  Slot j = 3 (dy + 1) + (dx + 1), dy, dx in {-1, 0, 1}, of
 * a pixel names cell (cy + dy, cx + dx), superpixel k_j = (cy + dy) * gw + (cx + dx); a slot outside the grid is invalid: it takes part
 * in no sum, and every output plane holds +0.0 there.  j_k(p) is the slot of pixel p that names k.  No atomics: every result is
 * bitwise reproducible and independent of the batch position and of the other channels. */
/* d_j = sum_c (F[c][p] - S[c][k_j])^2;  q_j = exp(-(d_j - min d)) / sum over the valid slots. */
int fslic_hip_soft_assign(int device, void* stream, int N, int C, int H, int W, int gh, int gw, const float* features,
                          const float* centres, float* q);
/* grad_d_j = -q_j (grad_q_j - sum_i grad_q_i q_i);  grad_features[c][p] = 2 sum_j grad_d_j (F[c][p] - S[c][k_j]).  The gradient of the
 * centres is -2 times fslic_hip_soft_pool(features, grad_d, centres). */
int fslic_hip_soft_assign_backward(int device, void* stream, int N, int C, int H, int W, int gh, int gw, const float* features,
                                   const float* centres, const float* q, const float* grad_q, float* grad_d, float* grad_features);
/* sums[c][k] = sum_p q_{j_k(p)}(p) F[c][p] over the pixels of the 3 x 3 cell window of k, with centres (optional) the sum of
 * q_{j_k(p)}(p) (F[c][p] - centres[c][k]);  weights (optional) [k] = sum_p q_{j_k(p)}(p). */
int fslic_hip_soft_pool(int device, void* stream, int N, int C, int H, int W, int gh, int gw, const float* features, const float* q,
                        const float* centres, float* sums, float* weights);
/* out[c][p] = sum over the valid slots of q_j(p) values[c][k_j]. */
int fslic_hip_soft_unpool(int device, void* stream, int N, int C, int H, int W, int gh, int gw, const float* values, const float* q,
                          float* out);
/* out_j(p) = sum_c a[c][p] b[c][k_j] + bias[k_j] (a: [N][C][H][W], b: [N][C][K], bias: [N][K] or NULL): the gradient of soft_pool and
 * of soft_unpool with respect to q. */
int fslic_hip_soft_dot(int device, void* stream, int N, int C, int H, int W, int gh, int gw, const float* a, const float* b,
                       const float* bias, float* out);

const char* fslic_hip_last_error(void);
const char* fslic_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FSLIC_HIP_H */
