"""ctypes binding of the C ABI in include/fslic_hip.h.

Plays the role cfast_slic.pyx plays in the reference: `SlicModel` owns the Cluster[K] block, forwards
`initialize` / `iterate` to the engine and converts the uint16 label map to the int16 map the
reference returns (cfast_slic.pyx:258-260).  Only the arch "hip/gfx950" exists here; the reference's
CPU archs stay in the reference.  There is deliberately NO CPU fallback: if the HIP library is
missing or no GPU is visible, constructing a SlicModel raises.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

ARCH_NAME = "hip/gfx950"
_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libfslic_hip.so")

CLUSTER_DTYPE = np.dtype([
    ("y", "<f4"), ("x", "<f4"), ("r", "<f4"), ("g", "<f4"), ("b", "<f4"), ("a", "<f4"),
    ("number", "<u2"), ("is_active", "u1"), ("is_updatable", "u1"), ("num_members", "<u4"),
])  # src/fast-slic-common.h:10-23
assert CLUSTER_DTYPE.itemsize == 32

FSLIC_OK, FSLIC_E_INVALID, FSLIC_E_UNSUPPORTED, FSLIC_E_HIP, FSLIC_E_INTERNAL = range(5)


class Params(C.Structure):
    _fields_ = [
        ("max_iter", C.c_int32), ("compactness", C.c_float), ("min_size_factor", C.c_float),
        ("subsample_stride", C.c_int32), ("convert_to_lab", C.c_int32),
        ("manhattan_spatial_dist", C.c_int32), ("preemptive", C.c_int32),
        ("preemptive_thres", C.c_float), ("num_threads", C.c_int32), ("debug_mode", C.c_int32),
        ("abi", C.c_int32), ("variant", C.c_int32), ("reserved", C.c_int32 * 4),
    ]


def _signatures():
    """(name, restype, argtypes) of every entry point of include/fslic_hip.h, once (tests/test_capi_cpu.py holds it against the header)."""
    vp, i32, i64, sz, f32, f64, text = C.c_void_p, C.c_int, C.c_longlong, C.c_size_t, C.c_float, C.c_double, C.c_char_p
    P = C.POINTER
    params = P(Params)
    frames = [i32, i32, i32, i32, vp, vp, vp]      # H, W, K, n_frames, rgb, clusters, labels: one pointer array each
    table = [
        ("fslic_hip_device_count", i32, []),
        ("fslic_hip_create", i32, [i32, i32, P(vp)]),
        ("fslic_hip_destroy", None, [vp]),
        ("fslic_hip_initialize_clusters", i32, [i32, i32, i32, vp, vp]),
        ("fslic_hip_seed_positions", i32, [i32, i32, i32, vp]),
        ("fslic_hip_iterate", i32, [vp, params, i32, i32, i32, vp, vp, vp]),
        ("fslic_hip_iterate_device", i32, [vp, i32, params, i32, i32, i32, vp, vp, vp]),
        ("fslic_hip_iterate_batch", i32, [vp, params] + frames + [i32]),
        ("fslic_hip_submit_group", i32, [vp, i32, params] + frames),
        ("fslic_hip_wait_group", i32, [vp, i32]),
        ("fslic_hip_rgb_to_lab", i32, [vp, i32, i32, vp, i32, vp]),
        ("fslic_hip_enforce_connectivity", i32, [vp, vp, i32, i32, i32, i32]),
        ("fslic_hip_enforce_connectivity_nodes", i32, [vp, vp, i32, i32, i32, i32, P(C.c_uint32)]),
        ("fslic_hip_last_prelabels", i32, [vp, i32, vp]),
        ("fslic_hip_last_timing_report", text, [vp]),
        ("fslic_hip_last_device_times", i32, [vp, i32, P(f32), P(f32)]),
        ("fslic_hip_set_launch_timing", i32, [vp, i32]),
        ("fslic_hip_last_assign_loop", i32, [vp, i32, P(f32), P(f64), P(i32)]),
        ("fslic_hip_last_group_frames", i32, [vp, i32]),
        ("fslic_hip_last_path", i32, [vp, i32]),
        ("fslic_hip_last_launch_mode", i32, [vp, i32]),
        ("fslic_hip_group_done", i32, [vp, i32]),
        ("fslic_hip_last_error", text, []),
        ("fslic_hip_version", text, []),
        ("fslic_hip_get_connectivity", i32, [vp, i32, i32, i32, vp, vp, vp]),
        ("fslic_hip_knn_connectivity", i32, [i32, i32, i32, vp, sz, vp, vp]),
        ("fslic_hip_get_mask_density", i32, [vp, i32, i32, i32, vp, vp, vp, vp]),
        ("fslic_hip_cluster_density_to_mask", i32, [vp, i32, i32, i32, vp, vp, vp]),
        ("fslic_hip_pipeline_submit", i32, [vp, params] + frames),
        ("fslic_hip_pipeline_drain", i32, [vp, P(f64), P(i64), P(i64), P(i64)]),
        ("fslic_hip_pipeline_batching", i32, [vp, i32]),
        ("fslic_hip_last_host_topk_frames", i32, [vp, i32]),
        ("fslic_hip_separate_pass_redos", i32, [vp, i32]),
        ("fslic_hip_uncovered_redos", i32, [vp, i32]),
        ("fslic_hip_overlapped_groups", i64, [vp]),
        ("fslic_hip_pipeline_overlap", i32, [vp, i32]),
        ("fslic_hip_copy_bandwidth", i32, [vp, sz, i32, P(f64)]),
        ("fslic_hip_last_recorder_report", i32, [vp, P(text), P(sz)]),
        ("fslic_hip_debug_lsc_state", i32, [vp, i32, i32, i32, vp, vp]),
        ("fslic_hip_debug_forms_seen", i32, [vp, i32, i32]),
        ("fslic_hip_debug_forms_all", i32, [vp, i32]),
        # SimpleCRF (fast_slic_amd/crf.py)
        ("fslic_hip_crf_new", i32, [sz, sz, P(vp)]),
        ("fslic_hip_crf_free", None, [vp]),
        ("fslic_hip_crf_copy", i32, [vp, P(vp)]),
        ("fslic_hip_crf_get_params", i32, [vp, vp]),
        ("fslic_hip_crf_set_params", i32, [vp, vp]),
        ("fslic_hip_crf_set_compat", i32, [vp, i32, f32]),
        ("fslic_hip_crf_get_compat", i32, [vp, i32, P(f32)]),
        ("fslic_hip_crf_num_classes", i32, [vp, P(sz), P(sz)]),
        ("fslic_hip_crf_first_time", i32, [vp]),
        ("fslic_hip_crf_last_time", i32, [vp]),
        ("fslic_hip_crf_num_frames", sz, [vp]),
        ("fslic_hip_crf_pop_frame", i32, [vp]),
        ("fslic_hip_crf_push_frame", i32, [vp, P(vp)]),
        ("fslic_hip_crf_frame", i32, [vp, i32, P(vp)]),
        ("fslic_hip_crf_frame_time", i32, [vp]),
        ("fslic_hip_crf_frame_set_clusters", i32, [vp, vp]),
        ("fslic_hip_crf_frame_get_clusters", i32, [vp, vp]),
        ("fslic_hip_crf_frame_set_connectivity", i32, [vp, i32, vp, vp, sz]),
        ("fslic_hip_crf_frame_set_connectivity_csr", i32, [vp, i32, vp, vp]),
        ("fslic_hip_crf_frame_get_connectivity", i32, [vp, vp, vp]),
        ("fslic_hip_crf_frame_set_mask", i32, [vp, vp, f32]),
        ("fslic_hip_crf_frame_set_proba", i32, [vp, vp]),
        ("fslic_hip_crf_frame_set_unbiased", i32, [vp]),
        ("fslic_hip_crf_frame_set_unary", i32, [vp, vp]),
        ("fslic_hip_crf_frame_get_unary", i32, [vp, vp]),
        ("fslic_hip_crf_frame_spatial_energy", i32, [vp, i32, i32, P(f32)]),
        ("fslic_hip_crf_frame_temporal_energy", i32, [vp, vp, i32, P(f32)]),
        ("fslic_hip_crf_frame_get_inferred", i32, [vp, vp]),
        ("fslic_hip_crf_frame_reset_inferred", i32, [vp]),
        ("fslic_hip_crf_initialize", i32, [vp]),
        ("fslic_hip_crf_inference", i32, [vp, vp, sz]),
        ("fslic_hip_crf_expf_host", i32, [vp, vp, sz, i32]),
        ("fslic_hip_crf_expf_device", i32, [vp, vp, vp, sz]),
        # attention over neighbour lists (fast_slic_amd/attention.py); device, stream, N, [C,] K, nnz, heads first.  (The stream entries
        # from the pooling on are listed in the order of tests/test_stream_refusals_cpu.py; these have tests/test_attention_cpu.py.)
        ("fslic_hip_attend_dot", i32, [i32, vp, i32, i32, i32, i64, i32, vp, vp, vp, vp, vp]),
        ("fslic_hip_attend_softmax", i32, [i32, vp, i32, i32, i64, i32, vp, vp, vp, vp]),
        ("fslic_hip_attend_softmax_backward", i32, [i32, vp, i32, i32, i64, i32, vp, vp, vp, vp, vp]),
        ("fslic_hip_attend_apply", i32, [i32, vp, i32, i32, i32, i64, i32, i32, vp, vp, vp, vp, vp, vp]),
        # nearest neighbours in feature space (fast_slic_amd/knn.py; tests/test_knn_cpu.py); device, stream, N, D, K, k, loop first
        ("fslic_hip_knn_graph", i32, [i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        # messages over neighbour lists (fast_slic_amd/messages.py; tests/test_messages_cpu.py); device, stream, N, C, K, nnz first
        ("fslic_hip_message_gather", i32, [i32, vp, i32, i32, i32, i64, i32, vp, vp, vp, vp, vp, vp]),
        ("fslic_hip_message_reduce", i32, [i32, vp, i32, i32, i32, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        # pixels over neighbour lists (fast_slic_amd/pixels.py; tests/test_pixels_cpu.py); device, stream, N, C, H, W, K, S, heads, nnz,
        # label_type, labels, offsets, indices first
        ("fslic_hip_pixel_dot", i32, [i32, vp] + [i32] * 7 + [i64, i32, vp, vp, vp, vp, vp, vp]),
        ("fslic_hip_pixel_mix", i32, [i32, vp] + [i32] * 7 + [i64, i32, vp, vp, vp, vp, vp, vp]),
        ("fslic_hip_pixel_softmax", i32, [i32, vp] + [i32] * 7 + [i64, i32, vp, vp, vp, i32, vp, vp, vp]),
        ("fslic_hip_pixel_scatter_workspace_size", i32, [i32, i32, i32, P(sz)]),
        ("fslic_hip_pixel_scatter", i32, [i32, vp] + [i32] * 7 + [i64, i32, vp, vp, vp, vp, vp, vp, vp, sz]),
        # superpixel pooling (fast_slic_amd/pool.py)
        ("fslic_hip_pool_workspace_size", i32, [i32, i32, i32, i32, P(sz)]),
        ("fslic_hip_pool", i32, [i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, sz]),
        ("fslic_hip_pool_finalize", i32, [i32, vp, i32, i32, i32, i32, vp, sz, vp, vp, vp]),
        ("fslic_hip_unpool", i32, [i32, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, f32, vp]),
        # region adjacency graph (fast_slic_amd/rag.py)
        ("fslic_hip_rag_workspace_size", i32, [i32, i32, i32, i64, P(sz)]),
        ("fslic_hip_rag_accumulate", i32, [i32, vp, i32, i32, i32, i32, i32, vp, i32, vp, i32, i64, vp, sz]),
        ("fslic_hip_rag_compact", i32, [i32, vp, i32, i32, i64, vp, sz, vp, vp, vp, i64]),
        # two label maps against each other (fast_slic_amd/compare.py)
        ("fslic_hip_overlap_workspace_size", i32, [i32, i64, P(sz)]),
        ("fslic_hip_overlap_accumulate", i32, [i32, vp, i32, i32, i32, i32, i32, vp, i32, vp, i32, i64, vp, sz]),
        ("fslic_hip_overlap_compact", i32, [i32, vp, i32, i64, vp, sz, vp, vp, i64]),
        ("fslic_hip_boundary_match", i32, [i32, vp, i32, i32, i32, vp, i32, vp, i32, i32, vp]),
    ]
    # SimpleCRF inference on torch tensors (fast_slic_amd/crf_torch.py)
    sweep = [i32, vp, i32, i32, i32, i32, i32]      # device, stream, N, C, K, temporal, max_iter
    inference = sweep + [vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, sz]
    inference_energies = sweep + [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, sz]
    table += [
        ("fslic_hip_crf_tensor_workspace_size", i32, [i32, i32, i32, i64, P(sz)]),
        ("fslic_hip_crf_tensor_inference", i32, inference),
        ("fslic_hip_crf_tensor_grad_workspace_size", i32, [i32, i32, i32, i64, i32, i32, P(sz)]),
        ("fslic_hip_crf_tensor_inference_saved", i32, inference),
        ("fslic_hip_crf_tensor_backward", i32, sweep + [vp, vp, vp, vp, vp, vp, i64] + [vp] * 10 + [sz]),
        ("fslic_hip_crf_tensor_energies", i32, [i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, i64, vp, vp]),
        ("fslic_hip_crf_tensor_energies_backward_workspace_size", i32, [i32, i32, P(sz)]),
        ("fslic_hip_crf_tensor_energies_backward", i32, [i32, vp, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, sz]),
        ("fslic_hip_crf_tensor_inference_energies", i32, inference_energies),
        ("fslic_hip_crf_tensor_inference_saved_energies", i32, inference_energies),
        ("fslic_hip_crf_tensor_backward_energies", i32, sweep + [vp, vp, vp, vp, i64] + [vp] * 14 + [sz]),
    ]
    # soft superpixel assignment on feature tensors (fast_slic_amd/soft.py)
    geom = [i32, vp, i32, i32, i32, i32, i32, i32]      # device, stream, N, C, H, W, gh, gw
    table += [
        ("fslic_hip_soft_assign", i32, geom + [vp, vp, vp]),
        ("fslic_hip_soft_assign_backward", i32, geom + [vp, vp, vp, vp, vp, vp]),
        ("fslic_hip_soft_pool", i32, geom + [vp, vp, vp, vp, vp]),
        ("fslic_hip_soft_unpool", i32, geom + [vp, vp, vp]),
        ("fslic_hip_soft_dot", i32, geom + [vp, vp, vp, vp]),
    ]
    # connectivity on label tensors (fast_slic_amd/connect.py)
    head = [i32, vp, i32, i32, i32, vp, i32]      # device, stream, N, H, W, labels, label_type
    table += [
        ("fslic_hip_connect_workspace_size", i32, [i32, i32, i32, P(sz)]),
        ("fslic_hip_connected_components", i32, head + [vp, vp, vp, sz]),
        ("fslic_hip_connect_enforce", i32, head + [i64, vp, vp, vp, sz]),
    ]
    # merging on the region adjacency graph (fast_slic_amd/merge.py)
    graph = [i32, vp, i32, i32, i64, vp, vp]      # device, stream, N, K, E, edge_index, offsets
    table += [
        ("fslic_hip_merge_best_workspace_size", i32, [i32, i32, P(sz)]),
        ("fslic_hip_merge_best_edges", i32, graph + [vp, i32, f64, vp, vp, sz]),
        ("fslic_hip_merge_components_workspace_size", i32, [i32, i32, P(sz)]),
        ("fslic_hip_merge_components", i32, graph + [vp, vp, i32, vp, vp, vp, sz]),
        ("fslic_hip_merge_labels", i32, [i32, vp, i32, i32, i32, i32, vp, i32, vp, vp]),
        ("fslic_hip_merge_contract_accumulate", i32, [i32, vp, i32, i32, i32, i64, vp, vp, vp, vp, i32, vp, i64, vp, sz]),
        # the features of merged regions (fast_slic_amd/regions.py)
        ("fslic_hip_region_sums_workspace_size", i32, [i32, i32, i32, P(sz)]),
        ("fslic_hip_region_sums", i32, [i32, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, sz]),
        ("fslic_hip_region_edge_weights", i32, [i32, vp, i32, i32, i32, i64, vp, vp, vp, vp, i32, i32, vp]),
        # frames of any tensor layout into the engine's form (fast_slic_amd/frames.py)
        ("fslic_hip_pack_rgb", i32, [i32, vp, i32, i32, i32, vp, i32, P(i64), f32, vp, sz]),
    ]
    # aggregation over neighbour lists (fast_slic_amd/propagate.py)
    lists = [i32, vp, i32, i32, i32, i64]      # device, stream, N, C, K, nnz
    table += [
        ("fslic_hip_aggregate_forward", i32, lists + [i32, vp, vp, vp, vp, vp, vp, vp]),
        ("fslic_hip_aggregate_backward_values", i32, lists + [i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        ("fslic_hip_aggregate_backward_weight", i32, lists + [vp, vp, vp, vp, vp]),
    ]
    return table


SIGNATURES = _signatures()
EXPORTS = [name for name, _, _ in SIGNATURES]

_lib = None
_lib_lock = threading.Lock()

# ---- the record of kernel forms (include/fslic_hip.h: fslic_hip_debug_forms_seen / _all; csrc/forms.h) ----
FORM_FAMILIES = {1: "blk", 2: "bin", 3: "pre", 4: "k32", 5: "generic", 6: "generic_rec", 7: "preempt_update"}
FORM_TABLES = {0: "notab", 1: "rowvec", 2: "rowvec16", 3: "2d", 4: "tabs16", 5: "lut"}


def form_name(code):
    """A form code as words, e.g. 'blk r16 fused s2 rowvec nolab', 'k32 r8 full srt lut lab', 'preempt_update lists'."""
    code = int(code)
    family = FORM_FAMILIES.get(code & 15, "family%d" % (code & 15))
    if family == "preempt_update":
        return family + (" allpairs" if (code >> 18) & 1 else " lists")
    stride = (code >> 11) & 7
    words = [family]
    if (code >> 4) & 63:
        words.append("r%d" % ((code >> 4) & 63))
    words += ["fused" if (code >> 10) & 1 else "full", "s%d" % stride if stride else "srt",
              FORM_TABLES.get((code >> 14) & 7, "table%d" % ((code >> 14) & 7)), "nolab" if (code >> 17) & 1 else "lab"]
    return " ".join(words)


def _form_codes(fn, *extra):
    buf = (C.c_uint32 * 256)()
    n = int(fn(buf, 256, *extra))
    if n < 0 or n > 256:
        raise RuntimeError("the form record cannot be read (%d)" % n)
    return [int(buf[i]) for i in range(n)]


def forms_seen(clear=False):
    """Names of the kernel forms this process has enqueued since the record was last cleared (a set)."""
    return {form_name(c) for c in _form_codes(load_library().fslic_hip_debug_forms_seen, 1 if clear else 0)}


def forms_all():
    """Names of every form the dispatch can produce, in the order of the library's static tables (a list)."""
    return [form_name(c) for c in _form_codes(load_library().fslic_hip_debug_forms_all)]


def form_codes_all():
    return _form_codes(load_library().fslic_hip_debug_forms_all)


def build_library(force=False):
    """Compile fast_slic_amd/libfslic_hip.so for gfx950 with hipcc (in-tree, see csrc/Makefile)."""
    csrc = os.path.join(_HERE, "csrc")
    args = ["make", "-s", "-C", csrc]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return _LIB_PATH


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.  If this library pulled in the system runtime first
    and torch were imported afterwards, the process would hold two HIP runtimes and torch would report
    "No HIP GPUs are available".  When torch is installed (not necessarily imported) bind to ITS runtime, so
    device pointers from torch tensors and this engine share one runtime whatever the import order."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        _preload_torch_hip_runtime()
        if not os.path.exists(_LIB_PATH):
            raise ImportError(
                "fast_slic_amd: %s is missing; build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C fast_slic_amd/csrc` (there is no CPU fallback)" % _LIB_PATH)
        lib = C.CDLL(os.environ.get("FSLIC_LIB") or _LIB_PATH)      # FSLIC_LIB: A/B a second build of the same ABI (scripts/gpu_ab.sh)
        # A library given through FSLIC_LIB may be an older build of this ABI, without the entries added since: a name it lacks is
        # skipped, and only the features that need it then fail.  The last row is a testing aid that is not in include/fslic_hip.h.
        for name, restype, argtypes in SIGNATURES + [("fslic_hip_lab_force_generic", C.c_int, [C.c_void_p, C.c_int])]:
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
        return lib


def _raise(rc):
    msg = load_library().fslic_hip_last_error().decode("utf-8", "replace")
    if rc == FSLIC_E_INVALID:
        raise ValueError(msg)
    if rc == FSLIC_E_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(msg)


def _check(rc):
    if rc != FSLIC_OK:
        _raise(rc)


class Engine(object):
    """One GPU, `n_slots` frames in flight.  Thin owner of an fslic_engine handle."""

    def __init__(self, device=0, n_slots=1):
        lib = load_library()
        h = C.c_void_p()
        _check(lib.fslic_hip_create(int(device), int(n_slots), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.n_slots = int(n_slots)

    def close(self):
        if getattr(self, "_h", None):
            load_library().fslic_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stage entry points -------------------------------------------------------------
    def rgb_to_lab(self, image, convert=True):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        H, W, ch = image.shape
        if ch != 3:
            raise ValueError("nchan != 3")
        out = np.empty((H, W, 4), np.uint8)
        _check(load_library().fslic_hip_rgb_to_lab(self._h, H, W, image.ctypes.data, int(bool(convert)), out.ctypes.data))
        return out

    def enforce_connectivity(self, labels_u16, K, min_threshold):
        out = np.ascontiguousarray(labels_u16, dtype=np.uint16).copy()
        H, W = out.shape
        _check(load_library().fslic_hip_enforce_connectivity(self._h, out.ctypes.data, H, W, int(K), int(min_threshold)))
        return out

    def enforce_connectivity_nodes(self, labels_u16, K, min_threshold):
        """enforce_connectivity, and the number of union-find nodes the device pass kept for the frame."""
        out = np.ascontiguousarray(labels_u16, dtype=np.uint16).copy()
        H, W = out.shape
        n = C.c_uint32(0)
        _check(load_library().fslic_hip_enforce_connectivity_nodes(self._h, out.ctypes.data, H, W, int(K), int(min_threshold), C.byref(n)))
        return out, int(n.value)

    # ---- superpixel-graph utilities (src/fast-slic.cpp); labels / mask / result: numpy arrays or raw device pointers (int) ----
    @staticmethod
    def _plane(a, dtype):
        """(pointer, keep-alive) of a host array or of device memory given as an integer address."""
        if isinstance(a, (int, np.integer)):
            return C.c_void_p(int(a)), None
        arr = np.ascontiguousarray(a, dtype=dtype)
        return C.c_void_p(arr.ctypes.data), arr

    def get_connectivity(self, labels, H, W, K):
        ptr, keep = self._plane(labels, np.uint16)
        num = np.zeros(K, np.int32)
        nb = np.zeros((K, 12), np.uint32)
        _check(load_library().fslic_hip_get_connectivity(self._h, H, W, int(K), ptr, num.ctypes.data, nb.ctypes.data))
        return num, nb

    def get_mask_density(self, clusters, labels, mask, H, W):
        lp, k1 = self._plane(labels, np.uint16)
        mp, k2 = self._plane(mask, np.uint8)
        cl = np.ascontiguousarray(clusters)
        dens = np.zeros(cl.shape[0], np.uint8)
        _check(load_library().fslic_hip_get_mask_density(self._h, H, W, cl.shape[0], cl.ctypes.data, lp, mp, dens.ctypes.data))
        return dens

    def cluster_density_to_mask(self, labels, densities, H, W, out=None):
        lp, k1 = self._plane(labels, np.uint16)
        d = np.ascontiguousarray(densities, dtype=np.uint8)
        if out is None:
            res = np.empty((H, W), np.uint8)
            op = C.c_void_p(res.ctypes.data)
        else:
            res, op = out, C.c_void_p(int(out))
        _check(load_library().fslic_hip_cluster_density_to_mask(self._h, H, W, d.shape[0], lp, d.ctypes.data, op))
        return res

    def iterate(self, image, clusters, params):
        """Host numpy in, host numpy out (uint16 labels); clusters (CLUSTER_DTYPE[K]) updated in place."""
        H, W, _ = image.shape
        labels = np.empty((H, W), np.uint16)
        _check(load_library().fslic_hip_iterate(self._h, C.byref(params), H, W, clusters.shape[0],
                                                image.ctypes.data, clusters.ctypes.data, labels.ctypes.data))
        return labels

    def iterate_device(self, d_rgb_ptr, d_labels_ptr, H, W, clusters, params, slot=0):
        """Frame and label map resident in HBM (raw device pointers, e.g. torch tensor.data_ptr())."""
        _check(load_library().fslic_hip_iterate_device(self._h, int(slot), C.byref(params), H, W, clusters.shape[0],
                                                       C.c_void_p(d_rgb_ptr), clusters.ctypes.data, C.c_void_p(d_labels_ptr)))

    def iterate_batch(self, rgb_ptrs, cluster_arrays, label_ptrs, H, W, params, device_ptrs):
        n = len(rgb_ptrs)
        K = cluster_arrays[0].shape[0]
        PA = C.c_void_p * n
        a_rgb = PA(*[C.c_void_p(int(p)) for p in rgb_ptrs])
        a_cl = PA(*[C.c_void_p(c.ctypes.data) for c in cluster_arrays])
        a_lab = PA(*[C.c_void_p(int(p)) for p in label_ptrs])
        _check(load_library().fslic_hip_iterate_batch(self._h, C.byref(params), H, W, K, n,
                                                      C.cast(a_rgb, C.c_void_p), C.cast(a_cl, C.c_void_p),
                                                      C.cast(a_lab, C.c_void_p), int(bool(device_ptrs))))

    @staticmethod
    def pointer_array(ptrs):
        """A C array of pointers (kept alive by the caller) for submit_group / iterate_batch."""
        PA = C.c_void_p * len(ptrs)
        return PA(*[C.c_void_p(int(p)) for p in ptrs])

    def submit_group(self, slot, a_rgb, a_clusters, a_labels, n, H, W, K, params):
        """Enqueue one group of n device-resident frames on `slot` and return immediately (pointer arrays from
        pointer_array(); the cluster blocks they point to are updated by wait_group)."""
        _check(load_library().fslic_hip_submit_group(self._h, int(slot), C.byref(params), H, W, K, n,
                                                     C.cast(a_rgb, C.c_void_p), C.cast(a_clusters, C.c_void_p),
                                                     C.cast(a_labels, C.c_void_p)))

    def wait_group(self, slot):
        _check(load_library().fslic_hip_wait_group(self._h, int(slot)))

    def pipeline_submit(self, a_rgb, a_clusters, a_labels, n, H, W, K, params):
        """Hand one group of n device-resident frames to whichever slot is free (blocks only while all are occupied)."""
        _check(load_library().fslic_hip_pipeline_submit(self._h, C.byref(params), H, W, K, n,
                                                        C.cast(a_rgb, C.c_void_p), C.cast(a_clusters, C.c_void_p),
                                                        C.cast(a_labels, C.c_void_p)))

    def pipeline_batching(self, max_frames_per_group):
        """Let a slot thread serve several waiting submissions of identical geometry / options as one group of up to
        `max_frames_per_group` (<= 16) frames; 0 switches it off (the default).  Call before the first pipeline_submit."""
        _check(load_library().fslic_hip_pipeline_batching(self._h, int(max_frames_per_group)))

    def pipeline_drain(self):
        """Wait for every submitted group; dict of the totals since the previous drain."""
        ms, g, f, h = C.c_double(), C.c_longlong(), C.c_longlong(), C.c_longlong()
        _check(load_library().fslic_hip_pipeline_drain(self._h, C.byref(ms), C.byref(g), C.byref(f), C.byref(h)))
        return {"device_ms": ms.value, "groups": g.value, "frames": f.value, "host_topk_frames": h.value}

    def last_host_topk_frames(self, slot=0):
        return int(load_library().fslic_hip_last_host_topk_frames(self._h, int(slot)))

    def separate_pass_redos(self):
        """Frames (all slots, since the engine was created) redone with the separate cluster pass because of a stale pixel."""
        return sum(int(load_library().fslic_hip_separate_pass_redos(self._h, s)) for s in range(self.n_slots))

    def uncovered_redos(self, slot=None):
        """Frames (one slot, or all of them; since the engine was created) redone with storing assign passes because a visited pixel
        lay outside every cluster window while the group's subsampled passes ran label-free (include/fslic_hip.h)."""
        lib = load_library()
        if not hasattr(lib, "fslic_hip_uncovered_redos"):      # (FSLIC_LIB: a build without label-free passes never redoes for this reason)
            return 0
        slots = range(self.n_slots) if slot is None else [int(slot)]
        return sum(int(lib.fslic_hip_uncovered_redos(self._h, s)) for s in slots)

    def overlapped_groups(self):
        """Groups of the submit / drain pipeline (since the engine was created) that a slot thread began while the slot's previous group
        had not been collected yet (include/fslic_hip.h)."""
        lib = load_library()
        if not hasattr(lib, "fslic_hip_overlapped_groups"):      # (FSLIC_LIB: a build with the serial loop only)
            return 0
        return int(lib.fslic_hip_overlapped_groups(self._h))

    def pipeline_overlap(self, on):
        """False: the slot threads finish every group before they begin the next one (the serial loop); True is the default."""
        _check(load_library().fslic_hip_pipeline_overlap(self._h, int(bool(on))))

    def copy_bandwidth(self, nbytes=1 << 30, reps=5):
        """Measured HBM rate of this GPU in GB/s: bytes read + written per second of a plain streaming copy of `nbytes`."""
        v = C.c_double()
        _check(load_library().fslic_hip_copy_bandwidth(self._h, C.c_size_t(int(nbytes)), int(reps), C.byref(v)))
        return v.value

    def group_done(self, slot):
        """True when wait_group(slot) would not block."""
        return load_library().fslic_hip_group_done(self._h, int(slot)) != 0

    def last_launch_mode(self, slot=0):
        """0 direct enqueue, 1 recorded as a hipGraph during the call, 2 graph replay."""
        return int(load_library().fslic_hip_last_launch_mode(self._h, int(slot)))

    def last_prelabels(self, H, W, slot=0):
        out = np.empty((H, W), np.uint16)
        _check(load_library().fslic_hip_last_prelabels(self._h, int(slot), out.ctypes.data))
        return out

    def debug_lsc_state(self, K, z=0, slot=0):
        """Debug entry (tests): frame z's LSC state of the last group on `slot` -- the ten feature means (float32[10]) and the K
        feature-space centroids (float32[K, 10]; NaN rows: clusters without a member in the last update)."""
        means, cfeat = np.empty(10, np.float32), np.empty((int(K), 10), np.float32)
        _check(load_library().fslic_hip_debug_lsc_state(self._h, int(slot), int(z), int(K), means.ctypes.data, cfeat.ctypes.data))
        return means, cfeat

    def last_timing_report(self):
        return load_library().fslic_hip_last_timing_report(self._h).decode("utf-8")

    def last_recorder_report(self):
        """The calling thread's last iterate() / iterate_device() recorder report as bytes (src/recorder.h's JSON): every snapshot
        with params.debug_mode set, the header alone otherwise."""
        p, n = C.c_char_p(), C.c_size_t()
        _check(load_library().fslic_hip_last_recorder_report(self._h, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value) if n.value else b""

    def last_device_times(self, slot=0):
        t, f = C.c_float(), C.c_float()
        _check(load_library().fslic_hip_last_device_times(self._h, int(slot), C.byref(t), C.byref(f)))
        return t.value, f.value

    def set_launch_timing(self, on):
        _check(load_library().fslic_hip_set_launch_timing(self._h, int(bool(on))))

    def last_assign_loop(self, slot=0):
        """(sum of the fused assign launches' durations in ms, pixels they visited, number of launches)."""
        ms, px, n = C.c_float(), C.c_double(), C.c_int()
        _check(load_library().fslic_hip_last_assign_loop(self._h, int(slot), C.byref(ms), C.byref(px), C.byref(n)))
        return ms.value, px.value, n.value

    def last_group_frames(self, slot=0):
        return load_library().fslic_hip_last_group_frames(self._h, int(slot))

    def last_path(self, slot=0):
        return load_library().fslic_hip_last_path(self._h, int(slot))

    def lab_force_generic(self, on):
        """Testing aid (not in include/fslic_hip.h): the following Slic groups of this engine take the brute-force gather kernel."""
        _check(load_library().fslic_hip_lab_force_generic(self._h, int(bool(on))))


_default_engines = {}
_engine_lock = threading.Lock()


DEFAULT_ENGINE_SLOTS = 8      # concurrent iterate() calls (different SlicModels, different threads) per GPU before they queue


def default_engine(device=0):
    """The process-wide engine of a GPU, shared by every SlicModel on it.  Its entry points are thread-safe: a call takes
    one of the engine's slots for its duration (cfast_slic.pyx:188-193 runs iterate() without the GIL, and so does ctypes)."""
    with _engine_lock:
        e = _default_engines.get(device)
        if e is None:
            e = Engine(device, DEFAULT_ENGINE_SLOTS)
            _default_engines[device] = e
        return e


def device_count():
    return load_library().fslic_hip_device_count()


def is_supported_arch(arch_name):
    """cfast_slic.is_supported_arch (cfast_slic.pyx:354-357) for the one arch this package provides."""
    return arch_name == ARCH_NAME


def get_supported_archs():
    """cfast_slic.get_supported_archs (cfast_slic.pyx:359-369)."""
    return [ARCH_NAME]


def make_params(max_iter, compactness, min_size_factor, subsample_stride, convert_to_lab=True,
                manhattan_spatial_dist=True, preemptive=False, preemptive_thres=0.05, num_threads=-1,
                debug_mode=False, variant=0):
    p = Params()
    p.abi = PARAMS_ABI
    p.variant = int(variant)        # 0: Slic (Context), 1: LSC (ContextLSC)
    p.max_iter = int(max_iter)
    p.compactness = float(compactness)
    p.min_size_factor = float(min_size_factor)
    p.subsample_stride = int(subsample_stride)
    p.convert_to_lab = int(bool(convert_to_lab))
    p.manhattan_spatial_dist = int(bool(manhattan_spatial_dist))
    p.preemptive = int(bool(preemptive))
    p.preemptive_thres = float(preemptive_thres)
    p.num_threads = int(num_threads)
    p.debug_mode = int(bool(debug_mode))
    return p


PARAMS_ABI = 0x46533033         # FSLIC_PARAMS_ABI, include/fslic_hip.h
VARIANT_SLIC, VARIANT_LSC, VARIANT_REALDIST, VARIANT_REALDIST_L2, VARIANT_REALDIST_NOQ = 0, 1, 2, 3, 4     # fslic_params.variant
_REAL_DIST_VARIANTS = {"standard": VARIANT_REALDIST, "l2": VARIANT_REALDIST_L2, "noq": VARIANT_REALDIST_NOQ, "lsc": VARIANT_LSC}


class SlicModel(object):
    """Mirror of cfast_slic.SlicModel (cfast_slic.pyx:14-328) for arch "hip/gfx950"."""

    def __init__(self, num_components, arch_name=ARCH_NAME, real_dist=False, device=0):
        if isinstance(arch_name, bytes):
            arch_name = arch_name.decode("utf-8")
        if not is_supported_arch(arch_name):
            raise NotImplementedError("Unsupported arch " + repr(arch_name))      # pyx:21-22
        if num_components >= 65534:
            raise ValueError("num_components cannot exceed 65534")                # pyx:24-25
        elif num_components <= 0:
            raise ValueError("num_components should be a non-negative integer")   # pyx:26-27
        self.num_components = int(num_components)
        self.num_threads = -1
        self.arch_name = arch_name
        self.real_dist = real_dist
        self.real_dist_type = "standard"
        self.convert_to_lab = False
        self.float_color = True
        self.debug_mode = False
        self.initialized = False
        self.preemptive = False
        self.preemptive_thres = 0.05
        self.manhattan_spatial_dist = True
        self.last_timing_report = ""
        self.last_recorder_report = ""
        self.device = int(device)
        self._clusters = np.zeros(self.num_components, CLUSTER_DTYPE)              # pyx:38-39
        self._engine = default_engine(self.device)   # raises when no GPU / library: no CPU fallback

    def copy(self):
        # cfast_slic.pyx:45-49 drops arch_name; here the arch is preserved.
        result = SlicModel(self.num_components, self.arch_name, device=self.device)
        result.real_dist = self.real_dist
        result.real_dist_type = self.real_dist_type
        result._clusters[:] = self._clusters
        result.initialized = self.initialized
        return result

    @property
    def clusters(self):                                                            # pyx:51-66
        out = []
        for c in self._clusters:
            out.append(dict(
                number=int(c["number"]),
                yx=(float(c["y"]), float(c["x"])),
                color=(float(c["r"]), float(c["g"]), float(c["b"])),
                num_members=int(c["num_members"]),
            ))
        return out

    @clusters.setter
    def clusters(self, clusters):                                                  # pyx:68-98
        n = len(clusters)
        new = np.zeros(n, CLUSTER_DTYPE)
        for i, d in enumerate(clusters):
            y, x = d["yx"]
            r, g, b = d["color"]
            new[i]["number"] = i
            new[i]["y"] = np.uint16(y)
            new[i]["x"] = np.uint16(x)
            new[i]["r"] = np.uint8(r)
            new[i]["g"] = np.uint8(g)
            new[i]["b"] = np.uint8(b)
            new[i]["num_members"] = np.uint32(d["num_members"])
        self._clusters = new
        self.num_components = n
        self.initialized = True

    @property
    def cluster_array(self):
        """The raw Cluster[K] block (structured numpy view); not part of the reference surface."""
        return self._clusters

    def to_yxmrgb(self):                                                           # pyx:100-113
        c = self._clusters
        return np.stack([c["y"], c["x"], c["num_members"].astype(np.float64), c["r"], c["g"], c["b"]], 1).astype(np.float64)

    @staticmethod
    def _check_image(image):
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 3 or not image.flags["C_CONTIGUOUS"]:
            raise ValueError("image must be a C-contiguous uint8 array of shape [H, W, 3]")
        if image.shape[2] != 3:
            raise ValueError("nchan != 3")                                         # pyx:125-126
        return image

    def initialize(self, image):                                                   # pyx:124-147
        image = self._check_image(image)
        H, W, _ = image.shape
        _check(load_library().fslic_hip_initialize_clusters(H, W, self.num_components, image.ctypes.data,
                                                            self._clusters.ctypes.data))
        self.initialized = True

    @staticmethod
    def _check_assignments(assignments):
        a = np.asarray(assignments)
        if a.dtype != np.int16 or a.ndim != 2 or not a.flags["C_CONTIGUOUS"]:
            raise ValueError("assignments must be a C-contiguous int16 array of shape [H, W]")
        return a

    def get_connectivity(self, assignments):                                       # pyx:262-273
        a = self._check_assignments(assignments)
        H, W = a.shape
        num, nb = self._engine.get_connectivity(a.view(np.uint16), H, W, self.num_components)
        return NodeConnectivity(num, nb)

    def get_knn_connectivity(self, assignments, num_neighbors):                    # pyx:275-282
        a = self._check_assignments(assignments)
        H, W = a.shape
        num, nb = knn_connectivity(H, W, self._clusters, num_neighbors)
        return NodeConnectivity(num, nb)

    def get_mask_density(self, mask, assignments):                                 # pyx:284-304
        a = self._check_assignments(assignments)
        m = np.asarray(mask)
        if m.dtype != np.uint8 or m.ndim != 2 or not m.flags["C_CONTIGUOUS"]:
            raise ValueError("mask must be a C-contiguous uint8 array of shape [H, W]")
        H, W = a.shape
        if m.shape[0] != H or m.shape[1] != W:
            raise ValueError("The shape of mask does not match the one of assignments")          # pyx:290-291
        return self._engine.get_mask_density(self._clusters, a.view(np.uint16), m, H, W)

    def broadcast_density_to_mask(self, densities, assignments):                   # pyx:306-324
        a = self._check_assignments(assignments)
        d = np.asarray(densities)
        if d.dtype != np.uint8 or d.ndim != 1:
            raise ValueError("densities must be a uint8 array of shape [K]")
        if d.shape[0] != self.num_components:
            raise ValueError("The shape of densities should match the number of clusters")       # pyx:310-311
        H, W = a.shape
        return self._engine.cluster_density_to_mask(a.view(np.uint16), d, H, W)

    def iterate_params(self, max_iter, compactness, min_size_factor, subsample_stride):
        """The fslic_params of an iterate() call with this model's options and variant (iterate below; frames.slic_tensor)."""
        variant = VARIANT_SLIC
        if self.real_dist:                                                         # pyx:198-235
            if self.real_dist_type not in _REAL_DIST_VARIANTS:
                raise RuntimeError("No such real_dist_type " + repr(self.real_dist_type))      # pyx:236
            variant = _REAL_DIST_VARIANTS[self.real_dist_type]
        return make_params(max_iter, compactness, min_size_factor, subsample_stride, self.convert_to_lab,
                           self.manhattan_spatial_dist, self.preemptive, self.preemptive_thres,
                           self.num_threads, self.debug_mode, variant)

    def iterate(self, image, max_iter, compactness, min_size_factor, subsample_stride):   # pyx:150-260
        if not self.initialized:
            raise RuntimeError("Slic model is not initialized")                    # pyx:151-152
        image = self._check_image(image)
        p = self.iterate_params(max_iter, compactness, min_size_factor, subsample_stride)
        labels = self._engine.iterate(image, self._clusters, p)
        self.last_timing_report = self._engine.last_timing_report()
        self.last_recorder_report = self._engine.last_recorder_report()     # bytes, after every call (pyx:196, :256)
        # pyx:258-260 makes an int16 copy and turns 0xFFFF into -1; the int16 VIEW of the same bytes is that array (0xFFFF is -1
        # already), without three passes over the map (250 us at 1280x720, more than the device-side work)
        return labels.view(np.int16)


class NodeConnectivity(object):
    """cfast_slic.NodeConnectivity (cfast_slic.pyx:330-351): per-cluster neighbour lists."""

    def __init__(self, num_neighbors, neighbors):
        self.num_neighbors = num_neighbors
        self.neighbors = neighbors

    def tolist(self):                                                              # pyx:337-347
        return [[int(v) for v in self.neighbors[k, :self.num_neighbors[k]]] for k in range(self.num_neighbors.shape[0])]


def knn_connectivity(H, W, clusters, num_neighbors):
    """fast_slic_knn_connectivity (src/fast-slic.cpp:80-130): host only, no engine needed."""
    cl = np.ascontiguousarray(clusters)
    K = cl.shape[0]
    n = int(num_neighbors)
    if n < 0:
        raise OverflowError("num_neighbors must be non-negative")
    num = np.zeros(K, np.int32)
    nb = np.zeros((K, max(n, 1)), np.uint32)
    _check(load_library().fslic_hip_knn_connectivity(int(H), int(W), K, cl.ctypes.data, n, num.ctypes.data, nb.ctypes.data))
    return num, nb[:, :n]


def enforce_connectivity(assignments, min_threshold, device=0):
    """cfast_slic.enforce_connectivity (cfast_slic.pyx:371-396): in place on an int16 [H, W] array."""
    a = np.asarray(assignments)
    if a.dtype != np.int16 or a.ndim != 2 or not a.flags["C_CONTIGUOUS"]:
        raise ValueError("assignments must be a C-contiguous int16 array of shape [H, W]")
    u = a.view(np.uint16)
    valid = u[u != 0xFFFF]
    K = (int(valid.max()) if valid.size else 0) + 1
    out = default_engine(device).enforce_connectivity(u, K, min_threshold)
    u[...] = out
    return assignments
