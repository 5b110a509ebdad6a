"""SimpleCRF's mean-field inference on torch tensors in HBM (csrc/crf_tensor.hip): the step between superpixel_pool /
superpixel_graph and superpixel_unpool, without a trip through the host.

    q = superpixel_crf(unaries, graph, yxrgb, members, max_iter=10, params=None, compat=None, temporal=False, q0=None)

`unaries` is a float32 tensor [C, K] or [N, C, K] on a ROCm GPU: energies, what SimpleCRFFrame.unaries holds.  A caller with
probabilities passes `-torch.log(p)`; that is torch's log, not the host logf of SimpleCRFFrame.set_proba, so the two can differ in
the last bit.  `graph` is a SuperpixelGraph (fast_slic_amd.rag) or a pair (offsets int64 [N * K + 1], indices int32 [nnz]): one CSR
over (frame, node) whose indices are node numbers inside the frame.  `yxrgb` ([5, K] / [N, 5, K] float32) holds the Cluster's y, x,
r, g, b channel-first, as superpixel_pool returns means; `members` ([K] / [N, K] int32) the Cluster's num_members, which is what
pool's counts are.  The result is a new float32 tensor of the unaries' shape, bit-equal to what SimpleCRF.inference computes on the
same inputs.  The work runs on torch's current stream of the unaries' device without host synchronisation; scratch memory comes from
torch's caching allocator.  SimpleCRF (fast_slic_amd.crf) remains the reference-shaped surface.  This module imports torch; the
package itself does not import it.
"""
import ctypes as C
import numbers

import torch

from . import _binding as B
from .crf import _PARAMS, _Params
from .pool import _check_device, _check_float_map, _stream
from .rag import SuperpixelGraph

__all__ = ["superpixel_crf", "DEFAULT_PARAMS"]

# a fresh SimpleCRF's (src/simple-crf.hpp:81-87); its compat is 1.0 for every class
DEFAULT_PARAMS = dict(spatial_w=10.0, temporal_w=10.0, spatial_srgb=13.0, temporal_srgb=13.0, spatial_sxy=80.0, spatial_smooth_w=0.0,
                      spatial_smooth_sxy=3.0)
_LIMIT = 1 << 31


def _lib():
    lib = B.load_library()
    if not hasattr(lib, "fslic_hip_crf_tensor_inference"):
        raise RuntimeError("fast_slic_amd: the loaded library has no CRF tensor entry points; rebuild it")
    return lib


# ---- argument checks: all of them run before any device work ----
def _check_tensor(t, dtype, shape, what, shape_text):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a torch tensor" % what)
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (what, str(dtype).replace("torch.", ""), t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s (%s) to match the unaries, got %s" % (what, tuple(shape), shape_text, tuple(t.shape)))


def _check_graph(graph, N, K):
    """-> the number of neighbour entries, known without looking at device memory."""
    if isinstance(graph, SuperpixelGraph):
        if graph.num_components != K or graph.num_frames != N:
            raise ValueError("graph has %d frames of %d nodes, the unaries have %d of %d"
                             % (graph.num_frames, graph.num_components, N, K))
        return 2 * int(graph.edge_index.shape[1])
    if not isinstance(graph, (tuple, list)) or len(graph) != 2:
        raise ValueError("graph must be a SuperpixelGraph or a pair (offsets, indices)")
    offsets, indices = graph
    if not isinstance(offsets, torch.Tensor) or not isinstance(indices, torch.Tensor):
        raise ValueError("graph offsets and indices must be torch tensors")
    if offsets.dtype != torch.int64:
        raise ValueError("graph offsets must be int64, got %s" % offsets.dtype)
    if indices.dtype != torch.int32:
        raise ValueError("graph indices must be int32, got %s" % indices.dtype)
    if offsets.dim() != 1 or offsets.shape[0] != N * K + 1:
        raise ValueError("graph offsets must have shape (%d,) (N * K + 1), got %s" % (N * K + 1, tuple(offsets.shape)))
    if indices.dim() != 1:
        raise ValueError("graph indices must be one-dimensional, got shape %s" % (tuple(indices.shape),))
    return int(indices.shape[0])


def _check_params(params):
    values = dict(DEFAULT_PARAMS)
    if params is not None:
        if not isinstance(params, dict):
            raise ValueError("params must be None or a dict over %s" % (_PARAMS,))
        for name, v in params.items():
            if name not in DEFAULT_PARAMS:
                raise ValueError("unknown params name %r; the names are %s" % (name, _PARAMS))
            if isinstance(v, bool) or not isinstance(v, numbers.Real):
                raise ValueError("params[%r] must be a real number" % name)
            values[name] = float(v)
    p = _Params()
    for name in _PARAMS:
        setattr(p, name, values[name])
    return p


def _check_compat(compat, Cn):
    """-> None (every class 1.0), the tensor, or a list of C floats."""
    if compat is None:
        return None
    if isinstance(compat, torch.Tensor):
        _check_tensor(compat, torch.float32, (Cn,), "compat", "[C]")
        return compat
    try:
        values = list(compat)
    except TypeError:
        raise ValueError("compat must be None, a sequence of C floats or a float32 [C] tensor")
    if len(values) != Cn:
        raise ValueError("compat must hold one value per class (%d), got %d" % (Cn, len(values)))
    if any(isinstance(v, bool) or not isinstance(v, numbers.Real) for v in values):
        raise ValueError("compat must hold real numbers")
    return [float(v) for v in values]


def superpixel_crf(unaries, graph, yxrgb, members, max_iter=10, params=None, compat=None, temporal=False, q0=None):
    """`max_iter` mean-field sweeps of SimpleCRF over `unaries` ([C, K] or [N, C, K] float32 energies on a ROCm GPU) -> q, a new
    tensor of the same shape.

    graph: a SuperpixelGraph, or (offsets int64 [N * K + 1], indices int32 [nnz]).  Rows may be empty, of any length, asymmetric, and
    hold duplicates and self-loops; an index outside [0, K) contributes nothing; row bounds are clamped into [0, nnz] and to
    non-decreasing on the device (nothing is validated on the host: that would synchronise).
    yxrgb [5, K] / [N, 5, K] float32, members [K] / [N, K] int32: the clusters.
    params: None or a dict over spatial_w, temporal_w, spatial_srgb, temporal_srgb, spatial_sxy, spatial_smooth_w,
    spatial_smooth_sxy (a fresh SimpleCRF's values for the names left out).  compat: None (1.0 per class), C floats, or a float32
    [C] tensor on the same GPU.
    temporal=False: the N frames are independent.  temporal=True: they are consecutive times of one window, node i of frame n
    linked to node i of n - 1 and n + 1, exactly as in SimpleCRF.
    q0: the starting q, float32 of the unaries' shape (never written); None: crf_expf(-unaries), which is SimpleCRF.initialize().
    max_iter=0 returns the starting q."""
    _check_float_map(unaries, (2, 3), "unaries", "[C, K] or [N, C, K]")
    batched = unaries.dim() == 3
    N = unaries.shape[0] if batched else 1
    Cn, K = (int(v) for v in unaries.shape[-2:])
    lead = (N,) if batched else ()
    _check_tensor(yxrgb, torch.float32, lead + (5, K), "yxrgb", "[5, K] or [N, 5, K]")
    _check_tensor(members, torch.int32, lead + (K,), "members", "[K] or [N, K]")
    if q0 is not None:
        _check_tensor(q0, torch.float32, tuple(unaries.shape), "q0", "the unaries' shape")
    nnz = _check_graph(graph, N, K)
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or max_iter < 0:
        raise ValueError("max_iter must be a non-negative integer, got %r" % (max_iter,))
    max_iter = int(max_iter)
    if max_iter >= _LIMIT:
        raise ValueError("max_iter must be below 2^31")
    p = _check_params(params)
    compat = _check_compat(compat, Cn)
    if not isinstance(temporal, bool):
        raise ValueError("temporal must be True or False, got %r" % (temporal,))
    if N * Cn * K >= _LIMIT or N * K + 1 >= _LIMIT or nnz >= _LIMIT:
        raise ValueError("N * C * K, N * K + 1 and the number of neighbour entries must be below 2^31")
    _check_device(unaries, "unaries")
    dev = unaries.device
    on_graph = (("graph.edge_index", graph.edge_index), ("graph.offsets", graph.offsets)) if isinstance(graph, SuperpixelGraph) \
        else (("graph offsets", graph[0]), ("graph indices", graph[1]))
    for what, t in (("yxrgb", yxrgb), ("members", members), ("q0", q0), ("compat", compat)) + on_graph:
        if isinstance(t, torch.Tensor):
            _check_device(t, what)
            if t.device != dev:
                raise ValueError("%s must be on the unaries' GPU %s, got %s" % (what, dev, t.device))

    lib = _lib()
    with torch.cuda.device(dev):
        if isinstance(graph, SuperpixelGraph):
            offsets, indices = graph.to_batch_csr()
        else:
            offsets, indices = graph[0].contiguous(), graph[1].contiguous()
        if compat is None:
            compat = torch.ones(Cn, dtype=torch.float32, device=dev)
        elif isinstance(compat, list):       # through pinned memory: an asynchronous copy, no host synchronisation
            compat = torch.tensor(compat, dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
        un, yx, mem, comp = unaries.contiguous(), yxrgb.contiguous(), members.contiguous(), compat.contiguous()
        start = q0.contiguous() if q0 is not None else None
        nbytes = C.c_size_t()
        B._check(lib.fslic_hip_crf_tensor_workspace_size(N, Cn, K, nnz, C.byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        q = torch.empty(tuple(unaries.shape), dtype=torch.float32, device=dev)
        B._check(lib.fslic_hip_crf_tensor_inference(dev.index, _stream(dev), N, Cn, K, int(temporal), max_iter, C.byref(p), comp.data_ptr(),
                                                    yx.data_ptr(), mem.data_ptr(), offsets.data_ptr(), indices.data_ptr() if nnz else None,
                                                    nnz, un.data_ptr(), start.data_ptr() if start is not None else None, q.data_ptr(),
                                                    ws.data_ptr(), nbytes.value))
    return q
