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

The call is differentiable (csrc/crf_tensor_grad.hip): when gradients are enabled and `unaries`, `q0` or a tensor `compat` requires
one, the same sweeps run with every iterate kept ((max_iter + 1) * 4 * N * C * K bytes), the result has the same bits, and backward()
gives deterministic gradients for those three.  Nothing flows to `yxrgb`, `members`, the graph or `params`: learning the kernel
weights is out of scope.
"""
import ctypes as C
import numbers

import torch
from torch.autograd.function import once_differentiable

from . import _binding as B
from .crf import _PARAMS, _Params
from .pool import _check_device, _check_float_map, _stream
from .rag import SuperpixelGraph

__all__ = ["superpixel_crf", "transpose_batch_csr", "DEFAULT_PARAMS"]

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


# ---- the differentiable path ----
def transpose_batch_csr(offsets, indices, N, K):
    """The transposed lists of one CSR over (frame, node) -> (t_offsets int64 [N * K + 1], t_entries int32 [nnz], t_rows int32 [nnz]):
    the neighbour entries whose target is node j of frame n are t_entries[t_offsets[n * K + j]:t_offsets[n * K + j + 1]], in ascending
    entry order, and t_rows names the row over (frame, node) of each.  An entry whose index is outside [0, K), or that lies behind the
    last row, is sorted behind every target and belongs to none.  Plain torch without a host synchronisation, on any device; nothing
    is validated (the backward kernels check every entry against the row bounds they clamp themselves)."""
    n, nnz = N * K, indices.shape[0]
    dev = indices.device
    # the row of entry k: how many rows end at or before k (n: behind the last row)
    row = torch.searchsorted(offsets[1:].contiguous(), torch.arange(nnz, dtype=torch.int64, device=dev), right=True)
    j = indices.to(torch.int64)
    key = (torch.div(row, K, rounding_mode="floor") * K + j).masked_fill((j < 0) | (j >= K) | (row >= n), n)
    key, entry = torch.sort(key, stable=True)              # stable: ascending entry order inside one target
    t_offsets = torch.searchsorted(key, torch.arange(n + 1, dtype=torch.int64, device=dev))
    return t_offsets, entry.to(torch.int32), row[entry].to(torch.int32)


def _workspace(lib, dev, N, Cn, K, nnz, backward, with_compat):
    nbytes = C.c_size_t()
    B._check(lib.fslic_hip_crf_tensor_grad_workspace_size(N, Cn, K, nnz, int(backward), int(with_compat), C.byref(nbytes)))
    return torch.empty(nbytes.value, dtype=torch.uint8, device=dev), nbytes.value


class _SuperpixelCRF(torch.autograd.Function):
    """The sweeps with every iterate kept, and their adjoint.  Tensors are contiguous and on one GPU; `start` is q0 or None."""

    @staticmethod
    def forward(ctx, un, start, comp, yx, mem, offsets, indices, N, max_iter, temporal, p):
        lib, dev = _lib(), un.device
        if not hasattr(lib, "fslic_hip_crf_tensor_backward"):
            raise RuntimeError("fast_slic_amd: the loaded library has no CRF tensor backward; rebuild it")
        Cn, K = (int(v) for v in un.shape[-2:])
        nnz = int(indices.shape[0])
        with torch.cuda.device(dev):
            ws, nbytes = _workspace(lib, dev, N, Cn, K, nnz, False, False)
            q_all = torch.empty((max_iter + 1,) + tuple(un.shape), dtype=torch.float32, device=dev)
            B._check(lib.fslic_hip_crf_tensor_inference_saved(dev.index, _stream(dev), N, Cn, K, int(temporal), max_iter, C.byref(p),
                                                              comp.data_ptr(), yx.data_ptr(), mem.data_ptr(), offsets.data_ptr(),
                                                              indices.data_ptr() if nnz else None, nnz, un.data_ptr(),
                                                              start.data_ptr() if start is not None else None, q_all.data_ptr(),
                                                              ws.data_ptr(), nbytes))
        ctx.save_for_backward(un, comp, yx, mem, offsets, indices, q_all)
        ctx.call = (N, max_iter, temporal, p, start is not None)
        return q_all[max_iter]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        un, comp, yx, mem, offsets, indices, q_all = ctx.saved_tensors
        N, max_iter, temporal, p, has_q0 = ctx.call
        lib, dev = _lib(), un.device
        Cn, K = (int(v) for v in un.shape[-2:])
        nnz = int(indices.shape[0])
        with torch.cuda.device(dev):
            g = g.contiguous()
            t_offsets, t_entries, t_rows = transpose_batch_csr(offsets, indices, N, K)
            du = torch.empty_like(un)
            dq0 = torch.empty_like(un) if has_q0 else None
            dcompat = torch.empty_like(comp) if ctx.needs_input_grad[2] else None
            ws, nbytes = _workspace(lib, dev, N, Cn, K, nnz, True, dcompat is not None)
            B._check(lib.fslic_hip_crf_tensor_backward(dev.index, _stream(dev), N, Cn, K, int(temporal), max_iter, C.byref(p),
                                                       comp.data_ptr(), yx.data_ptr(), mem.data_ptr(), offsets.data_ptr(),
                                                       indices.data_ptr() if nnz else None, nnz, t_offsets.data_ptr(),
                                                       t_entries.data_ptr() if nnz else None, t_rows.data_ptr() if nnz else None,
                                                       un.data_ptr(), q_all.data_ptr(), g.data_ptr(), du.data_ptr(),
                                                       dq0.data_ptr() if has_q0 else None,
                                                       dcompat.data_ptr() if dcompat is not None else None, ws.data_ptr(), nbytes))
        return du, dq0, dcompat, None, None, None, None, None, None, None, None


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
    max_iter=0 returns the starting q.

    Differentiable with respect to `unaries`, `q0` and a tensor `compat`: when gradients are enabled and one of them requires one,
    q is part of the autograd graph (the same bits; every iterate is kept for the backward, (max_iter + 1) * 4 * N * C * K bytes) and
    its backward is deterministic and once differentiable; q is then a view of the kept iterates, which autograd protects from
    in-place changes.  `yxrgb`, `members`, the graph and `params` get no gradient: learning the
    kernel weights (gradients with respect to params or the edge energies) is out of scope.  Otherwise q has no grad_fn."""
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
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (unaries, q0, compat)):
            return _SuperpixelCRF.apply(un, start, comp, yx.detach(), mem, offsets, indices, N, max_iter, temporal, p)
        nbytes = C.c_size_t()
        B._check(lib.fslic_hip_crf_tensor_workspace_size(N, Cn, K, nnz, C.byref(nbytes)))
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        q = torch.empty(tuple(unaries.shape), dtype=torch.float32, device=dev)
        B._check(lib.fslic_hip_crf_tensor_inference(dev.index, _stream(dev), N, Cn, K, int(temporal), max_iter, C.byref(p), comp.data_ptr(),
                                                    yx.data_ptr(), mem.data_ptr(), offsets.data_ptr(), indices.data_ptr() if nnz else None,
                                                    nnz, un.data_ptr(), start.data_ptr() if start is not None else None, q.data_ptr(),
                                                    ws.data_ptr(), nbytes.value))
    return q
