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
gives deterministic gradients for those three.

The edge energies can be learnt.  `params` may be a float32 [7] tensor on the GPU in PARAM_NAMES order (an nn.Parameter): backward()
then fills its gradient.  crf_edge_energies(graph, yxrgb, members, params, temporal) returns the energies themselves, one per
neighbour entry and two per node, and `energies=(edge, links)` runs the sweeps on energies a caller (a network) provides; the result
is differentiable with respect to both.  A tensor `params` is the composition of the two.  Nothing flows to `yxrgb`, `members` or the
graph.
"""
import ctypes as C
import numbers

import torch
from torch.autograd.function import once_differentiable

from . import _binding as B, _tensors as T
from .crf import _PARAMS, _Params
from .rag import SuperpixelGraph

__all__ = ["superpixel_crf", "crf_edge_energies", "transpose_batch_csr", "DEFAULT_PARAMS", "PARAM_NAMES"]

PARAM_NAMES = _PARAMS                 # the order of fslic_crf_params and of a params tensor

# a fresh SimpleCRF's (src/simple-crf.hpp:81-87); its compat is 1.0 for every class
DEFAULT_PARAMS = dict(spatial_w=10.0, temporal_w=10.0, spatial_srgb=13.0, temporal_srgb=13.0, spatial_sxy=80.0, spatial_smooth_w=0.0,
                      spatial_smooth_sxy=3.0)
_LIMIT = 1 << 31


def _library(entry="fslic_hip_crf_tensor_inference", what="entry points"):
    return T.library(entry, "CRF tensor " + what)


def _energies_library():
    _library()
    return _library("fslic_hip_crf_tensor_backward_energies", "energies entry points")


# ---- argument checks: all of them run before any device work ----
def _check_tensor(t, dtype, shape, what, shape_text):
    T.check_tensor(t, what, (dtype,), shape_text, lambda s: True)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s (%s) to match the unaries, got %s" % (what, tuple(shape), shape_text, tuple(t.shape)))


def _check_neighbours(graph, N, K):
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


def _check_params_tensor(params):
    if params.dtype != torch.float32:
        raise ValueError("a params tensor must be float32, got %s" % params.dtype)
    if tuple(params.shape) != (len(_PARAMS),):
        raise ValueError("a params tensor must have shape (%d,) in the order %s, got %s" % (len(_PARAMS), _PARAMS, tuple(params.shape)))


def _check_energies(energies, nnz, lead, K, temporal):
    """-> (edge, links or None)."""
    if not isinstance(energies, (tuple, list)) or len(energies) != 2:
        raise ValueError("energies must be a pair (edge, links)")
    edge, links = energies
    if not isinstance(edge, torch.Tensor):
        raise ValueError("energies: edge must be a torch tensor")
    if edge.dtype != torch.float32:
        raise ValueError("energies: edge must be float32, got %s" % edge.dtype)
    if tuple(edge.shape) != (nnz,):
        raise ValueError("energies: edge must have shape (%d,) (one value per neighbour entry), got %s" % (nnz, tuple(edge.shape)))
    if links is None:
        if temporal:
            raise ValueError("energies: links must be given with temporal=True")
        return edge, None
    _check_tensor(links, torch.float32, lead + (2, K), "energies: links", "[2, K] or [N, 2, K]")
    return edge, links


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


class _Call(object):
    """What every sweep entry of the library is given, from contiguous tensors on one GPU."""

    def __init__(self, un, comp, mem, offsets, indices, N, max_iter, temporal):
        self.un, self.comp, self.mem, self.offsets, self.indices = un, comp, mem, offsets, indices
        self.N, self.max_iter, self.temporal = N, max_iter, temporal
        self.dev = un.device
        self.Cn, self.K = (int(v) for v in un.shape[-2:])
        self.nnz = int(indices.shape[0])

    def _head(self):
        return (self.dev.index, T.stream(self.dev), self.N, self.Cn, self.K, int(self.temporal), self.max_iter)

    def _graph(self):
        return (T.ptr(self.mem), T.ptr(self.offsets), T.ptr(self.indices, self.nnz), self.nnz)

    def from_params(self, p, yx):
        """The arguments up to nnz of an entry that computes the energies from host params and yxrgb."""
        return self._head() + (C.byref(p), T.ptr(self.comp), T.ptr(yx)) + self._graph()

    def from_energies(self, edge, links):
        """The arguments up to links of an _energies entry."""
        return self._head() + (T.ptr(self.comp),) + self._graph() + (T.ptr(edge, self.nnz), T.ptr(links))

    def run(self, entry, lead, own, size_entry, *flags):
        """entry(*lead, *own, workspace, bytes) with as much workspace as size_entry(N, C, K, nnz, *flags) asks for."""
        ws, nbytes = T.scratch(self.dev, size_entry, self.N, self.Cn, self.K, self.nnz, *flags)
        B._check(entry(*lead, *own, ws.data_ptr(), nbytes))


def _plain(lib, entry, call, lead, start):
    """The call outside autograd -> q."""
    q = torch.empty_like(call.un)
    call.run(entry, lead, (T.ptr(call.un), T.ptr(start), T.ptr(q)), lib.fslic_hip_crf_tensor_workspace_size)
    return q


def _saved_forward(ctx, lib, entry, call, lead, start, kept):
    """The sweeps with every iterate kept -> q, a view of them.  `kept`: the energy source's tensors, saved behind the call's."""
    with torch.cuda.device(call.dev):
        q_all = torch.empty((call.max_iter + 1,) + tuple(call.un.shape), dtype=torch.float32, device=call.dev)
        call.run(entry, lead, (T.ptr(call.un), T.ptr(start), T.ptr(q_all)), lib.fslic_hip_crf_tensor_grad_workspace_size, 0, 0)
    ctx.save_for_backward(call.un, call.comp, call.mem, call.offsets, call.indices, q_all, *kept)
    ctx.call = (call.N, call.max_iter, call.temporal, start is not None)
    return q_all[call.max_iter]


def _saved_call(ctx):
    """What _saved_forward kept -> (the call, q_all, whether q0 was given, the energy source's tensors)."""
    N, max_iter, temporal, has_q0 = ctx.call
    return _Call(*ctx.saved_tensors[:5], N, max_iter, temporal), ctx.saved_tensors[5], has_q0, ctx.saved_tensors[6:]


def _saved_backward(lib, entry, call, lead, q_all, has_q0, with_compat, g, energy_grads=()):
    """The adjoint of _saved_forward -> (du, dq0, dcompat).  `energy_grads`: the pointers that follow dcompat's in the entry."""
    un, nnz = call.un, call.nnz
    with torch.cuda.device(call.dev):
        g = g.contiguous()
        t_offsets, t_entries, t_rows = transpose_batch_csr(call.offsets, call.indices, call.N, call.K)
        du = torch.empty_like(un)
        dq0 = torch.empty_like(un) if has_q0 else None
        dcompat = torch.empty_like(call.comp) if with_compat else None
        own = (T.ptr(t_offsets), T.ptr(t_entries, nnz), T.ptr(t_rows, nnz), T.ptr(un), T.ptr(q_all), T.ptr(g), T.ptr(du), T.ptr(dq0),
               T.ptr(dcompat)) + tuple(energy_grads)
        call.run(entry, lead, own, lib.fslic_hip_crf_tensor_grad_workspace_size, 1, int(with_compat))
    return du, dq0, dcompat


class _SuperpixelCRF(torch.autograd.Function):
    """The sweeps with every iterate kept, and their adjoint.  Tensors are contiguous and on one GPU; `start` is q0 or None."""

    @staticmethod
    def forward(ctx, un, start, comp, yx, mem, offsets, indices, N, max_iter, temporal, p):
        lib = _library("fslic_hip_crf_tensor_backward", "backward")
        call = _Call(un, comp, mem, offsets, indices, N, max_iter, temporal)
        ctx.p = p
        return _saved_forward(ctx, lib, lib.fslic_hip_crf_tensor_inference_saved, call, call.from_params(p, yx), start, (yx,))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lib = _library()
        call, q_all, has_q0, (yx,) = _saved_call(ctx)
        return _saved_backward(lib, lib.fslic_hip_crf_tensor_backward, call, call.from_params(ctx.p, yx), q_all, has_q0,
                               ctx.needs_input_grad[2], g) + (None,) * 8


class _SuperpixelCRFEnergies(torch.autograd.Function):
    """_SuperpixelCRF with the energies given: `edge` [nnz] and `links` [N, 2, K] or None get gradients too."""

    @staticmethod
    def forward(ctx, un, start, comp, edge, links, mem, offsets, indices, N, max_iter, temporal):
        lib = _energies_library()
        call = _Call(un, comp, mem, offsets, indices, N, max_iter, temporal)
        return _saved_forward(ctx, lib, lib.fslic_hip_crf_tensor_inference_saved_energies, call, call.from_energies(edge, links), start,
                              (edge,) if links is None else (edge, links))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lib = _energies_library()
        call, q_all, has_q0, kept = _saved_call(ctx)
        edge, links = (kept + (None,))[:2]
        dedge = torch.empty_like(edge) if ctx.needs_input_grad[3] else None
        dlinks = torch.empty_like(links) if links is not None and ctx.needs_input_grad[4] else None
        grads = _saved_backward(lib, lib.fslic_hip_crf_tensor_backward_energies, call, call.from_energies(edge, links), q_all, has_q0,
                                ctx.needs_input_grad[2], g, (T.ptr(dedge, call.nnz), T.ptr(dlinks)))
        return grads + (dedge, dlinks) + (None,) * 6


def _energies_raw(theta, yx, mem, offsets, indices, N, K, temporal):
    """edge [nnz] and links [N, 2, K] from contiguous tensors on one GPU."""
    lib, dev = _energies_library(), yx.device
    nnz = int(indices.shape[0])
    with torch.cuda.device(dev):
        edge = torch.empty(nnz, dtype=torch.float32, device=dev)
        links = torch.empty((N, 2, K), dtype=torch.float32, device=dev)
        B._check(lib.fslic_hip_crf_tensor_energies(dev.index, T.stream(dev), N, K, int(temporal), T.ptr(theta), T.ptr(yx), T.ptr(mem),
                                                   T.ptr(offsets), T.ptr(indices, nnz), nnz, T.ptr(edge, nnz), T.ptr(links)))
    return edge, links


class _EdgeEnergies(torch.autograd.Function):
    """The energies from a params tensor, and their backward to it."""

    @staticmethod
    def forward(ctx, theta, yx, mem, offsets, indices, N, K, temporal):
        edge, links = _energies_raw(theta, yx, mem, offsets, indices, N, K, temporal)
        ctx.save_for_backward(theta, yx, offsets, indices)
        ctx.call = (N, K, temporal)
        return edge, links

    @staticmethod
    @once_differentiable
    def backward(ctx, g_edge, g_links):
        theta, yx, offsets, indices = ctx.saved_tensors
        N, K, temporal = ctx.call
        lib, dev = _energies_library(), yx.device
        nnz = int(indices.shape[0])
        with torch.cuda.device(dev):
            g_edge = g_edge.contiguous() if g_edge is not None and nnz else None
            g_links = g_links.contiguous() if g_links is not None else None
            ws, nbytes = T.scratch(dev, lib.fslic_hip_crf_tensor_energies_backward_workspace_size, N, K)
            dtheta = torch.empty_like(theta)
            B._check(lib.fslic_hip_crf_tensor_energies_backward(
                dev.index, T.stream(dev), N, K, int(temporal), T.ptr(theta), T.ptr(yx), T.ptr(offsets), T.ptr(indices, nnz), nnz, T.ptr(g_edge),
                T.ptr(g_links), T.ptr(dtheta), ws.data_ptr(), nbytes))
        return dtheta, None, None, None, None, None, None, None


def _params_on(params, dev):
    """A dict or None -> the seven float32 values on `dev`, through pinned memory (no host synchronisation)."""
    p = _check_params(params)
    return torch.tensor([getattr(p, n) for n in _PARAMS], dtype=torch.float32).pin_memory().to(dev, non_blocking=True)


def _energies(theta, yx, mem, offsets, indices, N, K, temporal):
    if torch.is_grad_enabled() and theta.requires_grad:
        return _EdgeEnergies.apply(theta.contiguous(), yx.detach(), mem, offsets, indices, N, K, temporal)
    return _energies_raw(theta.detach().contiguous(), yx.detach(), mem, offsets, indices, N, K, temporal)


def _batch_csr(graph):
    if isinstance(graph, SuperpixelGraph):
        return graph.to_batch_csr()
    return graph[0].contiguous(), graph[1].contiguous()


def _check_same_device(dev, owner, graph, named):
    """Every tensor of `named` and of the graph is on the GPU `dev`, which is `owner`'s."""
    on_graph = (("graph.edge_index", graph.edge_index), ("graph.offsets", graph.offsets)) if isinstance(graph, SuperpixelGraph) \
        else (("graph offsets", graph[0]), ("graph indices", graph[1]))
    for what, t in named + on_graph:
        if isinstance(t, torch.Tensor):
            T.check_device(t, what)
            if t.device != dev:
                raise ValueError("%s must be on %s GPU %s, got %s" % (what, owner, dev, t.device))


def crf_edge_energies(graph, yxrgb, members, params=None, temporal=False):
    """The pairwise energies superpixel_crf computes for itself -> (edge float32 [nnz], links float32 [N, 2, K], or [2, K] for
    unbatched clusters).

    edge[k] is the spatial energy of neighbour entry k of the batch CSR (the pair as given, or graph.to_batch_csr()): 0.0 for a
    self-loop and for an entry whose index is outside [0, K).  links[n, 0, i] is the temporal energy of node i of frame n towards
    n - 1, links[n, 1, i] the one towards n + 1; 0.0 where there is no such frame or `temporal` is false.  The values are the very
    floats of the sweeps.  yxrgb [5, K] / [N, 5, K] float32 and members [K] / [N, K] int32 as for superpixel_crf.
    params: None, a dict, or a float32 [7] tensor on the clusters' GPU in PARAM_NAMES order, read on the device.  With a tensor that
    requires a gradient the result is differentiable with respect to it (terms and sums in double, a fixed order, no atomics); it is
    not differentiable with respect to yxrgb.  Runs on the current stream without host synchronisation."""
    T.check_float_map(yxrgb, (2, 3), "yxrgb", "[5, K] or [N, 5, K]")
    batched = yxrgb.dim() == 3
    N = yxrgb.shape[0] if batched else 1
    if yxrgb.shape[-2] != 5:
        raise ValueError("yxrgb must be [5, K] or [N, 5, K], got shape %s" % (tuple(yxrgb.shape),))
    K = int(yxrgb.shape[-1])
    lead = (N,) if batched else ()
    _check_tensor(members, torch.int32, lead + (K,), "members", "[K] or [N, K]")
    nnz = _check_neighbours(graph, N, K)
    if isinstance(params, torch.Tensor):
        _check_params_tensor(params)
    else:
        _check_params(params)
    if not isinstance(temporal, bool):
        raise ValueError("temporal must be True or False, got %r" % (temporal,))
    if N * K + 1 >= _LIMIT or nnz >= _LIMIT:
        raise ValueError("N * K + 1 and the number of neighbour entries must be below 2^31")
    T.check_device(yxrgb, "yxrgb")
    dev = yxrgb.device
    _check_same_device(dev, "yxrgb's", graph, (("members", members), ("params", params)))
    with torch.cuda.device(dev):
        offsets, indices = _batch_csr(graph)
        theta = params if isinstance(params, torch.Tensor) else _params_on(params, dev)
        edge, links = _energies(theta, yxrgb.contiguous(), members.contiguous(), offsets, indices, N, K, temporal)
    return edge, (links if batched else links[0])


def superpixel_crf(unaries, graph, yxrgb, members, max_iter=10, params=None, compat=None, temporal=False, q0=None, energies=None):
    """`max_iter` mean-field sweeps of SimpleCRF over `unaries` ([C, K] or [N, C, K] float32 energies on a ROCm GPU) -> q, a new
    tensor of the same shape.

    graph: a SuperpixelGraph, or (offsets int64 [N * K + 1], indices int32 [nnz]).  Rows may be empty, of any length, asymmetric, and
    hold duplicates and self-loops; an index outside [0, K) contributes nothing; row bounds are clamped into [0, nnz] and to
    non-decreasing on the device (nothing is validated on the host: that would synchronise).
    yxrgb [5, K] / [N, 5, K] float32, members [K] / [N, K] int32: the clusters.
    params: None or a dict over spatial_w, temporal_w, spatial_srgb, temporal_srgb, spatial_sxy, spatial_smooth_w,
    spatial_smooth_sxy (a fresh SimpleCRF's values for the names left out), or a float32 [7] tensor on the same GPU in PARAM_NAMES
    order, read on the device: the energies of crf_edge_energies, then the sweeps on them; q has the bits of the dict call with the
    same seven values.  compat: None (1.0 per class), C floats, or a float32 [C] tensor on the same GPU.
    energies: None, or (edge float32 [nnz], links float32 [N, 2, K] / [2, K]) on the same GPU in the layout of crf_edge_energies:
    the sweeps use them in place of computed ones, the weight of entry k being edge[k] times the member factor, also for a
    self-loop.  links may be None when temporal is false.  params must then be None and yxrgb may be None.
    temporal=False: the N frames are independent.  temporal=True: they are consecutive times of one window, node i of frame n
    linked to node i of n - 1 and n + 1, exactly as in SimpleCRF.
    q0: the starting q, float32 of the unaries' shape (never written); None: crf_expf(-unaries), which is SimpleCRF.initialize().
    max_iter=0 returns the starting q.

    Differentiable with respect to `unaries`, `q0` and a tensor `compat`: when gradients are enabled and one of them requires one,
    q is part of the autograd graph (the same bits; every iterate is kept for the backward, (max_iter + 1) * 4 * N * C * K bytes) and
    its backward is deterministic and once differentiable; q is then a view of the kept iterates, which autograd protects from
    in-place changes.  So is it with respect to a tensor `params` and to both `energies`: behind each sweep's adjoint one launch adds
    the sweep's part of the energy gradients, one owner thread per cell, and a params tensor receives the energies' backward of them.
    An entry whose index is outside [0, K), the link cells at the window's ends and all of links with temporal false get 0.0.
    `yxrgb`, `members` and the graph get no gradient.  Otherwise q has no grad_fn."""
    T.check_float_map(unaries, (2, 3), "unaries", "[C, K] or [N, C, K]")
    batched = unaries.dim() == 3
    N = unaries.shape[0] if batched else 1
    Cn, K = (int(v) for v in unaries.shape[-2:])
    lead = (N,) if batched else ()
    if yxrgb is not None or energies is None:
        if yxrgb is None:
            raise ValueError("yxrgb must be given unless energies are")
        _check_tensor(yxrgb, torch.float32, lead + (5, K), "yxrgb", "[5, K] or [N, 5, K]")
    _check_tensor(members, torch.int32, lead + (K,), "members", "[K] or [N, K]")
    if q0 is not None:
        _check_tensor(q0, torch.float32, tuple(unaries.shape), "q0", "the unaries' shape")
    nnz = _check_neighbours(graph, N, K)
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or max_iter < 0:
        raise ValueError("max_iter must be a non-negative integer, got %r" % (max_iter,))
    max_iter = int(max_iter)
    if max_iter >= _LIMIT:
        raise ValueError("max_iter must be below 2^31")
    p = edge = links = None
    if energies is not None and params is not None:
        raise ValueError("params must be None when energies are given")
    if isinstance(params, torch.Tensor):
        _check_params_tensor(params)
    elif energies is None:
        p = _check_params(params)
    compat = _check_compat(compat, Cn)
    if not isinstance(temporal, bool):
        raise ValueError("temporal must be True or False, got %r" % (temporal,))
    if energies is not None:
        edge, links = _check_energies(energies, nnz, lead, K, temporal)
    if N * Cn * K >= _LIMIT or N * K + 1 >= _LIMIT or nnz >= _LIMIT:
        raise ValueError("N * C * K, N * K + 1 and the number of neighbour entries must be below 2^31")
    T.check_device(unaries, "unaries")
    dev = unaries.device
    _check_same_device(dev, "the unaries'", graph, (("yxrgb", yxrgb), ("members", members), ("q0", q0), ("compat", compat),
                                                    ("params", params), ("energies: edge", edge), ("energies: links", links)))

    lib = _library()
    with torch.cuda.device(dev):
        offsets, indices = _batch_csr(graph)
        if compat is None:
            compat = torch.ones(Cn, dtype=torch.float32, device=dev)
        elif isinstance(compat, list):       # through pinned memory: an asynchronous copy, no host synchronisation
            compat = torch.tensor(compat, dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
        un, mem, comp = unaries.contiguous(), members.contiguous(), compat.contiguous()
        start = q0.contiguous() if q0 is not None else None

        def wants_grad(*tensors):
            return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)

        call = _Call(un, comp, mem, offsets, indices, N, max_iter, temporal)
        if p is not None:
            yx = yxrgb.contiguous()
            if wants_grad(unaries, q0, compat):
                return _SuperpixelCRF.apply(un, start, comp, yx.detach(), mem, offsets, indices, N, max_iter, temporal, p)
            return _plain(lib, lib.fslic_hip_crf_tensor_inference, call, call.from_params(p, yx), start)
        if energies is None:             # the composition: the energies from the params on the device, then the sweeps on them
            edge, links = _energies(params, yxrgb.contiguous(), mem, offsets, indices, N, K, temporal)
        edge = edge.contiguous()
        links = links.contiguous().view(N, 2, K) if links is not None else None
        if wants_grad(unaries, q0, compat, edge, links):
            return _SuperpixelCRFEnergies.apply(un, start, comp, edge, links, mem, offsets, indices, N, max_iter, temporal)
        lib = _energies_library()
        return _plain(lib, lib.fslic_hip_crf_tensor_inference_energies, call, call.from_energies(edge, links), start)
