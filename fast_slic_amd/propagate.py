"""Propagating features along the region adjacency graph, on torch tensors in HBM (csrc/aggregate.hip): the neighbour lists of a graph as
an object of their own, and weighted aggregation over them with exact, reproducible gradients.

    nl = neighbour_lists(graph)                                    # graph: a SuperpixelGraph, or (offsets, indices) with N and K given
    nl.offsets, nl.indices                                         # int64 [N * K + 1], int32 [nnz]: exactly graph.to_batch_csr()
    nl.edge                                                        # int64 [nnz]: the position in graph.edge_index of each entry (None for a raw pair)
    nl.rows                                                        # int32 [nnz]: the row over (frame, node) of each entry
    nl.degree()                                                    # int32 [N, K]: the entries of each row
    nl.entry_values(t)                                             # t [E] or [E, F] per undirected edge -> [nnz] / [nnz, F]: t[nl.edge]
    nl.transposed()                                                # (t_offsets, t_entries, t_rows) of crf_torch.transpose_batch_csr, computed once
    y = graph_aggregate(values, nl, weight=None, reduce="sum")     # values float32 [N, C, K] or [C, K] -> the same shape

The lists are one CSR over the N * K rows (frame, node): the neighbours of node i of frame f are indices[offsets[f * K + i] :
offsets[f * K + i + 1]], node numbers inside the frame.  neighbour_lists is plain torch (a sort of unique keys and searchsorted, as
SuperpixelGraph.to_batch_csr, with the edge's position carried along), works on any device and does not synchronise the host.  An
entry p of row (f, i) is *valid* when 0 <= indices[p] < K; every other entry contributes nothing anywhere.  The rules of
graph_aggregate:

1. reduce="sum".  y[f, c, i] is the left fold over the valid entries p of the row, in ascending p:
       acc = +0.0f;  acc = acc + (weight[p] * x[f, c, indices[p]])
   the product and the sum two separately rounded float32 operations, nothing fused.  Without `weight` the term is x[...] itself.  An
   empty row gives +0.0.  `weight` is float32 [nnz], one value per directed entry: entry p of row i scales what i receives from
   indices[p].
2. reduce="mean".  The unweighted sum of rule 1 divided by float32(d), d the number of valid entries of the row; the division is
   correctly rounded.  d = 0 gives +0.0.  A weight is refused.
3. reduce="max".  The maximum of x over the valid entries; d = 0 gives +0.0.  The call keeps an int32 [N, C, K] argmax for the
   backward (return_argmax=True also returns it): the smallest p that attains the maximum, -1 when d = 0.  NaN inputs leave the
   entry unspecified.  A weight is refused.
4. Gradients.  The call is a torch.autograd.Function with a once_differentiable backward, and no atomics appear anywhere in it.
   Sum: grad_x[f, c, j] is the left fold over the transposed list of target (f, j), in ascending entry order, of
   weight[p] * g[f, c, row(p)] (g[...] itself without a weight); grad_weight[p] is the left fold over c = 0 .. C - 1 of
   x[f, c, indices[p]] * g[f, c, row(p)], and +0.0 for an invalid entry.  Mean: the term is g[f, c, row(p)] / float32(d of row(p)), g
   first divided as the forward divided, then the unweighted sum backward.  Max: grad_x[f, c, j] folds g[f, c, row(p)] over the
   transposed entries p with argmax[f, c, row(p)] == p.  All folds are separately rounded float32 operations, so a numpy model
   written operation by operation (tests/aggregate_ref.py) reproduces every gradient bit for bit, and the same bits come out from run
   to run.  Nothing flows to the graph.  entry_values' own backward is deterministic as well: it is a torch gather whose backward
   adds exactly two entries per edge, and a float sum of two terms does not depend on their order.

Nothing of a raw pair is trusted on the device: a kernel clamps each row's bounds into [0, nnz], a row whose end lies before its start
is empty, and no index outside [0, K) is ever dereferenced: garbage gives unspecified values, never an access out of bounds.

Out of scope: self loops and normalisations as arguments (one elementwise torch line each: README), float16 / bfloat16, torch sparse
tensors, gradients to anything but `values` and `weight`.  A softmax over a node's entries, several weight heads and the score of an
entry from its two ends are attention.py's (neighbour_softmax, head_aggregate, neighbour_dot), on these lists.

Every argument is checked before any device work (ValueError; two GPUs are refused first and a CPU tensor last).  graph_aggregate
runs on torch's current stream of the tensors' GPU, takes its results and what it keeps for the backward from torch's caching
allocator and never synchronises the host.  There is no CPU fallback.
This module imports torch; the package itself does not import it.
"""
import numbers

import torch
from torch.autograd.function import once_differentiable

from . import _binding as B, _tensors as T
from .crf_torch import transpose_batch_csr
from .rag import SuperpixelGraph, check_graph

__all__ = ["neighbour_lists", "graph_aggregate", "NeighbourLists"]

_REDUCE = {"sum": 0, "mean": 1, "max": 2}                                  # kAggSum, kAggMean, kAggMax
LIMIT = 1 << 31                                                           # sizes and entry counts stay below it
_ENTRY = ("fslic_hip_aggregate_forward", "aggregation entry points")


class NeighbourLists(object):
    """What neighbour_lists returns: offsets int64 [N * K + 1], indices int32 [nnz], edge int64 [nnz] or None, rows int32 [nnz],
    num_frames N and num_components K."""

    def __init__(self, offsets, indices, edge, rows, num_frames, num_components):
        self.offsets, self.indices, self.edge, self.rows = offsets, indices, edge, rows
        self.num_frames, self.num_components = num_frames, num_components
        self._transposed = None

    def degree(self):
        """int32 [N, K]: the entries of each row."""
        return (self.offsets[1:] - self.offsets[:-1]).to(torch.int32).view(self.num_frames, self.num_components)

    def entry_values(self, t):
        """t [E] or [E, F], one value per undirected edge of the graph (boundary, contrast, a learnt tensor) -> [nnz] / [nnz, F]: both
        directed entries of an edge take the edge's value.  Plain torch, differentiable."""
        if self.edge is None:
            raise ValueError("entry_values needs the lists of a SuperpixelGraph; a raw pair has no edges")
        E = int(self.edge.shape[0]) // 2
        if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2) or t.shape[0] != E:
            raise ValueError("t must be a torch tensor [E] or [E, F] with E = %d, one per edge of the graph" % E)
        return t[self.edge]

    def transposed(self):
        """(t_offsets int64 [N * K + 1], t_entries int32 [nnz], t_rows int32 [nnz]) of crf_torch.transpose_batch_csr, computed once."""
        if self._transposed is None:
            self._transposed = transpose_batch_csr(self.offsets, self.indices, self.num_frames, self.num_components)
        return self._transposed


# ---- argument checks: all of them run before any device work ----
def _check_pair(graph, N, K):
    if not isinstance(graph, (tuple, list)) or len(graph) != 2:
        raise ValueError("graph must be a SuperpixelGraph or a pair (offsets, indices)")
    offsets, indices = graph
    T.check_tensor(offsets, "graph offsets", (torch.int64,), "[N * K + 1] = [%d]" % (N * K + 1), lambda s: s == (N * K + 1,))
    T.check_tensor(indices, "graph indices", (torch.int32,), "[nnz]", lambda s: len(s) == 1)


def check_lists(lists, N, K):
    """-> nnz of a NeighbourLists, a SuperpixelGraph or a raw pair for N frames of K nodes, known without looking at device memory."""
    if isinstance(lists, NeighbourLists):
        n, k = lists.num_frames, lists.num_components
    elif isinstance(lists, SuperpixelGraph):
        n, k, E, _ = check_graph(lists)
    else:
        _check_pair(lists, N, K)
        return int(lists[1].shape[0])
    if (n, k) != (N, K):
        raise ValueError("the graph has %d frames of %d nodes, the values have %d of %d" % (n, k, N, K))
    return int(lists.indices.shape[0]) if isinstance(lists, NeighbourLists) else 2 * E


def lists_tensors(nl):
    """The tensors of `nl` (checked by check_lists) that name its device, for _tensors.one_device."""
    if isinstance(nl, NeighbourLists):
        return [(nl.offsets, "nl.offsets"), (nl.indices, "nl.indices")]
    if isinstance(nl, SuperpixelGraph):
        return [(nl.edge_index, "graph.edge_index"), (nl.offsets, "graph.offsets")]
    return [(nl[0], "graph offsets"), (nl[1], "graph indices")]


def as_lists(nl, N, K):
    """`nl` itself, or the NeighbourLists of a SuperpixelGraph or a raw pair, built once per call."""
    return nl if isinstance(nl, NeighbourLists) else neighbour_lists(nl, N, K)


def check_map(t, what):
    """-> (N, C, K) of a float32 [N, C, K] or [C, K] tensor."""
    T.check_float_map(t, (2, 3), what, "[C, K] or [N, C, K]")
    Cc, K = (int(v) for v in t.shape[-2:])
    T.check_count(K, "K, the last dimension of %s," % what)
    return (int(t.shape[0]) if t.dim() == 3 else 1), Cc, K


def check_heads(heads, Cc, what="C"):
    if isinstance(heads, bool) or not isinstance(heads, numbers.Integral) or heads < 1:
        raise ValueError("heads must be a positive integer, got %r" % (heads,))
    if Cc % heads != 0:
        raise ValueError("%s = %d is not a multiple of heads = %d" % (what, Cc, heads))
    return int(heads)


def differentiable(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def neighbour_lists(graph, num_frames=None, num_components=None):
    """The NeighbourLists of a SuperpixelGraph, or of a raw pair (offsets int64 [N * K + 1], indices int32 [nnz]) with num_frames = N
    and num_components = K given.  Plain torch on the graph's device, no host synchronisation."""
    if not isinstance(graph, SuperpixelGraph):
        N, K = T.check_count(num_frames, "num_frames"), T.check_count(num_components, "num_components")
        _check_pair(graph, N, K)
        offsets, indices = graph[0].contiguous(), graph[1].contiguous()
        nnz = indices.shape[0]
        # the row of entry p: how many rows end at or before p (N * K: behind the last row)
        rows = torch.searchsorted(offsets[1:].contiguous(), torch.arange(nnz, dtype=torch.int64, device=indices.device), right=True)
        return NeighbourLists(offsets, indices, None, rows.to(torch.int32), N, K)
    N, K, E, _ = check_graph(graph)
    if num_frames not in (None, N) or num_components not in (None, K):
        raise ValueError("the graph has %d frames of %d nodes, not %r of %r" % (N, K, num_frames, num_components))
    dev = graph.edge_index.device
    frame = torch.searchsorted(graph.offsets[1:].contiguous(), torch.arange(E, dtype=torch.int64, device=dev), right=True)
    a, b = graph.edge_index[0], graph.edge_index[1]
    # key = (row over (frame, node)) * K + neighbour, as to_batch_csr: unique, so any sort gives this order; the sort's permutation
    # names the half of the concatenation, and so the edge, each entry came from
    flat, order = torch.cat([(frame * K + a) * K + b, (frame * K + b) * K + a]).sort()
    rows = torch.div(flat, K, rounding_mode="floor")
    offsets = torch.searchsorted(rows, torch.arange(N * K + 1, dtype=torch.int64, device=dev))
    return NeighbourLists(offsets, (flat - rows * K).to(torch.int32), torch.where(order >= E, order - E, order), rows.to(torch.int32), N, K)


# ---- the launches, on contiguous tensors of one GPU ----
def _forward(x, nl, w, mode):
    """-> (y, argmax or None, degree or None) of x float32 [N, C, K]."""
    lib, dev = T.library(*_ENTRY), x.device
    N, Cc, K = (int(v) for v in x.shape)
    nnz = int(nl.indices.shape[0])
    with torch.cuda.device(dev):
        y = torch.empty_like(x)
        argmax = torch.empty((N, Cc, K), dtype=torch.int32, device=dev) if mode == _REDUCE["max"] else None
        degree = torch.empty(N * K, dtype=torch.int32, device=dev) if mode == _REDUCE["mean"] else None
        B._check(lib.fslic_hip_aggregate_forward(dev.index, T.stream(dev), N, Cc, K, nnz, mode, nl.offsets.data_ptr(), T.ptr(nl.indices, nnz),
                                                 T.ptr(w, nnz), x.data_ptr(), y.data_ptr(), T.ptr(argmax), T.ptr(degree)))
    return y, argmax, degree


class _Aggregate(torch.autograd.Function):
    """graph_aggregate on contiguous tensors of one GPU -> (y, argmax or None); gradients for x and w."""

    @staticmethod
    def forward(ctx, x, w, nl, mode):
        y, argmax, degree = _forward(x, nl, w, mode)
        ctx.save_for_backward(x, w, argmax, degree)
        ctx.nl, ctx.mode = nl, mode
        if argmax is not None:
            ctx.mark_non_differentiable(argmax)
        return y, argmax

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        x, w, argmax, degree = ctx.saved_tensors
        nl, lib, dev = ctx.nl, T.library(*_ENTRY), x.device
        N, Cc, K = (int(v) for v in x.shape)
        nnz = int(nl.indices.shape[0])
        head = (dev.index, T.stream(dev), N, Cc, K, nnz)
        dx = dw = None
        with torch.cuda.device(dev):
            g = g.contiguous()
            if ctx.needs_input_grad[0]:
                t_offsets, t_entries, t_rows = nl.transposed()
                dx = torch.empty_like(x)
                B._check(lib.fslic_hip_aggregate_backward_values(*head, ctx.mode, t_offsets.data_ptr(), T.ptr(t_entries, nnz), T.ptr(t_rows, nnz),
                                                                 T.ptr(w, nnz), T.ptr(argmax), T.ptr(degree), g.data_ptr(), dx.data_ptr()))
            if w is not None and ctx.needs_input_grad[1]:
                dw = torch.empty_like(w)
                B._check(lib.fslic_hip_aggregate_backward_weight(*head, T.ptr(nl.rows, nnz), T.ptr(nl.indices, nnz), x.data_ptr(), g.data_ptr(),
                                                                 T.ptr(dw, nnz)))
        return dx, dw, None, None


def graph_aggregate(values, nl, weight=None, reduce="sum", *, return_argmax=False):
    """`values` float32 [N, C, K] ([C, K] when N = 1) aggregated over the neighbours of every node -> a new tensor of the same shape, by
    rules 1 to 4 of the module's text.  `nl`: NeighbourLists, or a SuperpixelGraph or a raw pair (offsets int64 [N * K + 1], indices
    int32 [nnz]), whose lists are then built once per call.  `weight`: None or float32 [nnz], with reduce="sum" only.  reduce: "sum",
    "mean" or "max"; with return_argmax=True and "max" the result is (y, argmax int32 of the values' shape).  Differentiable with
    respect to `values` and `weight`; one launch forward, one for each gradient, no host synchronisation."""
    N, Cc, K = check_map(values, "values")
    nnz = check_lists(nl, N, K)
    if not isinstance(reduce, str) or reduce not in _REDUCE:
        raise ValueError("reduce must be 'sum', 'mean' or 'max', got %r" % (reduce,))
    if weight is not None:
        if reduce != "sum":
            raise ValueError("a weight goes with reduce='sum' only, got reduce=%r" % reduce)
        T.check_tensor(weight, "weight", (torch.float32,), "[nnz] with nnz = %d, one per neighbour entry" % nnz, lambda s: s == (nnz,))
    if return_argmax and reduce != "max":
        raise ValueError("return_argmax goes with reduce='max' only, got reduce=%r" % reduce)
    if N * Cc * K >= LIMIT or nnz >= LIMIT:
        raise ValueError("N * C * K and the number of neighbour entries must be below 2^31")
    dev = T.one_device([(values, "values"), (weight, "weight")] + lists_tensors(nl))

    with torch.cuda.device(dev):
        nl = as_lists(nl, N, K)
        x = values.reshape(N, Cc, K).contiguous()
        w = weight.contiguous() if weight is not None else None
        mode = _REDUCE[reduce]
        if differentiable(x, w):
            y, argmax = _Aggregate.apply(x, w, nl, mode)
        else:
            y, argmax, _ = _forward(x, nl, w, mode)
    y = y.view(values.shape)
    return (y, argmax.view(values.shape)) if return_argmax else y
