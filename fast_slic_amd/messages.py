"""Messages over the neighbours of superpixels, on torch tensors in HBM (csrc/message.hip): the features of the two ends of every
neighbour entry as per-entry tensors, and the reduction of a per-entry tensor to the nodes -- so that what a node receives from a
neighbour may be any torch function of both ends of the entry and of the edge (EdgeConv's MLP on [x_i, x_j - x_i], GATv2's score, an
edge-conditioned convolution, PNA's sum / mean / max / min of the same messages), on the NeighbourLists of propagate.py, each with
exact, reproducible gradients.

    nl = neighbour_lists(graph)                                    # propagate.py
    xi = entry_gather(x, nl, end="target")                         # x float32 [N, C, K] -> float32 [C, nnz]: x[f, c, i], (f, i) = row(p)
    xj = entry_gather(x, nl, end="source")                         #                                          x[f, c, indices[p]]
    m = torch.relu(torch.einsum("oc,cp->op", w, torch.cat([xi, xj - xi])))        # any torch code per entry
    y = entry_reduce(m, nl, reduce="max")                          # [F, nnz] -> [N, F, K]; "sum", "mean", "max", "min"
    y, arg = entry_reduce(m, nl, reduce="min", return_argmax=True)
    z = entry_reduce(m, nl, reduce="sum", to="source")             # over nl.transposed(): what node j *sent*

The terms are propagate.py's and attention.py's: one CSR over the R = N * K rows (frame, node); entry p is *valid* when it lies inside
its row's clamped bounds and 0 <= indices[p] < K; row(p) = nl.rows[p] is the row whose bounds hold p, and nl.transposed() gives the
transposed lists.  A per-entry tensor is float32 [F, nnz], feature-major with the entries innermost (the layout of attention.py's
[Hd, nnz]); a 1-D [nnz] tensor is accepted where F = 1 (entry_reduce then returns [N, 1, K]) and its gradient comes back 1-D.  Every
sum and division below is one separately rounded float32 operation, nothing fused, the division correctly rounded.  The rules:

1. entry_gather.  out[c, p] = x[f, c, i] for end="target" and x[f, c, indices[p]] for end="source", with (f, i) = row(p).  An entry
   that is not valid, or whose row lies at or beyond N * K, gives +0.0.  The result is a copy: NaN and the sign of zero pass through.
   (A raw pair whose first offset is not 0 leaves the entries in front of it to row 0, as in attention.py.)
2. entry_reduce, to="target" (the default).  y[f, c, i] folds over the valid entries p of row (f, i) in ascending p:
       sum         acc = +0.0f;  acc = acc + m[c, p]
       mean        that sum divided by float32(d), d the number of valid entries; d = 0 gives +0.0
       max / min   the extremum; d = 0 gives +0.0.  An int32 [N, F, K] argmax is kept for the backward (return_argmax=True also returns
                   it, for "max" and "min" only): the smallest p that attains the extremum, -1 when d = 0.  NaN leaves the entry
                   unspecified.
3. entry_reduce, to="source".  The same folds over the transposed lists: y[f, c, j] folds m[c, t_entries[q]] over the transposed
   positions q of target (f, j) in ascending q, which is ascending p (crf_torch.transpose_batch_csr); d is the length of that list, and
   argmax still names the entry p.
4. Gradients.  Each call is a torch.autograd.Function with a once_differentiable backward; no atomics appear anywhere, and nothing
   flows to the graph.  entry_gather: grad_x is rule 2's sum of g for end="target" and rule 3's sum of g for end="source".
   entry_reduce, sum: grad_m[c, p] is rule 1's gather of g, at the target for to="target" and at the source for to="source"; mean: the
   same gather of g / float32(d), the gradient divided per node first, as the forward divided, and then gathered; max / min: g where
   argmax[f, c, node] == p and +0.0 elsewhere.  Every invalid entry gets +0.0.  So two kernel families close the set -- a gather with
   an optional per-node scale and argmax mask, a reduce in direct and transposed form -- and a numpy model written operation by
   operation (tests/messages_ref.py) reproduces every result and gradient bit for bit; the same bits come out from run to run.
5. Nothing a kernel reads from device memory becomes an address before it is checked (csrc/lists.h's rule): row bounds are clamped into
   [0, nnz] and an end before its start is an empty row; an index outside [0, K), an entry outside [0, nnz) and a row outside the
   target's frame contribute nothing.  Garbage lists give unspecified values, never an access out of bounds; knn_graph's padding
   (index -1) is simply not valid.

What follows from the rules, bit for bit: entry_reduce(entry_gather(x, nl, "source"), nl, r) is graph_aggregate(x, nl, reduce=r) for
sum, mean and max, with its argmax and its gradient for x; entry_reduce(w[None] * entry_gather(x, nl, "source"), nl) is
graph_aggregate(x, nl, weight=w); entry_reduce(m, nl, "sum", to="source") is attention.py's rule A transposed with weight m and g = 1.

Out of scope: float16 / bfloat16, a fused gather-MLP-reduce kernel, gradients to the graph, a `std` reduction (a mean of squares in
torch).

Every argument is checked before any device work (ValueError; two GPUs are refused first and a CPU tensor last).  Limits: N * C * K,
nnz and C * nnz below 2^31.  In place of `nl` a SuperpixelGraph or a raw pair (offsets int64 [N * K + 1], indices int32 [nnz]) is
accepted, whose lists are then built once per call.  Every call runs on torch's current stream of the tensors' GPU, takes its results
from torch's caching allocator and never synchronises the host.  There is no CPU fallback.
This module imports torch; the package itself does not import it.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _binding as B, _tensors as T
from .propagate import LIMIT, NeighbourLists, as_lists, check_lists, check_map, differentiable, lists_tensors
from .rag import SuperpixelGraph, check_graph

__all__ = ["entry_gather", "entry_reduce"]

_ENTRY = ("fslic_hip_message_reduce", "message entry points")
_END = {"target": 0, "source": 1}                                          # kMsgTarget, kMsgSource; also the `transposed` of a reduce
_REDUCE = {"sum": 0, "mean": 1, "max": 2, "min": 3}                        # kMsgSum, kMsgMean, kMsgMax, kMsgMin
_LIMIT_TEXT = "N * C * K, the number of neighbour entries and C * entries must be below 2^31"


def _check_messages(t, nnz):
    """-> F of a per-entry tensor float32 [F, nnz] or [nnz] (F = 1)."""
    text = "[F, nnz] or [nnz] with nnz = %d, one per feature and neighbour entry" % nnz
    T.check_tensor(t, "messages", (torch.float32,), text, lambda s: len(s) in (1, 2) and s[-1] == nnz and (len(s) == 1 or s[0] >= 1))
    return int(t.shape[0]) if t.dim() == 2 else 1


def _check_limits(cells, nnz, Cc):
    if cells >= LIMIT or nnz >= LIMIT or Cc * nnz >= LIMIT:
        raise ValueError(_LIMIT_TEXT)


# ---- the launches, on contiguous tensors of one GPU; nl a NeighbourLists ----
def _gather(x, nl, end, degree=None, argmax=None):
    """-> float32 [C, nnz] of x float32 [N, C, K]: rule 1, with the per-node scale or the argmax mask of a reduce's backward."""
    lib, dev = T.library(*_ENTRY), x.device
    N, Cc, K = (int(v) for v in x.shape)
    nnz = int(nl.indices.shape[0])
    with torch.cuda.device(dev):
        out = torch.empty((Cc, nnz), dtype=torch.float32, device=dev)
        B._check(lib.fslic_hip_message_gather(dev.index, T.stream(dev), N, Cc, K, nnz, end, T.ptr(nl.rows, nnz), T.ptr(nl.indices, nnz), x.data_ptr(),
                                              T.ptr(degree), T.ptr(argmax), T.ptr(out, nnz)))
    return out


def _reduce(m, nl, mode, transposed):
    """-> (y float32 [N, F, K], argmax int32 [N, F, K] or None, degree int32 [N * K] or None) of m float32 [F, nnz]."""
    lib, dev = T.library(*_ENTRY), m.device
    N, K, Fc, nnz = nl.num_frames, nl.num_components, int(m.shape[0]), int(nl.indices.shape[0])
    with torch.cuda.device(dev):
        offsets, ia, ib = nl.transposed() if transposed else (nl.offsets, nl.indices, None)
        y = torch.empty((N, Fc, K), dtype=torch.float32, device=dev)
        argmax = torch.empty((N, Fc, K), dtype=torch.int32, device=dev) if mode in (_REDUCE["max"], _REDUCE["min"]) else None
        degree = torch.empty(N * K, dtype=torch.int32, device=dev) if mode == _REDUCE["mean"] else None
        B._check(lib.fslic_hip_message_reduce(dev.index, T.stream(dev), N, Fc, K, nnz, mode, int(transposed), offsets.data_ptr(), T.ptr(ia, nnz),
                                              T.ptr(ib, nnz), T.ptr(m, nnz), y.data_ptr(), T.ptr(argmax), T.ptr(degree)))
    return y, argmax, degree


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, nl, end):
        ctx.nl, ctx.end = nl, end
        return _gather(x, nl, end)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return _reduce(g.contiguous(), ctx.nl, _REDUCE["sum"], ctx.end)[0], None, None


class _Reduce(torch.autograd.Function):
    """entry_reduce on contiguous tensors of one GPU -> (y, argmax or None); the gradient for m."""

    @staticmethod
    def forward(ctx, m, nl, mode, transposed):
        y, argmax, degree = _reduce(m, nl, mode, transposed)
        ctx.save_for_backward(argmax, degree)
        ctx.nl, ctx.transposed = nl, transposed
        if argmax is not None:
            ctx.mark_non_differentiable(argmax)
        return y, argmax

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        argmax, degree = ctx.saved_tensors
        return _gather(g.contiguous(), ctx.nl, ctx.transposed, degree, argmax), None, None, None


# ---- the public functions ----
def entry_gather(x, nl, end="target"):
    """The features of one end of every neighbour entry, by rule 1 of the module's text: `x` float32 [N, C, K] ([C, K] when N = 1) ->
    float32 [C, nnz], x at the entry's own row (end="target") or at its neighbour indices[p] (end="source"); +0.0 for an entry that is
    not valid.  Differentiable with respect to `x`; one launch forward and one backward, no host synchronisation."""
    N, Cc, K = check_map(x, "x")
    nnz = check_lists(nl, N, K)
    if not isinstance(end, str) or end not in _END:
        raise ValueError("end must be 'target' or 'source', got %r" % (end,))
    _check_limits(N * Cc * K, nnz, Cc)
    dev = T.one_device([(x, "x")] + lists_tensors(nl))
    with torch.cuda.device(dev):
        nl = as_lists(nl, N, K)
        x3 = x.reshape(N, Cc, K).contiguous()
        if differentiable(x3):
            return _Gather.apply(x3, nl, _END[end])
        return _gather(x3, nl, _END[end])


def entry_reduce(messages, nl, reduce="sum", to="target", *, return_argmax=False, num_frames=None, num_components=None):
    """`messages` float32 [F, nnz] (or [nnz], F = 1) reduced over the entries of every node, by rules 2 and 3 -> float32 [N, F, K]:
    to="target" over each row's own entries (what node i receives), to="source" over the transposed lists (what node j sent).  reduce:
    "sum", "mean", "max" or "min"; with return_argmax=True and "max" or "min" the result is (y, argmax int32 [N, F, K]).  A raw pair in
    place of `nl` needs num_frames = N and num_components = K, as neighbour_lists does.  Differentiable with respect to `messages`;
    one launch forward and one backward, no host synchronisation."""
    if isinstance(nl, NeighbourLists):
        N, K = nl.num_frames, nl.num_components
    elif isinstance(nl, SuperpixelGraph):
        N, K = check_graph(nl)[:2]
    else:
        N, K = T.check_count(num_frames, "num_frames"), T.check_count(num_components, "num_components")
    if (num_frames, num_components) not in ((None, None), (N, K)):
        raise ValueError("the graph has %d frames of %d nodes, not %r of %r" % (N, K, num_frames, num_components))
    nnz = check_lists(nl, N, K)
    Fc = _check_messages(messages, nnz)
    if not isinstance(reduce, str) or reduce not in _REDUCE:
        raise ValueError("reduce must be 'sum', 'mean', 'max' or 'min', got %r" % (reduce,))
    if not isinstance(to, str) or to not in _END:
        raise ValueError("to must be 'target' or 'source', got %r" % (to,))
    if return_argmax and reduce not in ("max", "min"):
        raise ValueError("return_argmax goes with reduce='max' and 'min' only, got reduce=%r" % reduce)
    _check_limits(N * Fc * K, nnz, Fc)
    dev = T.one_device([(messages, "messages")] + lists_tensors(nl))
    with torch.cuda.device(dev):
        nl = as_lists(nl, N, K)
        m = messages.reshape(Fc, nnz).contiguous()
        if differentiable(m):
            y, argmax = _Reduce.apply(m, nl, _REDUCE[reduce], _END[to])
        else:
            y, argmax, _ = _reduce(m, nl, _REDUCE[reduce], _END[to])
    return (y, argmax) if return_argmax else y
