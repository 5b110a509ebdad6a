"""Attention over the neighbours of superpixels, on torch tensors in HBM (csrc/attend.hip): the score of a neighbour entry from the
features of its two ends, a softmax over each node's entries, and a neighbour sum with one weight per head -- the three steps of a
graph-attention or graph-transformer layer between superpixel_pool and superpixel_unpool, on the NeighbourLists of propagate.py, each
with exact, reproducible gradients.

    nl = neighbour_lists(graph)                                    # propagate.py
    s = neighbour_dot(a, b, nl, heads=Hd)                          # a, b float32 [N, C, K] -> float32 [Hd, nnz]
    alpha = neighbour_softmax(s, nl)                               # [Hd, nnz] (or [nnz]) -> the same shape
    y = head_aggregate(values, nl, alpha)                          # values [N, Cv, K], alpha [Hd, nnz] -> [N, Cv, K]
    y = graph_attention(query, key, values, nl, heads=Hd)          # the three in sequence, the query scaled by D ** -0.5

The terms are propagate.py's: one CSR over the R = N * K rows (frame, node); entry p of row (f, i) is *valid* when it lies inside the
row's clamped bounds and 0 <= indices[p] < K, and row(p) is the row whose bounds hold p.  Hd is the number of heads, D = C / Hd the
channels of a head (C % Hd != 0 is refused) and h(c) = c // D the head of channel c.  A per-entry tensor is float32 [Hd, nnz],
head-major with the entries innermost; where Hd = 1 a 1-D [nnz] tensor is accepted and comes back 1-D.  Every product, sum, difference
and division below is one separately rounded float32 operation, nothing fused, the division correctly rounded.  The rules:

1. neighbour_dot.  For entry p with (f, i) = row(p) and j = indices[p], s[h, p] is the left fold over c = h D .. h D + D - 1:
       acc = +0.0f;  acc = acc + (a[f, c, i] * b[f, c, j])
   An entry that is not valid, or whose row lies at or beyond N * K, gives +0.0.  (The row of an entry is nl.rows[p]; a raw pair
   whose first offset is not 0 leaves the entries in front of it to row 0.)
2. neighbour_softmax.  For each head and row: m = the maximum of the scores of the row's valid entries; e_p = expf(s_p - m), expf the
   library's crf_expf (csrc/crf.h: glibc's expf bit for bit, on the host as fslic_hip_crf_expf_host(.., use_libm=0)); Z = the left
   fold of e_p over the valid entries in ascending p from +0.0; alpha_p = e_p / Z.  Z >= 1 always: the largest entry contributes
   expf(0) = 1.  An entry that is not valid gets +0.0 and takes part in neither m nor Z.  Defined for rows whose valid scores are
   finite or -inf with at least one finite; NaN and +inf leave the row unspecified.
3. head_aggregate (rule A).  y[f, c, i] is the left fold over the row's valid entries in ascending p:
       acc = +0.0f;  acc = acc + (weight[h(c), p] * x[f, c, indices[p]])
   With Hd = 1 these are the bits of graph_aggregate(values, nl, weight=w), and so are its gradients.
4. Gradients.  Every call is a torch.autograd.Function with a once_differentiable backward; no atomics appear anywhere.
   head_aggregate: grad_values[f, c, j] is the left fold over nl.transposed() of target (f, j), in ascending entry order, of
   weight[h(c), p] * g[f, c, row(p)] (rule A transposed); grad_weight[h, p] is rule 1's fold of x[f, c, indices[p]] * g[f, c, row(p)].
   neighbour_dot: grad_a is rule A with values = b and weight = grad_s; grad_b is rule A transposed with g = a and weight = grad_s.
   neighbour_softmax, from the alpha it returned: t = the left fold over the row's valid entries of alpha_p * g_p; grad_s_p =
   alpha_p * (g_p - t), and +0.0 for an entry that is not valid.
   The dot and the sum are each other's gradients, so three kernel families close the set, and a numpy model written operation by
   operation (tests/attention_ref.py) reproduces every result and gradient bit for bit; the same bits come out from run to run.
   Nothing flows to the graph.
5. graph_attention(query, key, values, nl, heads, scale) is
       head_aggregate(values, nl, neighbour_softmax(neighbour_dot(query * float32(scale), key, nl, heads), nl))
   scale = D ** -0.5 unless given, the multiplication plain torch; `values` may have a channel count Cv of its own (Cv % Hd == 0).  It
   adds no kernel: its result and every gradient are those of the composition, bit for bit.

The GAT score el[i] + er[j] is a dot with two channels per head: a = [el; 1], b = [1; er] (README).

Nothing of a raw pair is trusted on the device, by csrc/lists.h's rule: nothing a kernel reads from device memory becomes an address
before it is checked: row bounds are clamped into [0, nnz] and an end before its start is an empty row; an index outside [0, K), an
entry outside [0, nnz) and a row outside the target's frame contribute nothing.

Out of scope: float16 / bfloat16, dropout on alpha, gradients to the graph, torch sparse tensors, one fused kernel (the three steps
stay three launches, each a rule a model can state).

Every argument is checked before any device work (ValueError; two GPUs are refused first and a CPU tensor last).  Limits: N * C * K,
nnz and Hd * nnz below 2^31.  In place of `nl` a SuperpixelGraph or a raw pair (offsets int64 [N * K + 1], indices int32 [nnz]) is
accepted, whose lists are then built once per call.  Every call runs on torch's current stream of the tensors' GPU, takes its results
from torch's caching allocator and never synchronises the host.  There is no CPU fallback.
This module imports torch; the package itself does not import it.
"""
import numbers

import torch
from torch.autograd.function import once_differentiable

from . import _binding as B, _tensors as T
from .propagate import (LIMIT, NeighbourLists, as_lists, check_heads, check_lists, check_map, differentiable, lists_tensors,
                        neighbour_lists)      # neighbour_lists: kept as attention.neighbour_lists for callers of this module
from .rag import SuperpixelGraph, check_graph

__all__ = ["neighbour_dot", "neighbour_softmax", "head_aggregate", "graph_attention"]

_ENTRY = ("fslic_hip_attend_apply", "attention entry points")
_LIMIT_TEXT = "N * C * K, the number of neighbour entries and heads * entries must be below 2^31"


# ---- argument checks: all of them run before any device work ----
def _check_entries(t, what, nnz, heads=None):
    """-> Hd of a per-entry tensor float32 [Hd, nnz] or [nnz] (Hd = 1); `heads`: the Hd it must have."""
    text = "[Hd, nnz] or [nnz] with nnz = %d, one per head and neighbour entry" % nnz
    T.check_tensor(t, what, (torch.float32,), text, lambda s: len(s) in (1, 2) and s[-1] == nnz and (len(s) == 1 or s[0] >= 1))
    Hd = int(t.shape[0]) if t.dim() == 2 else 1
    if heads is not None and Hd != heads:
        raise ValueError("%s has %d heads, not %d" % (what, Hd, heads))
    return Hd


def _check_limits(cells, nnz, Hd):
    if cells >= LIMIT or nnz >= LIMIT or Hd * nnz >= LIMIT:
        raise ValueError(_LIMIT_TEXT)


# ---- the launches, on contiguous tensors of one GPU; nl a NeighbourLists ----
def _head(x, nl):
    N, Cc, K = (int(v) for v in x.shape)
    return (x.device.index, T.stream(x.device), N, Cc, K, int(nl.indices.shape[0]))


def _dot(a, b, nl, Hd):
    """-> s float32 [Hd, nnz] of a, b float32 [N, C, K]."""
    lib, nnz = T.library(*_ENTRY), int(nl.indices.shape[0])
    with torch.cuda.device(a.device):
        out = torch.empty((Hd, nnz), dtype=torch.float32, device=a.device)
        B._check(lib.fslic_hip_attend_dot(*_head(a, nl), Hd, T.ptr(nl.rows, nnz), T.ptr(nl.indices, nnz), a.data_ptr(), b.data_ptr(), T.ptr(out, nnz)))
    return out


def _softmax(t, g, nl):
    """t float32 [Hd, nnz] -> its softmax (g None), or the gradient of the scores from t = alpha and g."""
    lib, dev, nnz = T.library(*_ENTRY), t.device, int(nl.indices.shape[0])
    head = (dev.index, T.stream(dev), nl.num_frames, nl.num_components, nnz, int(t.shape[0]), nl.offsets.data_ptr(), T.ptr(nl.indices, nnz))
    with torch.cuda.device(dev):
        out = torch.empty_like(t)
        if g is None:
            B._check(lib.fslic_hip_attend_softmax(*head, T.ptr(t, nnz), T.ptr(out, nnz)))
        else:
            B._check(lib.fslic_hip_attend_softmax_backward(*head, T.ptr(t, nnz), T.ptr(g, nnz), T.ptr(out, nnz)))
    return out


def _apply(x, w, nl, transposed):
    """Rule A (or, transposed, its form over nl.transposed()) of x float32 [N, C, K] with w float32 [Hd, nnz]."""
    lib, nnz = T.library(*_ENTRY), int(nl.indices.shape[0])
    with torch.cuda.device(x.device):
        offsets, ia, ib = nl.transposed() if transposed else (nl.offsets, nl.indices, None)
        out = torch.empty_like(x)
        B._check(lib.fslic_hip_attend_apply(*_head(x, nl), int(w.shape[0]), int(transposed), offsets.data_ptr(), T.ptr(ia, nnz), T.ptr(ib, nnz),
                                            T.ptr(w, nnz), x.data_ptr(), out.data_ptr()))
    return out


class _Dot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, nl, Hd):
        ctx.save_for_backward(a, b)
        ctx.nl = nl
        return _dot(a, b, nl, Hd)

    @staticmethod
    @once_differentiable
    def backward(ctx, gs):
        a, b = ctx.saved_tensors
        gs = gs.contiguous()
        return (_apply(b, gs, ctx.nl, False) if ctx.needs_input_grad[0] else None,
                _apply(a, gs, ctx.nl, True) if ctx.needs_input_grad[1] else None, None, None)


class _Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, nl):
        alpha = _softmax(s, None, nl)
        ctx.save_for_backward(alpha)
        ctx.nl = nl
        return alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        alpha, = ctx.saved_tensors
        return _softmax(alpha, g.contiguous(), ctx.nl), None


class _Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, nl):
        ctx.save_for_backward(x, w)
        ctx.nl = nl
        return _apply(x, w, nl, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        return (_apply(g, w, ctx.nl, True) if ctx.needs_input_grad[0] else None,
                _dot(g, x, ctx.nl, int(w.shape[0])) if ctx.needs_input_grad[1] else None, None)


# ---- the public functions ----
def neighbour_dot(a, b, nl, heads=1):
    """The score of every neighbour entry from the features of its two ends, by rule 1 of the module's text: `a` (read at the entry's
    row) and `b` (read at its neighbour) float32 [N, C, K] ([C, K] when N = 1) of one shape -> float32 [heads, nnz].  Differentiable
    with respect to both; one launch forward, one for each gradient, no host synchronisation."""
    N, Cc, K = check_map(a, "a")
    T.check_tensor(b, "b", (torch.float32,), "the shape of a, %s" % (tuple(a.shape),), lambda s: s == tuple(a.shape))
    nnz = check_lists(nl, N, K)
    Hd = check_heads(heads, Cc)
    _check_limits(N * Cc * K, nnz, Hd)
    dev = T.one_device([(a, "a"), (b, "b")] + lists_tensors(nl))
    with torch.cuda.device(dev):
        nl = as_lists(nl, N, K)
        a3, b3 = a.reshape(N, Cc, K).contiguous(), b.reshape(N, Cc, K).contiguous()
        return _Dot.apply(a3, b3, nl, Hd) if differentiable(a3, b3) else _dot(a3, b3, nl, Hd)


def neighbour_softmax(scores, nl, *, num_frames=None, num_components=None):
    """The softmax of `scores` (float32 [Hd, nnz], or [nnz]) over the valid entries of each row, per head, by rule 2 -> the shape of
    `scores`.  A raw pair in place of `nl` needs num_frames = N and num_components = K, as neighbour_lists does.  Differentiable; one
    launch forward and one backward, no host synchronisation."""
    if isinstance(nl, NeighbourLists):
        N, K = nl.num_frames, nl.num_components
    elif isinstance(nl, SuperpixelGraph):
        N, K = check_graph(nl)[:2]
    else:
        N, K = T.check_count(num_frames, "num_frames"), T.check_count(num_components, "num_components")
    if (num_frames, num_components) not in ((None, None), (N, K)):
        raise ValueError("the graph has %d frames of %d nodes, not %r of %r" % (N, K, num_frames, num_components))
    nnz = check_lists(nl, N, K)
    Hd = _check_entries(scores, "scores", nnz)
    _check_limits(0, nnz, Hd)
    dev = T.one_device([(scores, "scores")] + lists_tensors(nl))
    with torch.cuda.device(dev):
        nl = as_lists(nl, N, K)
        s = scores.reshape(Hd, nnz).contiguous()
        alpha = _Softmax.apply(s, nl) if differentiable(s) else _softmax(s, None, nl)
    return alpha.view(scores.shape)


def head_aggregate(values, nl, weight):
    """`values` float32 [N, C, K] ([C, K] when N = 1) summed over the neighbours of every node with one weight per head and entry, by
    rule 3 -> a new tensor of the same shape.  `weight`: float32 [Hd, nnz] (or [nnz], one head) with C % Hd == 0.  Differentiable with
    respect to both; one launch forward, one for each gradient, no host synchronisation."""
    N, Cc, K = check_map(values, "values")
    nnz = check_lists(nl, N, K)
    Hd = check_heads(_check_entries(weight, "weight", nnz), Cc)
    _check_limits(N * Cc * K, nnz, Hd)
    dev = T.one_device([(values, "values"), (weight, "weight")] + lists_tensors(nl))
    with torch.cuda.device(dev):
        nl = as_lists(nl, N, K)
        x, w = values.reshape(N, Cc, K).contiguous(), weight.reshape(Hd, nnz).contiguous()
        y = _Apply.apply(x, w, nl) if differentiable(x, w) else _apply(x, w, nl, False)
    return y.view(values.shape)


def graph_attention(query, key, values, nl, heads=1, scale=None, return_weights=False):
    """Multi-head attention of every node over its neighbours, by rule 5: `query` and `key` float32 [N, C, K] ([C, K] when N = 1) of
    one shape, `values` float32 with the same N and K and Cv channels, C and Cv multiples of `heads` -> [N, Cv, K] (the shape of
    `values`); with return_weights=True (y, alpha float32 [heads, nnz]).  scale: None (D ** -0.5, D = C / heads) or a finite number.
    The three launches of neighbour_dot, neighbour_softmax and head_aggregate, and their backwards."""
    N, Cc, K = check_map(query, "query")
    T.check_tensor(key, "key", (torch.float32,), "the shape of query, %s" % (tuple(query.shape),), lambda s: s == tuple(query.shape))
    Nv, Cv, Kv = check_map(values, "values")
    if (Nv, Kv) != (N, K) or values.dim() != query.dim():
        raise ValueError("values must have the frames and nodes of query, got shapes %s and %s" % (tuple(values.shape), tuple(query.shape)))
    nnz = check_lists(nl, N, K)
    Hd = check_heads(heads, Cc)
    check_heads(heads, Cv, "Cv")
    if scale is None:
        scale = float(Cc // Hd) ** -0.5
    elif isinstance(scale, bool) or not isinstance(scale, numbers.Real) or scale != scale or scale in (float("inf"), float("-inf")):
        raise ValueError("scale must be None or a finite number, got %r" % (scale,))
    _check_limits(N * max(Cc, Cv) * K, nnz, Hd)
    dev = T.one_device([(query, "query"), (key, "key"), (values, "values")] + lists_tensors(nl))
    with torch.cuda.device(dev):
        nl = as_lists(nl, N, K)
        alpha = neighbour_softmax(neighbour_dot(query * torch.tensor(float(scale), dtype=torch.float32).item(), key, nl, Hd), nl)
        y = head_aggregate(values, nl, alpha)
    return (y, alpha) if return_weights else y
