"""Pixels over the neighbours of their superpixels, on torch tensors in HBM (csrc/pixel.hip): every pixel looks at its own superpixel
and at that superpixel's neighbours in a NeighbourLists -- S *slots* a pixel -- and the slots are scored from pixel and node features,
normalised, and used to mix node values back to the pixels (a learned, edge-aware decoder in place of superpixel_unpool) or to scatter
pixel features to the nodes (SSN's centre update, over Slic's labels and any graph), each with exact, reproducible gradients.

    nl = neighbour_lists(graph)                                    # propagate.py; or knn_graph's lists, or a merged map's graph
    s = pixel_dot(a, b, labels, nl, slots=9, heads=Hd)             # a float32 [N, C, H, W], b float32 [N, C, K] -> [N, Hd, S, H, W]
    alpha = pixel_softmax(s, labels, nl)                           # over the non-empty slots of every pixel and head
    y = pixel_mix(values, alpha, labels, nl)                       # values [N, Cv, K] -> [N, Cv, H, W]
    v = pixel_scatter(x, alpha, labels, nl, K)                     # x [N, C, H, W] -> [N, C, K]
    y = pixel_attention(query, key, values, labels, nl, slots=9, heads=Hd)
    j = pixel_slots(labels, nl, slots=9)                           # int32 [N, S, H, W]: the node of every slot, -1 where empty

The terms.  `labels` is what superpixel_pool accepts: [N, H, W] ([H, W] with unbatched inputs), int16 (numpy or torch; -1 is "no
label"), int32 or int64; a map that is not on the GPU yet is uploaded.  `nl` is a NeighbourLists over the N * K rows (frame, node); a
SuperpixelGraph or a raw pair (offsets int64 [N * K + 1], indices int32 [nnz]) is accepted as in entry_reduce, a raw pair with
num_components = K where no node tensor names K.  `slots` = S is an integer in [1, 32].  For pixel (f, y, x) with i = labels[f, y, x]:
if i is outside [0, K) every slot of the pixel is *empty*; otherwise slot 0 names node i itself, and slot s >= 1 names entry
p = lo + s - 1 of row (f, i), [lo, hi) the row's bounds clamped into [0, nnz] (an end before its start is an empty row): the slot is
non-empty iff p < hi and 0 <= indices[p] < K, and its node is j = indices[p].  A row longer than S - 1 entries is cut after its first
S - 1: the lowest-numbered neighbours on the adjacency graph, the nearest on knn_graph's lists.  Empty slots may lie between non-empty
ones (knn_graph's padding -1); they take part in nothing.  A per-slot tensor is float32 [N, Hd, S, H, W] ([Hd, S, H, W] unbatched);
Hd is the number of heads, D = C / Hd the channels of a head (C % Hd != 0 is refused) and h(c) = c // D the head of channel c.  Every
product, sum, difference and division in rules 1 - 3 is one separately rounded float32 operation, nothing fused, the division
correctly rounded.  The rules:

1. pixel_dot(a, b, labels, nl, slots, heads).  out[f, h, s, y, x] is the left fold over c = h D .. h D + D - 1:
       acc = +0.0f;  acc = acc + (a[f, c, y, x] * b[f, c, j])          j the slot's node
   An empty slot gives +0.0.
2. pixel_softmax(scores, labels, nl).  Per pixel and head, over the non-empty slots, as neighbour_softmax is over a row's valid
   entries: m = the maximum score; e_s = expf(score_s - m), expf the library's crf_expf (csrc/crf.h: glibc's expf bit for bit);
   Z = the left fold of e_s in ascending s from +0.0; alpha_s = e_s / Z.  Empty slots get +0.0.  A labelled pixel always has slot 0, so
   Z >= 1; a pixel without a label is all +0.0.  NaN or +inf leaves the pixel unspecified.
3. pixel_mix(values, weight, labels, nl).  out[f, c, y, x] is the left fold over the non-empty slots in ascending s:
       acc = +0.0f;  acc = acc + (weight[f, h(c), s, y, x] * values[f, c, j])
4. pixel_scatter(x, weight, labels, nl, num_components).  out[f, c, j] is the sum of weight[f, h(c), s, y, x] * x[f, c, y, x] over
   the pixels and slots that name node j, by the contract of superpixel_pool's sum extended by the slot: there is one float32
   *partial* per tile of 16 x 64 pixels (aligned at the frame's origin), label i, slot s and channel c -- the sum, in a fixed order
   of the kernel's, of the products of the tile's pixels of label i, each product rounded once; every partial is truncated towards
   zero to a multiple of 2^-96; the partials whose slot names node j are added exactly in fixed point (csrc/fixsum.h) and the total
   is rounded once to float32, ties to even.  A zero total is +0.0; non-finite input leaves the entry unspecified.  No float
   atomics: the bits are the same from run to run and at every batch position.  With S = 1 and unit weights these are the bits of
   superpixel_pool(x, labels, K, reduce="sum").
5. Gradients.  Each function is a torch.autograd.Function with a once_differentiable backward; nothing flows to labels or lists.
   The three families are each other's gradients:
       pixel_dot       grad_a = pixel_mix(b, g)                 grad_b = pixel_scatter(a, g)
       pixel_mix       grad_values = pixel_scatter(g, weight)   grad_weight = pixel_dot(g, values)
       pixel_scatter   grad_x = pixel_mix(g, weight)            grad_weight = pixel_dot(x, g)
   pixel_softmax, from the alpha it returned: t = the left fold of alpha_s * g_s over the non-empty slots; grad_s = alpha_s *
   (g_s - t), and +0.0 on empty slots.  A numpy model written operation by operation (tests/pixels_ref.py) reproduces dot, mix,
   softmax and every gradient that is one of those bit for bit, and the scatter wherever no partial rounds.
6. pixel_attention(query, key, values, labels, nl, slots, heads, scale) is
       pixel_mix(values, pixel_softmax(pixel_dot(query * float32(scale), key, labels, nl, slots, heads), labels, nl), labels, nl)
   scale = D ** -0.5 unless given, the multiplication plain torch; `values` may have a channel count Cv of its own (Cv % Hd == 0).
   It adds no kernel: its bits and gradients are those of the composition.
7. pixel_slots(labels, nl, slots) is the node of every slot as int32 [N, S, H, W], -1 where the slot is empty: plain torch on the
   device of the lists, for masks and for dense restatements; not a hot path.

Nothing of a map or a raw pair is trusted on the device, by csrc/lists.h's rule: nothing a kernel reads from device memory becomes an
address before it is checked.  Garbage lists give unspecified values, never an access out of bounds.

The cost of this design is the dense per-slot tensor: 4 N Hd S H W bytes for the scores and again for alpha (8 frames of 1280 x 720,
9 slots, 4 heads: 1.06 GB each), where the torch composition holds [N, C, S, H, W].  Out of scope: float16 / bfloat16, one fused
attention kernel, more than 32 slots, gradients to labels or lists, a node attending over its pixels, a pinned in-tile order of the
scatter (it is the kernel's, as in pooling).

Every argument is checked before any device work (ValueError; two GPUs are refused first and a CPU tensor last).  Limits: K in
[1, 65534]; N * C * H * W, N * Hd * S * H * W, N * C * K and nnz below 2^31.  Every call runs on torch's current stream of the tensors'
GPU, takes its results and scratch from torch's caching allocator and never synchronises the host.  There is no CPU fallback.
This module imports torch; the package itself does not import it.
"""
import numbers

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _binding as B, _tensors as T
from .propagate import LIMIT, NeighbourLists, as_lists, check_heads, check_lists, differentiable, lists_tensors
from .rag import SuperpixelGraph, check_graph

__all__ = ["pixel_dot", "pixel_softmax", "pixel_mix", "pixel_scatter", "pixel_attention", "pixel_slots"]

_ENTRY = ("fslic_hip_pixel_scatter", "pixel entry points")
MAX_SLOTS = 32
_LIMIT_TEXT = "N * C * H * W, N * heads * slots * H * W, N * C * K and the number of neighbour entries must be below 2^31"


# ---- argument checks: all of them run before any device work ----
def _check_slots(slots):
    if isinstance(slots, bool) or not isinstance(slots, numbers.Integral) or not 1 <= slots <= MAX_SLOTS:
        raise ValueError("slots must be an integer in [1, %d], got %r" % (MAX_SLOTS, slots))
    return int(slots)


def _check_pixels(t, what):
    """-> (batched, N, C, H, W) of a float32 [N, C, H, W] or [C, H, W] tensor."""
    T.check_float_map(t, (3, 4), what, "[C, H, W] or [N, C, H, W]")
    batched = t.dim() == 4
    Cc, H, W = (int(v) for v in t.shape[-3:])
    return batched, (int(t.shape[0]) if batched else 1), Cc, H, W


def _check_nodes(t, what, batched, N, Cc=None, K=None):
    """-> (C, K) of a float32 [N, C, K] tensor ([C, K] unbatched) with the frames, and where given the channels and nodes, named."""
    want = "[N, C, K] with N = %d" % N if batched else "[C, K]"
    T.check_float_map(t, (3,) if batched else (2,), what, want)
    if batched and int(t.shape[0]) != N:
        raise ValueError("%s must be %s, got shape %s" % (what, want, tuple(t.shape)))
    c, k = (int(v) for v in t.shape[-2:])
    if Cc is not None and c != Cc:
        raise ValueError("%s must have %d channels, got shape %s" % (what, Cc, tuple(t.shape)))
    if K is not None and k != K:
        raise ValueError("%s must have K = %d nodes, got shape %s" % (what, K, tuple(t.shape)))
    T.check_count(k, "K, the last dimension of %s," % what)
    return c, k


def _check_per_slot(t, what, batched=None, N=None, H=None, W=None):
    """-> (batched, N, Hd, S, H, W) of a per-slot tensor float32 [N, Hd, S, H, W] or [Hd, S, H, W]; the frames that are given must match."""
    ranks = (4, 5) if batched is None else (5,) if batched else (4,)
    T.check_float_map(t, ranks, what, "[Hd, S, H, W] or [N, Hd, S, H, W]" if batched is None else "[N, Hd, S, H, W]" if batched else "[Hd, S, H, W]")
    b = t.dim() == 5
    n = int(t.shape[0]) if b else 1
    Hd, s, h, w = (int(v) for v in t.shape[-4:])
    if N is not None and (n, h, w) != (N, H, W):
        raise ValueError("%s must be one value per head, slot and pixel of the %d frames of %d x %d, got shape %s" % (what, N, H, W, tuple(t.shape)))
    _check_slots(s)
    return b, n, Hd, s, h, w


def _check_labels(labels, batched, N, H, W):
    T.check_label_map(labels, "labels")
    shape = (N, H, W) if batched else (H, W)
    if tuple(labels.shape) != shape:
        raise ValueError("labels must have shape %s to match the pixels, got %s" % (shape, tuple(labels.shape)))


def _graph_size(nl, N, num_components, K=None):
    """-> (K, nnz) of the lists for N frames; K: the nodes a node tensor names, or None where only the lists or num_components do."""
    if num_components is not None:
        num_components = T.check_count(num_components, "num_components")
        if K is not None and K != num_components:
            raise ValueError("the node tensors have K = %d nodes, num_components is %d" % (K, num_components))
        K = num_components
    if isinstance(nl, NeighbourLists):
        K = nl.num_components if K is None else K
    elif isinstance(nl, SuperpixelGraph):
        K = check_graph(nl)[1] if K is None else K
    elif K is None:
        raise ValueError("a raw pair (offsets, indices) needs num_components")
    return K, check_lists(nl, N, K)


def _check_limits(N, C, H, W, K, Hd, S, nnz):
    if N * C * H * W >= LIMIT or N * Hd * S * H * W >= LIMIT or N * C * K >= LIMIT or nnz >= LIMIT:
        raise ValueError(_LIMIT_TEXT)


def _label_tensors(labels):
    """A map that is on a GPU names it; a numpy or CPU map is uploaded."""
    return [(labels, "labels")] if isinstance(labels, torch.Tensor) and labels.device.type == "cuda" else []


# ---- the launches, on contiguous batched tensors of one GPU ----
class _Geom(object):
    """What every launch shares: the label map on the GPU, its type code, the NeighbourLists and the sizes."""

    def __init__(self, labels, nl, dev, batched, N, H, W, K, S):
        self.lab, self.ltype = T.labels_on(labels, dev, batched)
        self.nl, self.dev = as_lists(nl, N, K), dev
        self.N, self.H, self.W, self.K, self.S = N, H, W, K, S
        self.nnz = int(self.nl.indices.shape[0])

    def head(self, Cc, Hd):
        return (self.dev.index, T.stream(self.dev), self.N, Cc, self.H, self.W, self.K, self.S, Hd, self.nnz, self.ltype, self.lab.data_ptr(),
                self.nl.offsets.data_ptr(), T.ptr(self.nl.indices, self.nnz))


def _dot(g, a, b, Hd):
    """-> float32 [N, Hd, S, H, W] of a float32 [N, C, H, W] and b float32 [N, C, K]: rule 1."""
    lib = T.library(*_ENTRY)
    with torch.cuda.device(g.dev):
        out = torch.empty((g.N, Hd, g.S, g.H, g.W), dtype=torch.float32, device=g.dev)
        B._check(lib.fslic_hip_pixel_dot(*g.head(int(a.shape[1]), Hd), a.data_ptr(), b.data_ptr(), out.data_ptr()))
    return out


def _mix(g, values, weight):
    """-> float32 [N, C, H, W] of values float32 [N, C, K] and weight float32 [N, Hd, S, H, W]: rule 3."""
    lib = T.library(*_ENTRY)
    with torch.cuda.device(g.dev):
        out = torch.empty((g.N, int(values.shape[1]), g.H, g.W), dtype=torch.float32, device=g.dev)
        B._check(lib.fslic_hip_pixel_mix(*g.head(int(values.shape[1]), int(weight.shape[1])), values.data_ptr(), weight.data_ptr(), out.data_ptr()))
    return out


def _softmax(g, t, grad):
    """t float32 [N, Hd, S, H, W] -> its softmax (grad None), or the gradient of the scores from t = alpha and grad: rules 2 and 5."""
    lib, Hd = T.library(*_ENTRY), int(t.shape[1])
    with torch.cuda.device(g.dev):
        out = torch.empty_like(t)
        B._check(lib.fslic_hip_pixel_softmax(*g.head(Hd, Hd), int(grad is not None), t.data_ptr(), T.ptr(grad), out.data_ptr()))
    return out


def _scatter(g, x, weight):
    """-> float32 [N, C, K] of x float32 [N, C, H, W] and weight float32 [N, Hd, S, H, W]: rule 4."""
    lib, Cc = T.library(*_ENTRY), int(x.shape[1])
    with torch.cuda.device(g.dev):
        out = torch.empty((g.N, Cc, g.K), dtype=torch.float32, device=g.dev)
        ws, nbytes = T.scratch(g.dev, lib.fslic_hip_pixel_scatter_workspace_size, g.N, Cc, g.K)
        B._check(lib.fslic_hip_pixel_scatter(*g.head(Cc, int(weight.shape[1])), x.data_ptr(), weight.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes))
    return out


class _Dot(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, g, Hd):
        ctx.save_for_backward(a, b)
        ctx.g = g
        return _dot(g, a, b, Hd)

    @staticmethod
    @once_differentiable
    def backward(ctx, gs):
        a, b = ctx.saved_tensors
        gs = gs.contiguous()
        return (_mix(ctx.g, b, gs) if ctx.needs_input_grad[0] else None, _scatter(ctx.g, a, gs) if ctx.needs_input_grad[1] else None, None, None)


class _Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, g):
        alpha = _softmax(g, s, None)
        ctx.save_for_backward(alpha)
        ctx.g = g
        return alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        alpha, = ctx.saved_tensors
        return _softmax(ctx.g, alpha, grad.contiguous()), None


class _Mix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, weight, g):
        ctx.save_for_backward(values, weight)
        ctx.g = g
        return _mix(g, values, weight)

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        values, weight = ctx.saved_tensors
        go = go.contiguous()
        return (_scatter(ctx.g, go, weight) if ctx.needs_input_grad[0] else None,
                _dot(ctx.g, go, values, int(weight.shape[1])) if ctx.needs_input_grad[1] else None, None)


class _Scatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, g):
        ctx.save_for_backward(x, weight)
        ctx.g = g
        return _scatter(g, x, weight)

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        x, weight = ctx.saved_tensors
        go = go.contiguous()
        return (_mix(ctx.g, go, weight) if ctx.needs_input_grad[0] else None,
                _dot(ctx.g, x, go, int(weight.shape[1])) if ctx.needs_input_grad[1] else None, None)


# ---- the public functions ----
def pixel_slots(labels, nl, slots, *, num_components=None):
    """The node of every slot of every pixel, by the terms of the module's text: int32 [N, S, H, W] ([S, H, W] for an [H, W] map),
    -1 where the slot is empty.  Plain torch on the device of the lists (a CPU graph gives a CPU result); a raw pair needs
    num_components = K."""
    T.check_label_map(labels, "labels")
    batched = labels.ndim == 3
    N = int(labels.shape[0]) if batched else 1
    S = _check_slots(slots)
    K, nnz = _graph_size(nl, N, num_components)
    nl = as_lists(nl, N, K)
    offsets, indices, dev = nl.offsets, nl.indices, nl.offsets.device
    if isinstance(labels, np.ndarray):
        labels = torch.from_numpy(np.ascontiguousarray(labels).view(np.int16) if labels.dtype == np.uint16 else np.ascontiguousarray(labels))
    i = labels.to(device=dev, dtype=torch.int64).reshape(N, 1, *labels.shape[-2:])
    has = (i >= 0) & (i < K)
    row = torch.arange(N, dtype=torch.int64, device=dev).view(N, 1, 1, 1) * K + torch.where(has, i, torch.zeros_like(i))
    lo, hi = offsets[row].clamp(0, nnz), offsets[row + 1].clamp(0, nnz)
    out = torch.full((N, S) + tuple(i.shape[-2:]), -1, dtype=torch.int32, device=dev)
    out[:, :1] = torch.where(has, i, torch.full_like(i, -1)).to(torch.int32)
    if S > 1 and nnz > 0:
        p = lo + torch.arange(S - 1, dtype=torch.int64, device=dev).view(1, S - 1, 1, 1)
        j = indices[p.clamp(max=nnz - 1)].to(torch.int64)
        ok = has & (p < hi) & (j >= 0) & (j < K)
        out[:, 1:] = torch.where(ok, j, torch.full_like(j, -1)).to(torch.int32)
    return out if batched else out[0]


def pixel_dot(a, b, labels, nl, slots, heads=1):
    """The score of every slot of every pixel, by rule 1 of the module's text: `a` float32 [N, C, H, W] ([C, H, W] unbatched) read
    at the pixel and `b` float32 [N, C, K] ([C, K]) read at the slot's node -> float32 [N, heads, slots, H, W].  Differentiable with
    respect to both; one launch forward, a mix and a scatter backward, no host synchronisation."""
    batched, N, Cc, H, W = _check_pixels(a, "a")
    _, K = _check_nodes(b, "b", batched, N, Cc)
    _check_labels(labels, batched, N, H, W)
    K, nnz = _graph_size(nl, N, None, K)
    S, Hd = _check_slots(slots), check_heads(heads, Cc)
    _check_limits(N, Cc, H, W, K, Hd, S, nnz)
    dev = T.one_device([(a, "a"), (b, "b")] + _label_tensors(labels) + lists_tensors(nl))
    with torch.cuda.device(dev):
        g = _Geom(labels, nl, dev, batched, N, H, W, K, S)
        a4, b3 = T.batch_of(a, batched), T.batch_of(b, batched)
        out = _Dot.apply(a4, b3, g, Hd) if differentiable(a4, b3) else _dot(g, a4, b3, Hd)
    return out if batched else out[0]


def pixel_softmax(scores, labels, nl, *, num_components=None):
    """The softmax of `scores` (float32 [N, Hd, S, H, W], or [Hd, S, H, W]) over the non-empty slots of every pixel, per head, by rule
    2 -> the shape of `scores`.  A raw pair in place of `nl` needs num_components = K.  Differentiable; one launch forward and one
    backward, no host synchronisation."""
    batched, N, Hd, S, H, W = _check_per_slot(scores, "scores")
    _check_labels(labels, batched, N, H, W)
    K, nnz = _graph_size(nl, N, num_components)
    _check_limits(N, Hd, H, W, K, Hd, S, nnz)
    dev = T.one_device([(scores, "scores")] + _label_tensors(labels) + lists_tensors(nl))
    with torch.cuda.device(dev):
        g = _Geom(labels, nl, dev, batched, N, H, W, K, S)
        s5 = T.batch_of(scores, batched)
        alpha = _Softmax.apply(s5, g) if differentiable(s5) else _softmax(g, s5, None)
    return alpha if batched else alpha[0]


def pixel_mix(values, weight, labels, nl):
    """Node values mixed to the pixels with one weight per head and slot, by rule 3: `values` float32 [N, Cv, K] ([Cv, K] unbatched),
    `weight` float32 [N, Hd, S, H, W] with Cv % Hd == 0 -> float32 [N, Cv, H, W].  Differentiable with respect to both; one launch
    forward, a scatter and a dot backward, no host synchronisation."""
    batched, N, Hd, S, H, W = _check_per_slot(weight, "weight")
    Cv, K = _check_nodes(values, "values", batched, N)
    _check_labels(labels, batched, N, H, W)
    K, nnz = _graph_size(nl, N, None, K)
    check_heads(Hd, Cv, "Cv")
    _check_limits(N, Cv, H, W, K, Hd, S, nnz)
    dev = T.one_device([(values, "values"), (weight, "weight")] + _label_tensors(labels) + lists_tensors(nl))
    with torch.cuda.device(dev):
        g = _Geom(labels, nl, dev, batched, N, H, W, K, S)
        v3, w5 = T.batch_of(values, batched), T.batch_of(weight, batched)
        out = _Mix.apply(v3, w5, g) if differentiable(v3, w5) else _mix(g, v3, w5)
    return out if batched else out[0]


def pixel_scatter(x, weight, labels, nl, num_components):
    """Pixel features summed into the nodes their slots name, with one weight per head and slot, by rule 4: `x` float32
    [N, C, H, W] ([C, H, W] unbatched), `weight` float32 [N, Hd, S, H, W] with C % Hd == 0 -> float32 [N, C, K], K = num_components.
    Exact and reproducible (no float atomics).  Differentiable with respect to both; a clear and two launches forward, a mix and a
    dot backward, no host synchronisation."""
    batched, N, Cc, H, W = _check_pixels(x, "x")
    _check_per_slot(weight, "weight", batched, N, H, W)
    Hd, S = int(weight.shape[-4]), int(weight.shape[-3])
    _check_labels(labels, batched, N, H, W)
    K, nnz = _graph_size(nl, N, T.check_count(num_components, "num_components"))
    check_heads(Hd, Cc)
    _check_limits(N, Cc, H, W, K, Hd, S, nnz)
    dev = T.one_device([(x, "x"), (weight, "weight")] + _label_tensors(labels) + lists_tensors(nl))
    with torch.cuda.device(dev):
        g = _Geom(labels, nl, dev, batched, N, H, W, K, S)
        x4, w5 = T.batch_of(x, batched), T.batch_of(weight, batched)
        out = _Scatter.apply(x4, w5, g) if differentiable(x4, w5) else _scatter(g, x4, w5)
    return out if batched else out[0]


def pixel_attention(query, key, values, labels, nl, slots, heads=1, scale=None, return_weights=False):
    """Multi-head attention of every pixel over its slots, by rule 6: `query` float32 [N, C, H, W] ([C, H, W] unbatched), `key`
    float32 [N, C, K], `values` float32 [N, Cv, K], C and Cv multiples of `heads` -> [N, Cv, H, W]; with return_weights=True
    (y, alpha float32 [N, heads, slots, H, W]).  scale: None (D ** -0.5, D = C / heads) or a finite number.  The three launches of
    pixel_dot, pixel_softmax and pixel_mix, and their backwards."""
    batched, N, Cc, H, W = _check_pixels(query, "query")
    _, K = _check_nodes(key, "key", batched, N, Cc)
    Cv, _ = _check_nodes(values, "values", batched, N, None, K)
    _check_labels(labels, batched, N, H, W)
    K, nnz = _graph_size(nl, N, None, K)
    S, Hd = _check_slots(slots), check_heads(heads, Cc)
    check_heads(heads, Cv, "Cv")
    if scale is None:
        scale = float(Cc // Hd) ** -0.5
    elif isinstance(scale, bool) or not isinstance(scale, numbers.Real) or scale != scale or scale in (float("inf"), float("-inf")):
        raise ValueError("scale must be None or a finite number, got %r" % (scale,))
    _check_limits(N, max(Cc, Cv), H, W, K, Hd, S, nnz)
    dev = T.one_device([(query, "query"), (key, "key"), (values, "values")] + _label_tensors(labels) + lists_tensors(nl))
    with torch.cuda.device(dev):
        nl = as_lists(nl, N, K)
        labels = T.labels_on(labels, dev, True)[0]                             # uploaded once for the three calls
        alpha = pixel_softmax(pixel_dot(query * torch.tensor(float(scale), dtype=torch.float32).item(), key, labels, nl, S, Hd), labels, nl)
        y = pixel_mix(values, alpha, labels, nl)
    return (y, alpha) if return_weights else y
