"""Exact k nearest neighbours in feature space, on torch tensors in HBM (csrc/knn.hip): for every node of every frame the k nearest nodes
of the same frame by squared Euclidean distance over the channels, as fixed-degree NeighbourLists that graph_aggregate and
graph_attention take as they are.  Neighbours by feature similarity, rebuilt every layer (EdgeConv / DGCNN, non-local attention), or
the nearest nodes of another frame (`other`), where superpixel_graph gives only the superpixels that touch.

    nl, dist = knn_graph(points, k)                                # points float32 [N, D, K] -> NeighbourLists, float32 [N * K * k]
    nl, dist = knn_graph(points, k, other=previous)                # candidates from another tensor of the same shape
    nl, dist = knn_graph(points, k, valid=counts > 0)              # empty superpixels are nobody's neighbour
    y = graph_aggregate(x, nl, reduce="max")                       # padding (index -1) contributes nothing anywhere

knn_graph(points, k, *, other=None, valid=None, loop=False) -> (nl, dist)

* `points`: float32 [N, D, K], or [D, K] for N = 1.  It may be any strided view; the layer makes it contiguous.  1 <= D <= 4096, K in
  check_count's range [1, 65534], 1 <= k <= 32, N * K * k < 2^31.
* `other`: None, or float32 of the same shape on the same GPU.  Candidates are then taken from `other` and queries from `points`: node j
  of frame f of `other` is a candidate for node i of the same frame of `points`.  `loop` is refused together with `other`: a node is
  not excluded from another tensor.
* `valid`: None, or torch.bool [N, K] ([K]).  It describes the nodes of both tensors.  An invalid node is nobody's neighbour, and an
  invalid node's own row is all padding.  The typical value is counts > 0, for empty superpixels that pool to 0.
* Distance of query i to candidate j is a left fold over c = 0 .. D - 1:
      acc = +0.0f;  t = x[f, c, i] - y[f, c, j];  acc = acc + t * t
  three separately rounded float32 operations per channel, with nothing fused.  Hence d(i, j) and d(j, i) are the same bits without
  `other`, d >= +0, and d is never -0.
* Candidates of row (f, i) are every valid j with a non-NaN d; without `other` and with loop=False, j != i as well.  +inf is an ordinary
  distance.  A NaN distance is not a candidate.
* Selection is the k smallest candidates in the total order (d, j), distance first and the smaller node number on ties.  They are
  written in that ascending order.  Rows with fewer than k candidates are padded behind the last one with index -1 and distance +inf.
  Nothing depends on the launch geometry, the tile size or how the candidates are split among threads: the same bits come out from
  run to run, and a numpy model written operation by operation (tests/knn_ref.py) gives the same integers and the same float bits.
* Result.  `nl` is a NeighbourLists (propagate.py) with edge=None, num_frames=N, num_components=K and
      offsets = arange(N * K + 1) * k, int64;  indices int32 [N * K * k];  rows = arange(N * K) repeated k times, int32
  `dist` is float32 [N * K * k], one value per entry: the `weight` shape of graph_aggregate.  It is not differentiable; the README
  shows the line that rebuilds it with gradients from neighbour_dot, |a|^2 + |b|^2 - 2 a.b.  Both outputs come from torch's caching
  allocator, on torch's current stream, with no host synchronisation and no workspace.
* Nothing flows to the graph.  There is no CPU fallback.

Out of scope: other metrics (the reference's L1 cell-window search is not reproduced, and get_knn_connectivity stays what it is); a
radius cut and approximate search; k > 32; float16 / bfloat16; gradients of the selection; symmetrising the lists (one torch.cat plus
neighbour_lists on a raw pair: README).

Every argument is checked before any device work (ValueError; two GPUs are refused first and a CPU tensor last).
This module imports torch; the package itself does not import it.
"""
import numbers

import torch

from . import _binding as B, _tensors as T
from .propagate import NeighbourLists

__all__ = ["knn_graph"]

_ENTRY = ("fslic_hip_knn_graph", "nearest-neighbour entry point")
MAX_K = 32
MAX_CHANNELS = 4096
_LIMIT = 1 << 31


def fixed_degree_lists(indices, N, K, k):
    """The NeighbourLists of `indices` int32 [N * K * k], k entries a row: plain torch on the tensor's device."""
    dev = indices.device
    offsets = torch.arange(N * K + 1, dtype=torch.int64, device=dev) * k
    rows = torch.arange(N * K, dtype=torch.int32, device=dev).repeat_interleave(k)
    return NeighbourLists(offsets, indices, None, rows, N, K)


def knn_graph(points, k, *, other=None, valid=None, loop=False):
    """The k nearest nodes of every node among the nodes of its frame, by the module's text: `points` float32 [N, D, K] ([D, K] when
    N = 1) -> (NeighbourLists with k entries a row, float32 [N * K * k] squared distances); padding is index -1 at distance +inf.
    One launch, no host synchronisation."""
    T.check_float_map(points, (2, 3), "points", "[D, K] or [N, D, K]")
    batched = points.dim() == 3
    N = int(points.shape[0]) if batched else 1
    D, K = (int(v) for v in points.shape[-2:])
    T.check_count(K, "K, the last dimension of points,")
    if D > MAX_CHANNELS:
        raise ValueError("D, the channels of points, must be in [1, %d], got %d" % (MAX_CHANNELS, D))
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= MAX_K:
        raise ValueError("k must be an integer in [1, %d], got %r" % (MAX_K, k))
    k = int(k)
    if other is not None:
        T.check_tensor(other, "other", (torch.float32,), "the shape of points, %s" % (tuple(points.shape),), lambda s: s == tuple(points.shape))
        if loop:
            raise ValueError("loop goes with points alone: a node is not excluded from another tensor")
    if valid is not None:
        shape = (N, K) if batched else (K,)
        T.check_tensor(valid, "valid", (torch.bool,), "%s, one per node" % (list(shape),), lambda s: s == shape)
    if N * K * k >= _LIMIT:
        raise ValueError("N * K * k must be below 2^31")
    dev = T.one_device([(points, "points"), (other, "other"), (valid, "valid")])

    lib = T.library(*_ENTRY)
    with torch.cuda.device(dev):
        x = points.reshape(N, D, K).contiguous()
        y = other.reshape(N, D, K).contiguous() if other is not None and other is not points else None
        v = valid.reshape(N, K).contiguous() if valid is not None else None
        indices = torch.empty(N * K * k, dtype=torch.int32, device=dev)
        dist = torch.empty(N * K * k, dtype=torch.float32, device=dev)
        # (`other is points` is the same candidates with nothing left out: the kernel's form without `other` and with the loop)
        B._check(lib.fslic_hip_knn_graph(dev.index, T.stream(dev), N, D, K, k, int(bool(loop) or other is points), x.data_ptr(), T.ptr(y), T.ptr(v),
                                         indices.data_ptr(), dist.data_ptr()))
        return fixed_degree_lists(indices, N, K, k), dist
