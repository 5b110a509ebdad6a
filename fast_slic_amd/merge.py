"""Merging superpixels along the region adjacency graph, on torch tensors in HBM (csrc/merge.hip): the parallel (Boruvka) round.

    join       = best_neighbour_edges(graph, weight, threshold=None)   # bool [E]
    mapping, n = merge_components(graph, join, members=None)           # int32 [N, K], int32 [N]
    coarse     = merge_labels(labels, mapping)                         # int32, of the labels' shape
    graph2     = contract_graph(graph, mapping, num_components)        # a SuperpixelGraph of the groups, without a pixel pass
    total      = compose_mappings(first, then)                         # int32 [N, K]: then[f, first[f, v]]

`graph` is a SuperpixelGraph (rag.py): N frames, K = num_components nodes a frame, E edges, `offsets`.  The edges of frame f are
[offsets[f], offsets[f + 1]), sorted by (lo, hi); the *position* of an edge is its index minus offsets[f].  The rules:

1. Best edges.  `weight` is float32 [E], values >= 0; -0.0 counts as +0.0; a NaN or negative value leaves the result unspecified.
   An edge is *eligible* if `threshold` is None or weight[e] < threshold (strictly).  A node's *best edge* is the eligible edge
   incident to it with the smallest (weight, position) pair: weight first, position breaks ties; a node with no eligible edge has
   none.  join[e] is true exactly when e is the best edge of at least one of its two endpoints.
2. Components.  A node is *present* if `members` is None or its count is > 0; an edge with an absent endpoint is ignored, whatever
   `join` says.  Groups are the connected components of the present nodes of a frame under the edges with `join` true.  A group's
   leader is its smallest node number; groups are numbered 0, 1, 2, ... in ascending leader order.  mapping[f, v] is the number of
   v's group, -1 for an absent node; n[f] is the number of groups, and the labels 0 .. n[f] - 1 all occur in mapping[f].
3. Labels.  out = mapping[f, l] for a label l in [0, K), and -1 for any other label and where the mapping is -1.
4. Contraction.  Every edge (a, b) of frame f becomes (a', b') = (mapping[f, a], mapping[f, b]); it is dropped if either is outside
   [0, K2) or a' == b'; otherwise its boundary and its contrast row are added to the pair (min, max).  For every map, mapping and
   bound K2 = num_components:
       contract_graph(superpixel_graph(labels, K, c, image), mapping, K2) == superpixel_graph(merge_labels(labels, mapping), K2, c, image)
   field for field (edge_index, boundary, contrast, offsets).  K2 is the caller's bound on n, passed on without reading n back.

Out of scope: the sequential priority-queue order of skimage's merge_hierarchical (the parallel round above is the semantics);
gradients; 8- versus 4-connectivity, which is the graph's business.  Reproducible float sums of group features, the weights from
them and the whole loop are regions.py's (group_sums, edge_weights, merge_hierarchical); equality of those sums with a re-pool from
the pixels holds for counts and exactly representable sums only, since pooled node sums are already rounded.

The work runs on torch's current stream of the graph's (the map's) device and scratch memory comes from torch's caching allocator;
results live on that GPU.  best_neighbour_edges, merge_components, merge_labels and compose_mappings do not synchronise the host;
contract_graph synchronises once for the number of edges, and again only when its pair table has to grow (as superpixel_graph).
There is no CPU fallback.  All of it is integer arithmetic or comparison: results are exact and identical from run to run.
This module imports torch; the package itself does not import it.
"""
import numbers

import torch

from . import _binding as B, _pairtable as PT, _tensors as T
from .rag import SuperpixelGraph, check_graph, first_capacity, graph_device, graph_edges

__all__ = ["best_neighbour_edges", "merge_components", "merge_labels", "contract_graph", "compose_mappings"]

_ENTRY = ("fslic_hip_merge_components", "graph merging entry points")


# ---- argument checks: all of them run before any device work ----
def _check_mapping(mapping, N, K=None, what="mapping"):
    T.check_tensor(mapping, what, (torch.int32,), "[N, K] with N = %d%s" % (N, "" if K is None else " and K = %d" % K),
                   lambda s: len(s) == 2 and s[0] == N and s[1] >= 1 and (K is None or s[1] == K))


def best_neighbour_edges(graph, weight, threshold=None):
    """join bool [E]: true where the edge is the best edge of at least one of its endpoints (rule 1 of the module's text).  `weight`
    float32 [E] on the graph's GPU; `threshold` None or a Python number: only edges with weight < threshold are eligible."""
    N, K, E, _ = check_graph(graph)
    T.check_tensor(weight, "weight", (torch.float32,), "[E] with E = %d, one per edge of the graph" % E, lambda s: s == (E,))
    if threshold is not None and (isinstance(threshold, bool) or not isinstance(threshold, numbers.Real)):
        raise ValueError("threshold must be None or a number, got %r" % (threshold,))
    dev = graph_device(graph, ((weight, "weight"),))

    lib = T.library(*_ENTRY)
    with torch.cuda.device(dev):
        join = torch.empty(E, dtype=torch.bool, device=dev)
        if E == 0:
            return join
        ei, offsets = graph_edges(graph)
        w = weight.contiguous()
        ws, nbytes = T.scratch(dev, lib.fslic_hip_merge_best_workspace_size, N, K)
        B._check(lib.fslic_hip_merge_best_edges(dev.index, T.stream(dev), N, K, E, ei.data_ptr(), offsets.data_ptr(), w.data_ptr(),
                                                0 if threshold is None else 1, 0.0 if threshold is None else float(threshold),
                                                join.data_ptr(), ws.data_ptr(), nbytes))
    return join


def merge_components(graph, join, members=None):
    """(mapping int32 [N, K], n int32 [N]): the groups of the present nodes under the edges with `join` true, numbered by their
    smallest node (rule 2 of the module's text).  `join` bool [E]; `members` None or int32 / int64 [N, K] ([K] allowed when N = 1),
    superpixel_pool's counts: a node without members is absent.  The same six launches whatever the graph, no host synchronisation."""
    N, K, E, _ = check_graph(graph)
    T.check_tensor(join, "join", (torch.bool,), "[E] with E = %d, one per edge of the graph" % E, lambda s: s == (E,))
    if members is not None:
        T.check_tensor(members, "members", tuple(T.MEMBER_TYPE), "[N, K] = [%d, %d]%s" % (N, K, " or [K]" if N == 1 else ""),
                       lambda s: s == (N, K) or (N == 1 and s == (K,)))
    dev = graph_device(graph, ((join, "join"), (members, "members")))

    lib = T.library(*_ENTRY)
    with torch.cuda.device(dev):
        ei, offsets = graph_edges(graph)
        jn = join.contiguous()
        mem = members.contiguous() if members is not None else None
        mapping = torch.empty((N, K), dtype=torch.int32, device=dev)
        n = torch.empty((N,), dtype=torch.int32, device=dev)
        ws, nbytes = T.scratch(dev, lib.fslic_hip_merge_components_workspace_size, N, K)
        B._check(lib.fslic_hip_merge_components(dev.index, T.stream(dev), N, K, E, T.ptr(ei, E), offsets.data_ptr(), T.ptr(jn, E),
                                                T.ptr(mem), T.MEMBER_TYPE[mem.dtype] if mem is not None else 0, mapping.data_ptr(),
                                                n.data_ptr(), ws.data_ptr(), nbytes))
    return mapping, n


def merge_labels(labels, mapping, *, device=None):
    """out int32, of the labels' shape: mapping[f, l] for a label l in [0, K), -1 for any other label and where the mapping is -1
    (rule 3).  `labels` [H, W] (N = 1) or [N, H, W]; int16, int32 or int64; numpy (uploaded) or torch.  `mapping` int32 [N, K] on
    the GPU.  One pass over the pixels, N * H * W < 2^31, no host synchronisation."""
    T.check_label_map(labels, "labels")
    N = int(labels.shape[0]) if labels.ndim == 3 else 1
    H, W = (int(v) for v in labels.shape[-2:])
    if N * H * W >= 1 << 31:
        raise ValueError("N * H * W must be below 2^31, got shape %s" % (tuple(labels.shape),))
    _check_mapping(mapping, N)
    K = T.check_count(int(mapping.shape[1]), "num_components")
    dev = T.one_device(((labels, "labels"), (mapping, "mapping")), device)

    lib = T.library(*_ENTRY)
    with torch.cuda.device(dev):
        lab, ltype = T.labels_on(labels, dev)
        mp = mapping.contiguous()
        out = torch.empty(tuple(labels.shape), dtype=torch.int32, device=dev)
        B._check(lib.fslic_hip_merge_labels(dev.index, T.stream(dev), N, H, W, K, lab.data_ptr(), ltype, mp.data_ptr(), out.data_ptr()))
    return out


def contract_capacity_limit(K2, E):
    """Slots per frame that hold any contraction at half load: no more distinct pairs than label pairs or edges."""
    pairs = min(K2 * (K2 - 1) // 2, E)
    return min(PT.MAX_CAPACITY, max(first_capacity(K2), PT.pow2_at_least(2 * pairs)))


def contract_graph(graph, mapping, num_components, *, _start_capacity=None):
    """The SuperpixelGraph of the groups (rule 4): every edge's boundary and contrast row added to the pair of its endpoints' groups,
    sorted exactly as superpixel_graph sorts them, with num_components = K2.  `mapping` int32 [N, K].  The pair table of the graph
    holds the sums, and the graph's compact pass reads them out: one host synchronisation for the number of edges, more only when
    the table has to grow (the first has a power of two >= 8 K2 slots per frame).  `_start_capacity` (testing) sets the first
    table's slots per frame."""
    N, K, E, Cc = check_graph(graph)
    _check_mapping(mapping, N, K)
    K2 = T.check_count(num_components, "num_components")
    capacity, limit = PT.start_capacity(first_capacity(K2), contract_capacity_limit(K2, E), _start_capacity)
    dev = graph_device(graph, ((mapping, "mapping"),))

    lib = T.library(*_ENTRY)
    with torch.cuda.device(dev):
        if E == 0:
            return SuperpixelGraph(torch.zeros((2, 0), dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                                   torch.zeros((0, Cc), dtype=torch.int64, device=dev) if Cc else None,
                                   torch.zeros(N + 1, dtype=torch.int64, device=dev), K2, capacity)
        ei, offsets = graph_edges(graph)
        boundary, mp = graph.boundary.contiguous(), mapping.contiguous()
        contrast = graph.contrast.contiguous() if Cc else None

        def accumulate(capacity):
            ws, nbytes = T.scratch(dev, lib.fslic_hip_rag_workspace_size, N, K2, Cc, capacity)
            B._check(lib.fslic_hip_merge_contract_accumulate(dev.index, T.stream(dev), N, K, K2, E, ei.data_ptr(), offsets.data_ptr(),
                                                             boundary.data_ptr(), T.ptr(contrast), Cc, mp.data_ptr(), capacity,
                                                             ws.data_ptr(), nbytes))
            return ws, nbytes

        def compact(ws, nbytes, capacity, R, keys, count, sums=None):
            B._check(lib.fslic_hip_rag_compact(dev.index, T.stream(dev), N, Cc, capacity, ws.data_ptr(), nbytes, keys.data_ptr(),
                                               count.data_ptr(), T.ptr(sums), R))

        edge_index, count, extra, out_offsets, capacity = PT.run(accumulate, compact, N, capacity, limit, dev,
                                                                 [((Cc,), torch.int64)] if Cc else [])
    return SuperpixelGraph(edge_index, count, extra[0] if extra else None, out_offsets, K2, capacity)


def compose_mappings(first, then):
    """int32 [N, K]: then[f, first[f, v]], and -1 where first is -1 (or names no node of `then`): the total mapping of two rounds.
    `first` int32 [N, K], `then` int32 [N, K'], on one GPU.  Plain torch, no host synchronisation."""
    T.check_tensor(first, "first", (torch.int32,), "[N, K]", lambda s: len(s) == 2 and s[0] >= 1 and s[1] >= 1)
    _check_mapping(then, int(first.shape[0]), what="then")
    for t, what in ((first, "first"), (then, "then")):
        T.check_device(t, what)
    if first.device != then.device:
        raise ValueError("first and then must be on one GPU, got %s and %s" % (first.device, then.device))
    ok = (first >= 0) & (first < then.shape[1])
    picked = torch.gather(then, 1, first.clamp(0, then.shape[1] - 1).long())
    return torch.where(ok, picked, torch.full_like(picked, -1))
