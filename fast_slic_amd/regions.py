"""Merging regions by similarity along the region adjacency graph, on torch tensors in HBM (csrc/region.hip and merge.py's round):
reproducible features of the groups, the weights of the edges, a limit on the joins of a round, and the whole loop as one call.

    gsums, gcounts = group_sums(values, mapping, num_groups, counts)         # float32 [N, C, K2], counts' dtype [N, K2]
    weight         = edge_weights(graph, sums, counts, mode="mean")          # float32 [E]
    join           = limit_joins(graph, weight, join, quota)                 # bool [E]
    result         = merge_hierarchical(graph, sums, counts, threshold=None, target=None, max_rounds=8, mode="mean")
    result.mapping, result.n, result.graph, result.sums, result.counts

`graph` is a SuperpixelGraph (rag.py) of N frames, K = num_components nodes a frame and E edges; frames, positions and the rules 1 to
4 of the merge round are merge.py's.  `sums` float32 [N, C, K] and `counts` int32 or int64 [N, K] are what superpixel_pool(...,
reduce="sum", return_counts=True) gives for the graph's map ([C, K] and [K] are allowed when N = 1).  The rules:

1. Group sums.  A node v with mapping[f, v] in [0, K2) contributes values[f, c, v] to group mapping[f, v]; every other node
   contributes nothing.  A group's entry is the sum of its contributions by the model of superpixel_pool's sum (tests/pool_ref.py,
   exact_sum_bits): each contribution is truncated towards zero to a multiple of 2^-96, the contributions are added exactly, and the
   total is rounded once to float32, ties to even.  A zero total, or an empty group, gives +0.0; a NaN or Inf input leaves its
   group's entry unspecified.  The result does not depend on the order of the nodes or on the launch: the same bits from run to run.
   Counts are added as integers, in their dtype (a total beyond the dtype is unspecified).  No gradients.
2. Edge weights.  For an edge (a, b) of frame f, with n = float32(counts[f, .]): m_c = sums[f, c, .] / n for each channel c,
   d_c = m_c(a) - m_c(b), s = (((d_0^2 + d_1^2) + d_2^2) + ...) in ascending channel order.  mode "mean": w = sqrt(s), skimage's
   rag_mean_color; mode "ward": w = ((n_a * n_b) / (n_a + n_b)) * s, evaluated in that order.  Every operation is a separately rounded
   IEEE float32 operation, nothing is fused, division and square root are correctly rounded: a numpy float32 model written
   operation by operation gives the same bits.  The weight is +inf where an endpoint is outside [0, K) or its count is <= 0.
   Subnormal operands or intermediates leave the weight unspecified.
3. Limited joins.  Among the edges of frame f with `join` true and a finite weight, the quota[f] edges with the smallest
   (weight, position) key stay true -- the key of rule 1 of merge.py, -0.0 counted as +0.0 -- and everything else is false; a quota
   <= 0 keeps none.  The keys of a frame are distinct, so the joined edges of merge.py's rule 1 form a forest: an edge (a, b) closes
   no cycle, because along a cycle of best edges the keys would have to descend all the way round.  Each kept edge therefore lowers
   the number of groups by exactly one, and a quota of n - target leaves at least `target` groups.
4. The loop.  merge_hierarchical runs at most `max_rounds` rounds.  A round: edge_weights on the current regions;
   best_neighbour_edges(graph, weight, threshold); with `target`, limit_joins with quota = (n - target).clamp_min(0), where the first
   n is the number of nodes with a count > 0; merge_components(graph, join, members=counts); compose_mappings; contract_graph(graph,
   mapping, K); and the regions' features as group_sums of the caller's *original* sums and counts under the total mapping.  So a
   region's feature is one rounding of the exact sum of its original nodes, however many rounds formed it:
       result.sums, result.counts == group_sums(sums, result.mapping, K, counts), bit for bit.
   The loop also ends when the contracted graph has no edge, or as many edges as before the round (a join always removes an edge, so
   nothing joined).  With `target`: n[f] >= target always, and n[f] == target unless the rounds ran out or no eligible edge was left.
   result.graph has num_components = K; result.mapping is the total mapping int32 [N, K] from the graph's nodes, result.n int32 [N].

Out of scope: the sequential priority-queue order of skimage's merge_hierarchical (the parallel round is the semantics); gradients;
equality of the group sums with a re-pool from the *pixels* -- pooled node sums are already rounded, so it holds for the counts and
for features whose sums are exactly representable (integer features with sums below 2^24), not in general.

Every argument is checked before any device work.  The work runs on torch's current stream of the graph's (the mapping's) device and
scratch memory comes from torch's caching allocator; results live on that GPU.  group_sums, edge_weights and limit_joins do not
synchronise the host (limit_joins is plain torch: a stable sort of the 64-bit keys, then of the frames); merge_hierarchical adds no
synchronisation to contract_graph's, whose edge count is all its stopping rules read.  There is no CPU fallback.
This module imports torch; the package itself does not import it.
"""
import numbers

import torch

from . import _binding as B, _tensors as T
from .merge import best_neighbour_edges, compose_mappings, contract_graph, merge_components
from .rag import check_graph, graph_device, graph_edges

__all__ = ["group_sums", "edge_weights", "limit_joins", "merge_hierarchical", "MergeResult"]

_MODES = {"mean": 0, "ward": 1}                                            # kRegionMean, kRegionWard


_ENTRY = ("fslic_hip_region_sums", "region feature entry points")


class MergeResult(object):
    """What merge_hierarchical returns: mapping int32 [N, K], n int32 [N], graph (a SuperpixelGraph with num_components = K),
    sums float32 [N, C, K] and counts [N, K] of the regions."""

    def __init__(self, mapping, n, graph, sums, counts):
        self.mapping, self.n, self.graph, self.sums, self.counts = mapping, n, graph, sums, counts


# ---- argument checks: all of them run before any device work ----
def _check_values(values, what, N, K):
    """-> C of a float32 [N, C, K] tensor ([C, K] allowed when N = 1)."""
    T.check_tensor(values, what, (torch.float32,), "[N, C, K] = [%d, C, %d]%s with C >= 1" % (N, K, " or [C, K]" if N == 1 else ""),
                   lambda s: (len(s) == 3 and s[0] == N and s[1] >= 1 and s[2] == K) or (N == 1 and len(s) == 2 and s[0] >= 1 and s[1] == K))
    Cc = int(values.shape[-2])
    if N * Cc * K >= 1 << 31:
        raise ValueError("N * C * K must be below 2^31, got %s of shape %s" % (what, tuple(values.shape)))
    return Cc


def _check_counts(counts, N, K, what="counts"):
    T.check_tensor(counts, what, tuple(T.MEMBER_TYPE), "[N, K] = [%d, %d]%s" % (N, K, " or [K]" if N == 1 else ""),
                   lambda s: s == (N, K) or (N == 1 and s == (K,)))


def _check_mode(mode):
    if not isinstance(mode, str) or mode not in _MODES:
        raise ValueError("mode must be 'mean' or 'ward', got %r" % (mode,))
    return _MODES[mode]


def group_sums(values, mapping, num_groups, counts=None):
    """float32 [N, C, K2], and with `counts` (that, counts' dtype [N, K2]): the sums of `values` float32 [N, C, K] ([C, K] when N = 1)
    and of `counts` int32 / int64 [N, K] over the groups of `mapping` int32 [N, K], K2 = num_groups (rule 1 of the module's text).
    Exact and reproducible; two launches behind two clears, no host synchronisation, no gradients."""
    T.check_tensor(mapping, "mapping", (torch.int32,), "[N, K]", lambda s: len(s) == 2 and s[0] >= 1 and 1 <= s[1] <= T.MAX_COMPONENTS)
    N, K = (int(v) for v in mapping.shape)
    Cc = _check_values(values, "values", N, K)
    if isinstance(num_groups, bool) or not isinstance(num_groups, numbers.Integral) or not 1 <= int(num_groups) <= T.MAX_COMPONENTS:
        raise ValueError("num_groups must be an integer in [1, %d], got %r" % (T.MAX_COMPONENTS, num_groups))
    K2 = int(num_groups)
    if N * Cc * K2 >= 1 << 31:
        raise ValueError("N * C * num_groups must be below 2^31")
    if counts is not None:
        _check_counts(counts, N, K)
    dev = T.one_device(((values, "values"), (mapping, "mapping"), (counts, "counts")))

    lib = T.library(*_ENTRY)
    with torch.cuda.device(dev):
        val, mp = values.detach().contiguous(), mapping.contiguous()
        cnt = counts.contiguous() if counts is not None else None
        sums = torch.empty((N, Cc, K2), dtype=torch.float32, device=dev)
        out_counts = torch.empty((N, K2), dtype=cnt.dtype, device=dev) if cnt is not None else None
        ws, nbytes = T.scratch(dev, lib.fslic_hip_region_sums_workspace_size, N, Cc, K2)
        B._check(lib.fslic_hip_region_sums(dev.index, T.stream(dev), N, Cc, K, K2, val.data_ptr(), mp.data_ptr(), T.ptr(cnt),
                                           T.MEMBER_TYPE[cnt.dtype] if cnt is not None else 0, sums.data_ptr(), T.ptr(out_counts),
                                           ws.data_ptr(), nbytes))
    return sums if counts is None else (sums, out_counts)


def edge_weights(graph, sums, counts, mode="mean"):
    """float32 [E]: the weight of every edge from the means of its two regions (rule 2 of the module's text).  `sums` float32
    [N, C, K], `counts` int32 / int64 [N, K] on the graph's GPU; mode "mean" or "ward".  One launch, no host synchronisation."""
    N, K, E, _ = check_graph(graph)
    Cc = _check_values(sums, "sums", N, K)
    _check_counts(counts, N, K)
    m = _check_mode(mode)
    dev = graph_device(graph, ((sums, "sums"), (counts, "counts")))

    lib = T.library(*_ENTRY)
    with torch.cuda.device(dev):
        weight = torch.empty(E, dtype=torch.float32, device=dev)
        if E == 0:
            return weight
        ei, offsets = graph_edges(graph)
        s, cnt = sums.detach().contiguous(), counts.contiguous()
        B._check(lib.fslic_hip_region_edge_weights(dev.index, T.stream(dev), N, Cc, K, E, ei.data_ptr(), offsets.data_ptr(), s.data_ptr(),
                                                   cnt.data_ptr(), T.MEMBER_TYPE[cnt.dtype], m, weight.data_ptr()))
    return weight


def limit_joins(graph, weight, join, quota):
    """bool [E]: of frame f's edges with `join` true and a finite weight, the quota[f] with the smallest (weight, position) stay true
    (rule 3 of the module's text).  `weight` float32 [E], `join` bool [E], `quota` int32 / int64 [N].  Plain torch: a stable sort of
    the 64-bit keys, then of the frames; no host synchronisation."""
    N, K, E, _ = check_graph(graph)
    T.check_tensor(weight, "weight", (torch.float32,), "[E] with E = %d, one per edge of the graph" % E, lambda s: s == (E,))
    T.check_tensor(join, "join", (torch.bool,), "[E] with E = %d, one per edge of the graph" % E, lambda s: s == (E,))
    T.check_tensor(quota, "quota", tuple(T.MEMBER_TYPE), "[N] with N = %d, one per frame" % N, lambda s: s == (N,))
    dev = graph_device(graph, ((weight, "weight"), (join, "join"), (quota, "quota")))

    with torch.cuda.device(dev):
        if E == 0:
            return torch.empty(0, dtype=torch.bool, device=dev)
        offsets = graph.offsets.contiguous()
        index = torch.arange(E, device=dev)
        frame = torch.searchsorted(offsets[1:].contiguous(), index, right=True).clamp_max(N - 1)
        w = weight.contiguous()
        ok = join & torch.isfinite(w)
        bits = torch.where(w == 0, torch.zeros_like(w), w).view(torch.int32).long()      # non-negative float bits order like the values
        key = torch.where(ok, (bits << 32) | (index - offsets[frame]), torch.full_like(bits, (1 << 63) - 1))
        order = torch.argsort(key, stable=True)
        order = order[torch.argsort(frame[order], stable=True)]                          # by (frame, key): a frame's edges are neighbours
        f = frame[order]
        keep = ok[order] & (index - offsets[f] < quota.long()[f])
        return torch.zeros(E, dtype=torch.bool, device=dev).index_put_((order,), keep)


def merge_hierarchical(graph, sums, counts, threshold=None, target=None, max_rounds=8, mode="mean"):
    """A MergeResult (mapping, n, graph, sums, counts): the rounds of rule 4 of the module's text.  `threshold` None or a number: only
    edges with a weight below it join; `target` None or an integer >= 1: no frame goes below that many regions; at most `max_rounds`
    rounds.  One host synchronisation a round, contract_graph's."""
    N, K, E, _ = check_graph(graph)
    Cc = _check_values(sums, "sums", N, K)
    _check_counts(counts, N, K)
    if threshold is not None and (isinstance(threshold, bool) or not isinstance(threshold, numbers.Real)):
        raise ValueError("threshold must be None or a number, got %r" % (threshold,))
    if target is not None and (isinstance(target, bool) or not isinstance(target, numbers.Integral) or target < 1):
        raise ValueError("target must be None or an integer >= 1, got %r" % (target,))
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, numbers.Integral) or max_rounds < 1:
        raise ValueError("max_rounds must be an integer >= 1, got %r" % (max_rounds,))
    _check_mode(mode)
    dev = graph_device(graph, ((sums, "sums"), (counts, "counts")))

    with torch.cuda.device(dev):
        sums0, counts0 = sums.detach().reshape(N, Cc, K).contiguous(), counts.reshape(N, K).contiguous()
        g, s, c, total = graph, sums0, counts0, None
        n = (counts0 > 0).sum(1, dtype=torch.int32)
        for _ in range(int(max_rounds)):
            before = int(g.edge_index.shape[1])
            w = edge_weights(g, s, c, mode)
            join = best_neighbour_edges(g, w, threshold)
            if target is not None:
                join = limit_joins(g, w, join, (n - int(target)).clamp_min(0))
            mapping, n = merge_components(g, join, members=c)
            total = mapping if total is None else compose_mappings(total, mapping)
            g = contract_graph(g, mapping, K)
            s, c = group_sums(sums0, total, K, counts0)
            after = int(g.edge_index.shape[1])
            if after == 0 or after == before:
                break
    return MergeResult(total, n, g, s, c)
