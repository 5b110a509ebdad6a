"""The model of fast_slic_amd/regions.py: numpy and plain Python, written from the rules of that module's text.  Group sums are
tests/pool_ref.py's exact sum (Python integers, one rounding); the edge weights are numpy float32 arithmetic, one operation a line,
each rounded on its own; limit_joins sorts a frame's joined edges by (weight, position); the driver runs the rounds over
tests/merge_ref.py's functions.  A graph is the dict of tests/rag_ref.py."""
import numpy as np

import merge_ref as M
import pool_ref

F32 = np.float32


def group_sums(values, mapping, K2, counts=None):
    """values float32 [N, C, K], mapping [N, K] -> float32 [N, C, K2] (and counts' dtype [N, K2]): per group the exact sum."""
    values = np.ascontiguousarray(values, F32)
    mapping = np.asarray(mapping)
    N, K = mapping.shape
    values = values.reshape(N, -1, K)
    bits = values.view(np.uint32)
    out = np.zeros((N, values.shape[1], K2), np.uint32)
    for f in range(N):
        members = {}
        for v in range(K):
            if 0 <= mapping[f, v] < K2:
                members.setdefault(int(mapping[f, v]), []).append(v)
        for c in range(values.shape[1]):
            row = bits[f, c].tolist()
            for grp, nodes in members.items():
                out[f, c, grp] = pool_ref.exact_sum_bits([row[v] for v in nodes])
    sums = out.view(F32)
    if counts is None:
        return sums
    counts = np.asarray(counts).reshape(N, K)
    total = np.zeros((N, K2), counts.dtype)
    for f in range(N):
        ok = (mapping[f] >= 0) & (mapping[f] < K2)
        np.add.at(total[f], mapping[f][ok], counts[f][ok])
    return sums, total


def frame_of_edges(g):
    off = np.asarray(g["offsets"])
    E = np.asarray(g["edge_index"]).shape[1]
    return np.minimum(np.searchsorted(off[1:], np.arange(E), side="right"), len(off) - 2)


def edge_weights(g, sums, counts, mode="mean"):
    """float32 [E], every operation a float32 operation of its own."""
    a, b = np.asarray(g["edge_index"])
    counts = np.asarray(counts)
    N = len(g["offsets"]) - 1
    K = counts.shape[-1]
    counts = counts.reshape(N, K)
    sums = np.asarray(sums, F32).reshape(N, -1, K)
    frame = frame_of_edges(g)
    inside = (a >= 0) & (a < K) & (b >= 0) & (b < K)
    ia, ib = np.where(inside, a, 0), np.where(inside, b, 0)
    ca, cb = counts[frame, ia], counts[frame, ib]
    ok = inside & (ca > 0) & (cb > 0)
    na, nb = np.where(ok, ca, 1).astype(F32), np.where(ok, cb, 1).astype(F32)      # (int -> float32: to nearest, ties to even)
    s = None
    with np.errstate(all="ignore"):
        for c in range(sums.shape[1]):
            ma = sums[frame, c, ia] / na
            mb = sums[frame, c, ib] / nb
            d = ma - mb
            q = d * d
            s = q if s is None else s + q
        if mode == "mean":
            w = np.sqrt(s)
        else:
            p = na * nb
            t = na + nb
            r = p / t
            w = r * s
    assert w.dtype == F32
    return np.where(ok, w, F32(np.inf)).astype(F32)


def limit_joins(g, weight, join, quota):
    """bool [E]: per frame the quota[f] joined edges of finite weight with the smallest (weight, position)."""
    w = np.asarray(weight, F32).astype(np.float64) + 0.0                    # (-0.0 + 0.0 is +0.0)
    join = np.asarray(join, bool)
    out = np.zeros(join.shape[0], bool)
    for f, (lo, hi) in enumerate(M.frames_of(g)):
        cand = sorted((w[e], e - lo) for e in range(lo, hi) if join[e] and np.isfinite(w[e]))
        for _, pos in cand[:max(int(quota[f]), 0)]:
            out[lo + pos] = True
    return out


def merge_hierarchical(g, sums, counts, threshold=None, target=None, max_rounds=8, mode="mean"):
    """dict(mapping, n, graph, sums, counts, rounds): the rounds of rule 4."""
    counts0 = np.asarray(counts)
    N = len(g["offsets"]) - 1
    K = counts0.shape[-1]
    counts0 = counts0.reshape(N, K)
    sums0 = np.asarray(sums, F32).reshape(N, -1, K)
    s, c, total = sums0, counts0, None
    n = (counts0 > 0).sum(1).astype(np.int32)
    rounds = 0
    for _ in range(max_rounds):
        before = g["boundary"].shape[0]
        w = edge_weights(g, s, c, mode)
        join = M.best_edges(g, w, threshold)
        if target is not None:
            join = limit_joins(g, w, join, np.maximum(n.astype(np.int64) - target, 0))
        mapping, n = M.components(g, join, K, c)
        total = mapping if total is None else M.compose(total, mapping)
        g = M.contract(g, mapping, K)
        s, c = group_sums(sums0, total, K, counts0)
        rounds += 1
        after = g["boundary"].shape[0]
        if after == 0 or after == before:
            break
    return dict(mapping=total, n=n, graph=g, sums=s, counts=c, rounds=rounds)


def graph_components(g, K, members):
    """Per frame the connected components of the present nodes under all the graph's edges between present nodes."""
    E = g["boundary"].shape[0]
    return M.components(g, np.ones(E, bool), K, members)[1]
