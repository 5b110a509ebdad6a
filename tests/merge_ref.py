"""The model of fast_slic_amd/merge.py: numpy and plain Python, written from the rules of that module's text (each node's best edge
by (weight, position); the groups of the present nodes under the joined edges, numbered by their smallest node; the relabelled
pixels; the contracted graph; the composition of two mappings).  A graph is the dict tests/rag_ref.py returns (edge_index int64
[2, E], boundary, contrast or None, offsets int64 [N + 1]).  Slow and plain on purpose: one frame at a time, one edge at a time."""
import numpy as np


def frames_of(g):
    """Per frame (first edge, one past the last)."""
    off = np.asarray(g["offsets"])
    return [(int(off[f]), int(off[f + 1])) for f in range(len(off) - 1)]


def best_edges(g, weight, threshold=None):
    """join bool [E]."""
    a, b = np.asarray(g["edge_index"])
    w = np.asarray(weight, np.float32).astype(np.float64) + 0.0            # (-0.0 + 0.0 is +0.0)
    join = np.zeros(a.shape[0], bool)
    for lo, hi in frames_of(g):
        best = {}                                                          # node -> ((weight, position), edge)
        for e in range(lo, hi):
            if threshold is not None and not w[e] < threshold:
                continue
            key = (w[e], e - lo)
            for v in (int(a[e]), int(b[e])):
                if v not in best or key < best[v][0]:
                    best[v] = (key, e)
        for _, e in best.values():
            join[e] = True
    return join


def components(g, join, K, members=None):
    """(mapping int32 [N, K], n int32 [N])."""
    a, b = np.asarray(g["edge_index"])
    spans = frames_of(g)
    N = len(spans)
    present = np.ones((N, K), bool) if members is None else np.asarray(members).reshape(N, K) > 0
    mapping = np.full((N, K), -1, np.int32)
    n = np.zeros(N, np.int32)
    for f, (lo, hi) in enumerate(spans):
        parent = list(range(K))

        def find(v):
            while parent[v] != v:
                parent[v] = parent[parent[v]]
                v = parent[v]
            return v

        for e in range(lo, hi):
            u, v = int(a[e]), int(b[e])
            if join[e] and present[f, u] and present[f, v]:
                ru, rv = find(u), find(v)
                if ru != rv:
                    parent[max(ru, rv)] = min(ru, rv)                      # the root of a set is its smallest node: the leader
        number = {}
        for v in range(K):                                                 # ascending: a leader comes before every other node of its group
            if present[f, v]:
                r = find(v)
                if r == v:
                    number[v] = len(number)
                mapping[f, v] = number[r]
        n[f] = len(number)
    return mapping, n


def labels(lab, mapping):
    """int32, of the shape of lab."""
    lab = np.asarray(lab)
    if lab.dtype == np.int16:
        lab = lab.view(np.uint16)                                          # the int16 map is read as uint16: -1 is 0xFFFF, above any K
    mapping = np.asarray(mapping)
    if mapping.ndim == 1:
        mapping = mapping[None]
    l3 = lab.astype(np.int64).reshape((-1,) + lab.shape[-2:])
    K = mapping.shape[1]
    out = np.full(l3.shape, -1, np.int32)
    for f in range(l3.shape[0]):
        ok = (l3[f] >= 0) & (l3[f] < K)
        out[f][ok] = mapping[f][l3[f][ok]]
    return out.reshape(lab.shape)


def contract(g, mapping, K2):
    """The graph dict of the groups."""
    a, b = np.asarray(g["edge_index"])
    mapping = np.asarray(mapping)
    contrast = g["contrast"]
    edges, boundary, rows, offsets = [], [], [], [0]
    for f, (lo, hi) in enumerate(frames_of(g)):
        acc = {}                                                           # (lo, hi) -> [boundary, contrast row]
        for e in range(lo, hi):
            u, v = int(mapping[f, a[e]]), int(mapping[f, b[e]])
            if not (0 <= u < K2 and 0 <= v < K2) or u == v:
                continue
            cell = acc.setdefault((min(u, v), max(u, v)), [0, 0 if contrast is None else np.zeros(contrast.shape[1], np.int64)])
            cell[0] += int(g["boundary"][e])
            if contrast is not None:
                cell[1] = cell[1] + np.asarray(contrast[e], np.int64)
        for pair in sorted(acc):
            edges.append(pair)
            boundary.append(acc[pair][0])
            rows.append(acc[pair][1])
        offsets.append(len(edges))
    C = 0 if contrast is None else contrast.shape[1]
    return dict(edge_index=np.asarray(edges, np.int64).reshape(-1, 2).T.copy(), boundary=np.asarray(boundary, np.int64),
                contrast=None if contrast is None else np.asarray(rows, np.int64).reshape(-1, C), offsets=np.asarray(offsets, np.int64))


def compose(first, then):
    first, then = np.asarray(first), np.asarray(then)
    out = np.full(first.shape, -1, np.int32)
    for f in range(first.shape[0]):
        ok = (first[f] >= 0) & (first[f] < then.shape[1])
        out[f][ok] = then[f][first[f][ok]]
    return out


def same_graph(x, y):
    """Field for field."""
    return (np.array_equal(x["edge_index"], y["edge_index"]) and np.array_equal(x["boundary"], y["boundary"])
            and np.array_equal(x["offsets"], y["offsets"]) and (x["contrast"] is None) == (y["contrast"] is None)
            and (x["contrast"] is None or np.array_equal(x["contrast"], y["contrast"])))
