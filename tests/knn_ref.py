"""The numpy model of fast_slic_amd.knn.knn_graph, operation by operation: float32 arrays, the fold over the channels as written in
the module's text (t = x - y; acc = acc + t * t, each a float32 operation rounded on its own), the masks, and the selection of a
row with np.lexsort((j, d)): distance first, the smaller node number on ties.  The kernel is held to it bit for bit."""
import numpy as np

F32 = np.float32


def distances(x, y):
    """d float32 [N, K, K] of x, y float32 [N, D, K]: d[f, i, j] = the left fold over c of (x[f, c, i] - y[f, c, j]) ** 2."""
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == F32 and y.dtype == F32 and x.shape == y.shape and x.ndim == 3
    N, D, K = x.shape
    acc = np.zeros((N, K, K), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(D):
            t = x[:, c, :, None] - y[:, c, None, :]
            acc = acc + t * t
    assert acc.dtype == F32
    return acc


def knn(points, k, other=None, valid=None, loop=False):
    """-> (indices int32 [N * K * k], dist float32 [N * K * k]) of points float32 [N, D, K]."""
    x = np.asarray(points)
    assert not (loop and other is not None)
    N, D, K = x.shape
    d = distances(x, x if other is None else np.asarray(other))
    ok = np.ones((N, K), bool) if valid is None else np.asarray(valid, bool).reshape(N, K)
    indices, dist = np.full((N, K, k), -1, np.int32), np.full((N, K, k), np.inf, F32)
    nodes = np.arange(K)
    for f in range(N):
        for i in range(K):
            if not ok[f, i]:
                continue
            cand = ok[f] & ~np.isnan(d[f, i])
            if other is None and not loop:
                cand[i] = False
            j = nodes[cand]
            dj = d[f, i, cand]
            order = np.lexsort((j, dj))[:k]
            indices[f, i, :order.size], dist[f, i, :order.size] = j[order], dj[order]
    return indices.reshape(-1), dist.reshape(-1)


def brute64(points, k, other=None, valid=None, loop=False):
    """The same selection from float64 distances summed in one call: exact, and equal to the model's, where every partial sum is an
    integer below 2^24."""
    x = np.asarray(points, np.float64)
    y = x if other is None else np.asarray(other, np.float64)
    N, D, K = x.shape
    d = ((x[:, :, :, None] - y[:, :, None, :]) ** 2).sum(axis=1)
    ok = np.ones((N, K), bool) if valid is None else np.asarray(valid, bool).reshape(N, K)
    indices, dist = np.full((N, K, k), -1, np.int64), np.full((N, K, k), np.inf)
    for f in range(N):
        for i in range(K):
            if not ok[f, i]:
                continue
            cand = [(d[f, i, j], j) for j in range(K) if ok[f, j] and not (other is None and not loop and j == i)]
            for o, (dj, j) in enumerate(sorted(cand)[:k]):
                indices[f, i, o], dist[f, i, o] = j, dj
    return indices.reshape(-1), dist.reshape(-1)
