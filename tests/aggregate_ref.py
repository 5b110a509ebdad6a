"""The numpy model of fast_slic_amd/propagate.py's rules 1 to 4, float32 operation by operation (every numpy float32 array operation
rounds each element once, so vectorising over the channels or the entries keeps the order of every fold), and a float64 restatement
through a dense adjacency matrix.  No torch, no GPU.

Lists: offsets int64 [N * K + 1], indices int32 [nnz], weight float32 [nnz] or None; x and g float32 [N, C, K]."""
import numpy as np

F32 = np.float32


def rows_of(offsets, nnz):
    """The row over (frame, node) of every entry: how many rows end at or before it (N * K: behind the last row)."""
    return np.searchsorted(np.asarray(offsets)[1:], np.arange(nnz), side="right")


def transposed(offsets, indices, N, K):
    """target row -> the list of (entry p, row of p) whose index names it, in ascending p; invalid entries belong to none."""
    rows = rows_of(offsets, len(indices))
    out = [[] for _ in range(N * K)]
    for p in range(len(indices)):
        j, r = int(indices[p]), int(rows[p])
        if 0 <= j < K and r < N * K:
            out[(r // K) * K + j].append((p, r))
    return out


def forward(x, offsets, indices, weight=None, reduce="sum"):
    """-> (y float32 [N, C, K], argmax int32 [N, C, K] (max, else None), degree int64 [N * K] of valid entries)."""
    x = np.asarray(x, F32)
    N, C, K = x.shape
    y = np.zeros((N, C, K), F32)
    arg = np.full((N, C, K), -1, np.int32)
    deg = np.zeros(N * K, np.int64)
    for r in range(N * K):
        f, i = divmod(r, K)
        acc = np.zeros(C, F32)
        best = np.full(C, -1, np.int32)
        d = 0
        for p in range(int(offsets[r]), int(offsets[r + 1])):
            j = int(indices[p])
            if not 0 <= j < K:
                continue
            d += 1
            v = x[f, :, j]
            if reduce == "max":
                take = (best < 0) | (v > acc)
                acc = np.where(take, v, acc)
                best = np.where(take, np.int32(p), best)
            else:
                term = v if weight is None or reduce == "mean" else (F32(weight[p]) * v).astype(F32)
                acc = (acc + term).astype(F32)
        if reduce == "mean" and d > 0:
            acc = (acc / F32(d)).astype(F32)
        y[f, :, i] = acc
        arg[f, :, i] = best
        deg[r] = d
    return y, (arg if reduce == "max" else None), deg


def backward_values(g, offsets, indices, weight=None, reduce="sum", argmax=None, degree=None):
    """grad_x float32 [N, C, K] by rule 4; argmax with max and degree with mean as forward() gave them."""
    g = np.asarray(g, F32)
    N, C, K = g.shape
    gx = np.zeros((N, C, K), F32)
    for t, entries in enumerate(transposed(offsets, indices, N, K)):
        f, j = divmod(t, K)
        acc = np.zeros(C, F32)
        for p, r in entries:
            i = r - f * K
            v = g[f, :, i]
            if reduce == "sum":
                term = v if weight is None else (F32(weight[p]) * v).astype(F32)
            elif reduce == "mean":
                term = (v / F32(degree[r])).astype(F32)
            else:
                acc = np.where(argmax[f, :, i] == p, (acc + v).astype(F32), acc)      # the fold skips every other entry
                continue
            acc = (acc + term).astype(F32)
        gx[f, :, j] = acc
    return gx


def backward_weight(x, g, offsets, indices):
    """grad_weight float32 [nnz]: the fold over c of x[f, c, indices[p]] * g[f, c, row(p)]; +0.0 for an invalid entry."""
    x, g = np.asarray(x, F32), np.asarray(g, F32)
    N, C, K = x.shape
    rows, j = rows_of(offsets, len(indices)), np.asarray(indices, np.int64)
    valid = (j >= 0) & (j < K) & (rows < N * K)
    f, i, j = np.where(valid, rows // K, 0), np.where(valid, rows % K, 0), np.where(valid, j, 0)
    acc = np.zeros(len(indices), F32)
    for c in range(C):                                                     # every entry at once, the channels in order
        acc = (acc + (x[f, c, j] * g[f, c, i]).astype(F32)).astype(F32)
    return np.where(valid, acc, F32(0))


# ---- the float64 restatement: y = A x with the dense A[f][i][j] = the sum of the weights of the valid entries (i <- j) ----
def dense(offsets, indices, weight, N, K):
    A = np.zeros((N, K, K), np.float64)
    rows = rows_of(offsets, len(indices))
    for p in range(len(indices)):
        j, r = int(indices[p]), int(rows[p])
        if 0 <= j < K and r < N * K:
            A[r // K, r % K, j] += 1.0 if weight is None else float(weight[p])
    return A


def sum64(x, g, offsets, indices, weight=None):
    """-> (y, grad_x, grad_weight) of reduce="sum" in float64, and the sums of the absolute terms of each (for the error bound)."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    N, C, K = x.shape
    A = dense(offsets, indices, weight, N, K)
    y, gx = np.einsum("fij,fcj->fci", A, x), np.einsum("fij,fci->fcj", A, g)
    ya, gxa = np.einsum("fij,fcj->fci", np.abs(A), np.abs(x)), np.einsum("fij,fci->fcj", np.abs(A), np.abs(g))
    rows = rows_of(offsets, len(indices))
    gw, gwa = np.zeros(len(indices)), np.zeros(len(indices))
    for p in range(len(indices)):
        j, r = int(indices[p]), int(rows[p])
        if 0 <= j < K and r < N * K:
            prod = x[r // K, :, j] * g[r // K, :, r % K]
            gw[p], gwa[p] = prod.sum(), np.abs(prod).sum()
    return (y, gx, gw), (ya, gxa, gwa)


def gamma(d):
    """The standard bound of a product plus d - 1 additions, d the terms of the fold: (d + 1) u / (1 - (d + 1) u), u = 2^-24."""
    u = (d + 1) * 2.0 ** -24
    return u / (1.0 - u)
