"""Numpy model of the comparison of two label maps (fast_slic_amd/compare.py): np.unique on frame * K * M + a * M + b over the pixels
that take part, the four quantities derived from the table, and the boundary match by OR over shifted copies of the boundary mask.
Slow and obvious on purpose: it is the yardstick of tests/test_gpu_compare.py, and tests/test_compare_cpu.py checks it against plain
loops where no GPU exists."""
import numpy as np


def _frames(a):
    a = np.asarray(a)
    return a[None] if a.ndim == 2 else a


def overlap(labels, other, K, M):
    """[H, W] or [N, H, W] -> dict(pairs int64 [2, P] sorted by (frame, a, b), count int64 [P], offsets int64 [N + 1], frame int64 [P])."""
    la, ot = _frames(labels).astype(np.int64), _frames(other).astype(np.int64)      # (a uint16 view's 0xFFFF stays outside any K)
    N = la.shape[0]
    ok = (la >= 0) & (la < K) & (ot >= 0) & (ot < M)
    frame = np.broadcast_to(np.arange(N, dtype=np.int64)[:, None, None], la.shape)
    keys, count = np.unique((frame * K * M + la * M + ot)[ok], return_counts=True)
    f, rest = keys // (K * M), keys % (K * M)
    offsets = np.zeros(N + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(f, minlength=N))
    return dict(pairs=np.stack([rest // M, rest % M]).astype(np.int64).reshape(2, -1), count=count.astype(np.int64), offsets=offsets, frame=f)


def _n(t):
    return t["offsets"].shape[0] - 1


def areas(t, K, M):
    """(int64 [N, K], int64 [N, M]): the pixels of every a and of every b among those that take part."""
    A, Bm = np.zeros((_n(t), K), np.int64), np.zeros((_n(t), M), np.int64)
    np.add.at(A, (t["frame"], t["pairs"][0]), t["count"])
    np.add.at(Bm, (t["frame"], t["pairs"][1]), t["count"])
    return A, Bm


def majority(t, K, M):
    """int64 [N, K]: the b of the largest count of every a, the smallest such b on a tie; -1 where a has no pixel."""
    out = np.full((_n(t), K), -1, np.int64)
    f, (a, b), c = t["frame"], t["pairs"], t["count"]
    order = np.lexsort((-b, c, a, f))                  # within one (frame, a): ascending count, then descending b -- the last one wins
    out[f[order], a[order]] = b[order]                 # (numpy assigns repeated indices in order: the last assignment stays)
    return out


def _totals(t):
    n = np.zeros(_n(t), np.int64)
    np.add.at(n, t["frame"], t["count"])
    return n.astype(np.float64)


def best_overlap(t, K, M):
    best = np.zeros((_n(t), K), np.int64)
    np.maximum.at(best, (t["frame"], t["pairs"][0]), t["count"])
    with np.errstate(invalid="ignore"):
        return best.sum(1).astype(np.float64) / _totals(t)


def undersegmentation_error(t, K, M):
    A, _ = areas(t, K, M)
    leak = np.zeros(_n(t), np.int64)
    np.add.at(leak, t["frame"], np.minimum(t["count"], A[t["frame"], t["pairs"][0]] - t["count"]))
    with np.errstate(invalid="ignore"):
        return leak.astype(np.float64) / _totals(t)


def boundary_mask(a):
    """[H, W] -> bool [H, W]: the value differs from the right or the lower neighbour's (as tests/util.py::boundary_mask)."""
    a = np.asarray(a)
    m = np.zeros(a.shape, bool)
    m[:, :-1] |= a[:, :-1] != a[:, 1:]
    m[:-1, :] |= a[:-1, :] != a[1:, :]
    return m


def dilate(m, r):
    """OR over the copies of m shifted by (dy, dx), |dy| <= r and |dx| <= r, inside the image."""
    H, W = m.shape
    out = np.zeros_like(m)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, yd = (slice(0, max(H - dy, 0)), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, max(H + dy, 0)))
            xs, xd = (slice(0, max(W - dx, 0)), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, max(W + dx, 0)))
            out[yd, xd] |= m[ys, xs]
    return out


def boundary_match(labels, other, tolerance=0):
    """[H, W] -> int64 [3], [N, H, W] -> int64 [N, 3]: (hits, boundary pixels of other, boundary pixels of labels)."""
    la, ot = _frames(labels), _frames(other)
    rows = []
    for n in range(la.shape[0]):
        ml, mo = boundary_mask(la[n]), boundary_mask(ot[n])
        rows.append([int((mo & dilate(ml, tolerance)).sum()), int(mo.sum()), int(ml.sum())])
    out = np.array(rows, np.int64)
    return out if np.asarray(labels).ndim == 3 else out[0]
