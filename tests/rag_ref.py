"""Numpy reference of the region adjacency graph (fast_slic_amd/rag.py): the pair keys of every direction, np.unique with counts for
the boundary lengths, np.add.at for the contrast.  Slow and obvious on purpose: it is the yardstick of tests/test_gpu_rag.py, and
tests/test_rag_cpu.py checks it by hand where no GPU exists."""
import numpy as np

# (dy, dx) of the neighbour every pixel looks at: 4-connectivity the first two, 8-connectivity all four
DIRECTIONS = ((0, 1), (1, 0), (1, 1), (1, -1))


def _sides(a, dy, dx):
    """The two views of a [H, W, ...] array whose elements at equal positions are the pixel and its (dy, dx) neighbour."""
    H, W = a.shape[:2]
    if dx >= 0:
        return a[:H - dy, :W - dx], a[dy:, dx:]
    return a[:H - dy, -dx:], a[dy:, :W + dx]


def graph_frame(labels, K, connectivity=4, image=None):
    """One [H, W] map -> (edges int64 [E, 2] with column 0 < column 1, sorted by (column 0, column 1); boundary int64 [E];
    contrast int64 [E, C] or None)."""
    lab = np.asarray(labels).astype(np.int64)
    keys, diffs = [], []
    for dy, dx in DIRECTIONS[:2 if connectivity == 4 else 4]:
        p, q = _sides(lab, dy, dx)
        ok = (p >= 0) & (p < K) & (q >= 0) & (q < K) & (p != q)
        keys.append((np.minimum(p, q) * K + np.maximum(p, q))[ok])
        if image is not None:
            ip, iq = _sides(np.asarray(image).astype(np.int64), dy, dx)
            diffs.append(np.abs(ip - iq)[ok])
    keys = np.concatenate(keys)
    uniq, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    edges = np.stack([uniq // K, uniq % K], axis=1).astype(np.int64).reshape(-1, 2)
    contrast = None
    if image is not None:
        contrast = np.zeros((uniq.shape[0], np.asarray(image).shape[-1]), np.int64)
        np.add.at(contrast, inverse.reshape(-1), np.concatenate(diffs))
    return edges, counts.astype(np.int64), contrast


def graph(labels, K, connectivity=4, image=None):
    """[H, W] or [N, H, W] -> dict(edge_index int64 [2, E], boundary int64 [E], contrast int64 [E, C] or None, offsets int64 [N + 1]),
    the edges of frame n at [offsets[n], offsets[n + 1])."""
    lab = np.asarray(labels)
    if lab.ndim == 2:
        lab = lab[None]
        image = None if image is None else np.asarray(image)[None]
    parts = [graph_frame(lab[n], K, connectivity, None if image is None else image[n]) for n in range(lab.shape[0])]
    offsets = np.zeros(lab.shape[0] + 1, np.int64)
    offsets[1:] = np.cumsum([p[0].shape[0] for p in parts])
    return dict(edge_index=np.concatenate([p[0] for p in parts]).T.copy(),
                boundary=np.concatenate([p[1] for p in parts]),
                contrast=None if image is None else np.concatenate([p[2] for p in parts]),
                offsets=offsets)
