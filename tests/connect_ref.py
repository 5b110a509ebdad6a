"""The model of fast_slic_amd/connect.py: numpy and a plain Python union-find, written from the five rules of that module's text
(components by leader order; kept components numbered in leader order; component 0 takes label 0; every other unkept component takes
the final label of the component left of, or for a leader in column 0 above, its leader; n = kept components, or 1).  Slow and plain on
purpose: one frame at a time, one pixel at a time."""
import numpy as np


def blocky(H, W, K, seed, dtype=np.int32):
    """A map of about K labels in blocks a few pixels wide, edges ragged (as tests/test_gpu_compare.py's maps)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    bh, bw = int(rng.integers(3, 12)), int(rng.integers(5, 40))
    grid = (y // bh) * ((W + bw - 1) // bw) + x // bw
    return ((grid + (rng.random((H, W)) < 0.05) * rng.integers(0, K, (H, W))) % K).astype(dtype)


def noise(H, W, K, seed, dtype=np.int32):
    """Every pixel one of K labels at random: with K = 3 many components, and many of them across every tile edge."""
    return np.random.default_rng(seed).integers(0, K, (H, W)).astype(dtype)


def components(lab):
    """lab [H, W] -> (comp int32 [H, W]: the number of every pixel's component, leaders: the raster index of every component's first
    pixel, ascending, areas: the pixels of every component)."""
    lab = np.asarray(lab)
    H, W = lab.shape
    flat = lab.reshape(-1)
    parent = list(range(H * W))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    left = np.zeros((H, W), bool)
    left[:, 1:] = lab[:, 1:] == lab[:, :-1]
    up = np.zeros((H, W), bool)
    up[1:, :] = lab[1:, :] == lab[:-1, :]
    for same, step in ((left.reshape(-1), 1), (up.reshape(-1), W)):
        for p in np.flatnonzero(same).tolist():
            a, b = find(p), find(p - step)
            if a != b:
                parent[max(a, b)] = min(a, b)              # the root of a set is its smallest index: the leader
    roots = np.fromiter((find(p) for p in range(H * W)), np.int64, H * W)
    leaders, comp, areas = np.unique(roots, return_inverse=True, return_counts=True)
    assert flat.shape[0] == comp.shape[0]
    return comp.reshape(H, W).astype(np.int32), leaders, areas


def enforce(lab, min_size):
    """lab [H, W] -> (out int32 [H, W], n)."""
    comp, leaders, areas = components(lab)
    H, W = comp.shape
    flat = comp.reshape(-1)
    kept = areas >= min_size
    sub = np.full(len(leaders), -1, np.int64)
    sub[kept] = np.arange(int(kept.sum()))                  # rule 2
    if not kept[0]:
        sub[0] = 0                                          # rule 3
    for c in range(1, len(leaders)):                        # rule 4: ascending, so that the neighbour's label is final
        if sub[c] < 0:
            p = int(leaders[c])
            q = p - 1 if p % W else p - W
            assert flat[q] < c
            sub[c] = sub[flat[q]]
    return sub[comp].astype(np.int32), max(int(kept.sum()), 1)


def components_batch(labs):
    """[N, H, W] -> (comp [N, H, W] int32, n [N] int32)."""
    res = [components(l) for l in labs]
    return np.stack([r[0] for r in res]), np.array([len(r[1]) for r in res], np.int32)


def enforce_batch(labs, min_size):
    res = [enforce(l, min_size) for l in labs]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32)
