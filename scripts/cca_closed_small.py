"""How many of the connectivity pass's tile components need no node (CPU only).

    python scripts/cca_closed_small.py W H K [seed ...]        # e.g. 1280 720 1600 0 1

The device pass (fast_slic_amd/csrc/cca.hip) cuts the label map into 64x32 tiles; a component of a tile is CLOSED SMALL when
  1. none of its pixels lies on a tile edge that has a neighbouring tile across it (it is a whole component of the frame),
  2. its area is below the threshold (it can never be one of the kept components, src/cca.cpp:213-217), and
  3. its first pixel in raster order is not pixel 0 (src/cca.cpp:238).
Such a component only ever takes the final label of the component left of (image column 0: above) its first pixel, and that pixel
lies in the same tile, so k_cca_local resolves it in LDS and gives it no node.  This file restates the rule with a plain union-find;
tests/test_gpu_cca_fragments.py compares the device's node count with `count(...)["nodes_left"]`.

The frames are the benchmark's (synth.variant("A")), the label map is the one before connectivity (oracle.slic_iterate(...,
stages=True)), the threshold int(0.25 * H * W / K).
"""
import os
import sys

import numpy as np

TILE_W, TILE_H = 64, 32


def components(lab, tw=None, th=None):
    """4-connected components of equal labels, cut at the tile grid (tw, th) when given.
    Returns (comp, area, leader): per pixel the component's number (numbered in raster order of the first pixels), per component
    its area and the raster index of its first pixel."""
    lab = np.ascontiguousarray(lab)
    H, W = lab.shape
    start = np.ones((H, W), bool)
    start[:, 1:] = lab[:, 1:] != lab[:, :-1]
    if tw:
        start[:, ::tw] = True
    run = (np.cumsum(start.ravel()) - 1).reshape(H, W)          # runs in raster order
    nrun = int(run[-1, -1]) + 1
    same = lab[1:] == lab[:-1]
    if th:
        same[th - 1::th] = False                                # no contact across a horizontal tile edge
    pairs = np.unique(np.stack([run[1:][same], run[:-1][same]], axis=1), axis=0)
    parent = list(range(nrun))
    for a, b in pairs.tolist():                                 # plain union-find; the smaller run (earlier first pixel) becomes the root
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b
    parent = np.asarray(parent, np.int64)
    while True:
        nxt = parent[parent]
        if np.array_equal(nxt, parent):
            break
        parent = nxt
    roots, dense = np.unique(parent, return_inverse=True)
    comp = dense[run]
    area = np.bincount(comp.ravel(), minlength=roots.size)
    leader = np.flatnonzero(start.ravel())[roots]
    return comp, area, leader


def count(lab, threshold, tw=TILE_W, th=TILE_H):
    """The table's columns for one label map."""
    H, W = lab.shape
    _, area, _ = components(lab)
    comp, tarea, tleader = components(lab, tw, th)
    y = np.arange(H)[:, None]
    x = np.arange(W)[None, :]
    on_open_edge = ((x % tw == 0) & (x > 0)) | ((x % tw == tw - 1) & (x + 1 < W)) | ((y % th == 0) & (y > 0)) | ((y % th == th - 1) & (y + 1 < H))
    is_open = np.bincount(comp.ravel(), weights=on_open_edge.ravel(), minlength=tarea.size) > 0
    closed_small = ~is_open & (tarea < threshold) & (tleader != 0)
    return {"components": int(area.size), "tile_nodes": int(tarea.size), "candidates": int((area >= threshold).sum()),
            "closed_small": int(closed_small.sum()), "nodes_left": int(tarea.size - closed_small.sum())}


def main(argv):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as orc
    from fast_slic_amd.synth import variant
    if len(argv) < 3:
        raise SystemExit(__doc__)
    W, H, K = int(argv[0]), int(argv[1]), int(argv[2])
    seeds = [int(s) for s in argv[3:]] or [0]
    print("| shape | components | tile components | candidates | closed small | nodes left |")
    print("|---|---|---|---|---|---|")
    for seed in seeds:
        img = variant("A", H, W, seed=seed)
        _, _, _, pre = orc.slic_iterate(img, orc.initialize_clusters(img, K), stages=True)
        c = count(pre, int(0.25 * H * W / K))
        print("| %dx%d K=%d, seed %d | %d | %d | %d | %d (%.1f %%) | %d |" % (
            W, H, K, seed, c["components"], c["tile_nodes"], c["candidates"], c["closed_small"],
            100.0 * c["closed_small"] / c["tile_nodes"], c["nodes_left"]))


if __name__ == "__main__":
    main(sys.argv[1:])
