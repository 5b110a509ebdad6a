"""The connectivity pass on maps full of fragments: components the tile kernel resolves in LDS without giving them a node
(closed small components, fast_slic_amd/csrc/cca.hip) next to ones that look like them but must stay nodes.

Every case compares the device pass bit for bit with oracle.enforce_connectivity (the CPU port that tests/test_oracle.py pins to
the compiled reference), and the number of nodes the device kept with the plain CPU restatement of the rule
(scripts/cca_closed_small.py: tile components minus the closed small ones).  A map that the pass leaves unchanged would test
nothing, so every case also asserts that the expected output differs from the input."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("cca_closed_small", os.path.join(ROOT, "scripts", "cca_closed_small.py"))
closed_small = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(closed_small)

TW, TH = closed_small.TILE_W, closed_small.TILE_H
BH, BW = 24, 40          # the base map's blocks: 960 pixels each, cut by the 64x32 tile grid at varying offsets
FRAG_AREA = 6            # the 2x3 fragments of the cases below
# 0, 1: nothing is small; 2: single pixels only; one below, at and one above a fragment's area; an ordinary threshold; larger than a tile
THRESHOLDS = [0, 1, 2, FRAG_AREA - 1, FRAG_AREA, FRAG_AREA + 1, 240, TW * TH + 1000]
# (H, W): neither a multiple of the tile; both multiples (3 x 3 tiles); smaller than one tile; one tile exactly; narrow and tall
SHAPES = [(203, 331), (96, 192), (20, 50), (32, 64), (150, 70)]


def base_map(H, W):
    nbx = (W + BW - 1) // BW
    y = np.arange(H)[:, None] // BH
    x = np.arange(W)[None, :] // BW
    lab = (y * nbx + x).astype(np.uint16)
    return lab, max(int(lab.max()) + 1, 8)      # (at least 8 labels: the fragments of a small image take the unused ones)


def stamp(lab, y, x, h, w, shift, K):
    """A h x w fragment at (y, x), clipped to the image, labelled `shift` away from what lies under its first pixel."""
    H, W = lab.shape
    if y < 0 or x < 0 or y >= H or x >= W:
        return
    lab[y:y + h, x:x + w] = (int(lab[y, x]) + shift) % K


def tile_edge_offsets():
    # the four corners, the middles of the four edges, and the same one pixel inside
    return [(oy, ox) for oy in (0, 1, 15, TH - 2, TH - 1) for ox in (0, 1, 31, TW - 2, TW - 1) if (oy, ox) != (15, 31)]


def case_tile_edges(H, W, size):
    lab, K = base_map(H, W)
    n = 0
    for ty in range(0, H, TH):
        for tx in range(0, W, TW):
            for oy, ox in tile_edge_offsets():
                n += 1
                if size == 1:
                    stamp(lab, ty + oy, tx + ox, 1, 1, 1 + n % 5, K)
                elif oy in (0, 1, 15) and ox in (0, 1, 31):        # 2x3 fragments that reach from the edge into the tile
                    stamp(lab, ty + oy, tx + ox, 2, 3, 1 + n % 5, K)
                else:                                              # ... and ones that end on the far edges
                    stamp(lab, ty + oy - 1, tx + ox - 2, 2, 3, 1 + n % 5, K)
    return lab, K


def case_image_edges(H, W):
    lab, K = base_map(H, W)
    for x in range(2, W, 5):
        stamp(lab, 0, x, 1, 2, 3, K)
        stamp(lab, H - 1, x, 1, 2, 4, K)
        stamp(lab, max(H - 2, 0), x + 2, 2, 3, 5, K)
    for y in range(2, H, 5):
        stamp(lab, y, 0, 2, 1, 3, K)
        stamp(lab, y, W - 1, 2, 1, 4, K)
        stamp(lab, y + 2, max(W - 3, 0), 2, 3, 5, K)
    return lab, K


def case_row_chains(H, W):
    # every pixel of a chain row is a component of its own that adopts from the one on its left: along the whole row, through the
    # tiles; the two-pixel-tall chains lie across a strip seam (rows 7 | 8 of a tile) and across a tile seam (rows 31 | 32)
    lab, K = base_map(H, W)
    cyc = np.array([K - 1, K - 2, K - 3], np.uint16)
    for y, h in ((3, 1), (7, 2), (12, 1), (TH - 1, 2), (TH + 9, 1), (2 * TH + 15, 2)):
        if y + h > H:
            continue
        xs = np.arange(2, W - 2)
        lab[y:y + h, 2:W - 2] = cyc[(xs + y) % 3][None, :]
    return lab, K


def case_column0_chain(H, W):
    # down image column 0 (adoption from above, through the strips of a tile and from tile to tile), and down the first column of
    # the second tile column (adoption from the left, across the vertical seam)
    lab, K = base_map(H, W)
    cyc = np.array([K - 1, K - 2, K - 3], np.uint16)
    ys = np.arange(1, H)
    lab[1:, 0] = cyc[ys % 3]
    if W > TW + 2:
        lab[1:, TW] = cyc[(ys + 1) % 3]
    # wider chain elements in column 0: their first pixel is in column 0, the rest is not
    for y in range(4, H - 1, 9):
        lab[y, 0:3] = cyc[(y + 2) % 3]
    return lab, K


def case_enclosed(H, W):
    # a fragment inside a fragment inside a fragment: the inner ones adopt from the ring around them, whose first pixel lies above
    # and to the left; placed inside tiles, on tile seams and in the image corner
    lab, K = base_map(H, W)
    for y in range(1, H - 6, 13):
        for x in range(1, W - 6, 17):
            stamp(lab, y, x, 5, 5, 2, K)
            stamp(lab, y + 1, x + 1, 3, 3, 3, K)
            stamp(lab, y + 2, x + 2, 1, 1, 4, K)
    stamp(lab, 0, 0, 5, 5, 2, K)
    stamp(lab, 1, 1, 3, 3, 3, K)
    return lab, K


def case_pixel0_small(H, W):
    # the component of pixel 0 is small and closed, and keeps its node (src/cca.cpp:238); fragments right of and below it adopt from it
    lab, K = base_map(H, W)
    lab[0:2, 0:2] = K - 1
    lab[0, 2:4] = K - 2
    lab[2:4, 0] = K - 3
    lab[1, 2] = K - 4
    return lab, K


def case_span_two_tiles(H, W):
    # components below the threshold that lie across a tile seam (they stay nodes in both tiles), and 2x2 ones on the crossings
    lab, K = base_map(H, W)
    for tx in range(TW, W, TW):
        for y in range(3, H - 2, 7):
            stamp(lab, y, tx - 1, 1, 2, 3, K)
            stamp(lab, y + 3, tx - 2, 2, 3, 4, K)
    for ty in range(TH, H, TH):
        for x in range(3, W - 3, 7):
            stamp(lab, ty - 1, x, 2, 1, 5, K)
            stamp(lab, ty - 1, x + 3, 3, 2, 6, K)
    for ty in range(TH, H, TH):
        for tx in range(TW, W, TW):
            stamp(lab, ty - 1, tx - 1, 2, 2, 7, K)
    if H <= TH and W <= TW:                                    # one tile: no seam; fragments so that the pass still has something to do
        stamp(lab, H // 2, W // 2, 2, 3, 3, K)
    return lab, K


def case_noise(H, W):
    # the node count at its largest
    rng = np.random.default_rng(H * 1000 + W)
    return rng.integers(0, 7, size=(H, W)).astype(np.uint16), 7


CASES = {
    "tile_edges_1px": lambda H, W: case_tile_edges(H, W, 1),
    "tile_edges_2x3": lambda H, W: case_tile_edges(H, W, 6),
    "image_edges": case_image_edges,
    "row_chains": case_row_chains,
    "column0_chain": case_column0_chain,
    "enclosed": case_enclosed,
    "pixel0_small": case_pixel0_small,
    "span_two_tiles": case_span_two_tiles,
    "noise": case_noise,
}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % (s[1], s[0]))
@pytest.mark.parametrize("case", sorted(CASES))
def test_fragments_match_the_reference_and_the_node_rule(engine, case, shape):
    H, W = shape
    lab, K = CASES[case](H, W)
    assert lab.shape == (H, W) and lab.dtype == np.uint16 and int(lab.max()) < K
    for thr in THRESHOLDS:
        exp = orc.enforce_connectivity(lab, K, thr)
        assert not np.array_equal(exp, lab), "%s %dx%d thr %d: the pass leaves the map as it is" % (case, W, H, thr)
        got, nodes = engine.enforce_connectivity_nodes(lab, K, thr)
        want = closed_small.count(lab, thr)
        print("%s %dx%d thr %d: tile components %d, closed small %d, nodes %d (device %d)" % (
            case, W, H, thr, want["tile_nodes"], want["closed_small"], want["nodes_left"], nodes))
        assert nodes == want["nodes_left"], "%s %dx%d thr %d: device kept %d nodes, the rule leaves %d of %d" % (
            case, W, H, thr, nodes, want["nodes_left"], want["tile_nodes"])
        bad = np.argwhere(got != exp)
        assert bad.size == 0, "%s %dx%d thr %d: %d pixels differ, first at (y, x) = %s: got %d, expected %d" % (
            case, W, H, thr, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


def test_cases_contain_what_they_claim():
    """(No GPU work: the fixtures of this file do contain closed small components, chains of them and near misses.)"""
    lab, K = case_row_chains(203, 331)
    c = closed_small.count(lab, 2)
    assert c["closed_small"] > 900                              # three single-pixel chain rows of 327 pixels, minus the pixels on tile seams
    lab, K = case_span_two_tiles(96, 192)
    c1, c2 = closed_small.count(lab, 240), closed_small.count(lab, 240, 10 ** 6, 10 ** 6)
    assert c1["nodes_left"] > c2["tile_nodes"] - c2["closed_small"]      # small components that stay nodes because a seam cuts them
    lab, K = case_pixel0_small(96, 192)
    assert closed_small.count(lab, 240)["closed_small"] == 3    # the three fragments around pixel 0's component, not that one
    lab, K = case_noise(203, 331)
    assert closed_small.count(lab, 1)["closed_small"] == 0 and closed_small.count(lab, 3000)["closed_small"] > 10000
