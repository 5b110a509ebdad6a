"""The comparison of two label maps on the MI355X (fast_slic_amd/compare.py, csrc/compare.hip) against the numpy model
(tests/compare_ref.py), with exact equality throughout -- no tolerance anywhere: the overlap table and the four quantities derived
from it on blocky maps across every tile seam (the overlap kernel's tile is 64 columns x 16 rows), the pair (0, 0), counts beyond 16
bits, labels outside the range at every width, the largest K and M, noise that overflows a tile's lanes and makes the table grow,
batches, determinism, a non-default stream, a Slic map against an LSC map; the boundary match (tile: 64 columns x 32 rows, halo of
`tolerance`) across its seams, at the largest windows, with -1 regions, swapped arguments and against tests/util.py."""
import math

import numpy as np
import pytest
import torch

import compare_ref as R
import util as U
from fast_slic_amd.compare import boundary_match, first_capacity, label_overlap

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def blocky(H, W, K, seed, dtype=np.int32, batch=None):
    """A map of about K labels in blocks a few pixels wide, edges ragged: a tile holds a handful of labels."""
    rng = np.random.default_rng(seed)
    shape = (H, W) if batch is None else (batch, H, W)
    y, x = np.mgrid[0:H, 0:W]
    bh, bw = int(rng.integers(3, 12)), int(rng.integers(5, 40))
    grid = (y // bh) * ((W + bw - 1) // bw) + x // bw
    return ((grid + (rng.random(shape) < 0.05) * rng.integers(0, K, shape)) % K).astype(dtype)


def assert_table(t, ref, K, M, what="", batched=False):
    """Types, device, shapes and every value of an OverlapTable, and of what derives from it, against the model."""
    assert t.pairs.dtype == torch.int64 and t.count.dtype == torch.int32 and t.offsets.dtype == torch.int64, what
    assert t.pairs.device == DEV and t.count.device == DEV and t.offsets.device == DEV, what
    assert t.num_components == K and t.num_other == M, what
    P = ref["pairs"].shape[1]
    assert tuple(t.pairs.shape) == (2, P), "%s: %d pairs, the model has %d" % (what, t.pairs.shape[1], P)
    assert np.array_equal(t.offsets.cpu().numpy(), ref["offsets"]), what + ": offsets"
    assert np.array_equal(t.pairs.cpu().numpy(), ref["pairs"]), what + ": pairs"
    assert np.array_equal(t.count.cpu().numpy(), ref["count"]), what + ": count"
    lead = (lambda a: a) if batched else (lambda a: a[0])
    A, Bm = t.areas()
    rA, rB = R.areas(ref, K, M)
    assert A.dtype == torch.int64 and Bm.dtype == torch.int64 and A.device == DEV, what
    assert np.array_equal(A.cpu().numpy(), lead(rA)) and np.array_equal(Bm.cpu().numpy(), lead(rB)), what + ": areas"
    maj = t.majority()
    assert maj.dtype == torch.int64 and np.array_equal(maj.cpu().numpy(), lead(R.majority(ref, K, M))), what + ": majority"
    for got, want in ((t.best_overlap(), R.best_overlap(ref, K, M)), (t.undersegmentation_error(), R.undersegmentation_error(ref, K, M))):
        assert got.dtype == torch.float64 and got.device == DEV, what
        assert np.array_equal(got.cpu().numpy(), lead(want), equal_nan=True), what + ": ratios"          # bit for bit


def assert_same(a, b):
    assert torch.equal(a.pairs, b.pairs) and torch.equal(a.count, b.count) and torch.equal(a.offsets, b.offsets)


# ---- overlap: seams and edges ----
@pytest.mark.parametrize("H,W", [(1, 1), (1, 200), (200, 1), (16, 64), (17, 65), (33, 130), (15, 63)])
def test_overlap_across_the_tile_seams(H, W):
    for K, M, seed in ((5, 40, 1), (40, 7, 2), (23, 23, 3)):
        la, ot = blocky(H, W, K, seed * 1000 + H + W), blocky(H, W, M, seed * 2000 + H + W)
        ref = R.overlap(la, ot, K, M)
        for da, db in ((np.int16, np.int16), (np.int32, np.int64), (np.int64, np.int16)):
            t = label_overlap(torch.from_numpy(la.astype(da)).to(DEV), torch.from_numpy(ot.astype(db)).to(DEV), K, M)
            assert_table(t, ref, K, M, "%dx%d K=%d M=%d %s x %s" % (H, W, K, M, da.__name__, db.__name__))
            assert int(t.count.sum()) == H * W and t.capacity == first_capacity(K, M)


def test_all_zero_maps_give_the_pair_zero_zero():
    z = np.zeros((40, 70), np.int16)
    t = label_overlap(z, z, 1, 1)
    assert t.pairs.tolist() == [[0], [0]] and t.count.tolist() == [2800] and t.offsets.tolist() == [0, 1]
    assert_table(t, R.overlap(z, z, 1, 1), 1, 1, "zeros")
    assert t.majority().tolist() == [0] and t.best_overlap().item() == 1.0 and t.undersegmentation_error().item() == 0.0


def test_constant_maps_count_beyond_16_bits():
    la = torch.full((512, 512), 7, dtype=torch.int16, device=DEV)
    ot = torch.full((512, 512), 300, dtype=torch.int32, device=DEV)
    t = label_overlap(la, ot, 8, 301)
    assert t.pairs.tolist() == [[7], [300]] and t.count.tolist() == [262144] and t.offsets.tolist() == [0, 1]
    a, b = t.areas()
    assert a.tolist() == [0] * 7 + [262144] and int(b[300]) == 262144 and int(b.sum()) == 262144
    assert t.majority().tolist() == [-1] * 7 + [300]


# ---- labels outside the range ----
def holes(shape, seed):
    r = np.random.default_rng(seed).random(shape)
    return r < 0.05, r > 0.95, (r * 1e4).astype(np.int64) % 3                  # where below, where above, which of three values


def test_labels_outside_the_range_at_every_width():
    H, W, K, M = 33, 130, 21, 9
    la, ot = blocky(H, W, K, 5, np.int64), blocky(H, W, M, 6, np.int64)
    la_below, la_above, pick = holes((H, W), 7)
    ot_below, ot_above, opick = holes((H, W), 8)
    mask_a, mask_b = np.where(la_below | la_above, -1, la), np.where(ot_below | ot_above, -1, ot)
    ref = R.overlap(mask_a, mask_b, K, M)
    assert 0 < ref["count"].sum() < H * W and ref["count"].sum() == ((mask_a >= 0) & (mask_b >= 0)).sum()

    def with_holes(m, below, above, pk, dtype, lows, highs):
        out = m.astype(dtype)
        out[below] = np.array(lows, dtype)[pk[below]]
        out[above] = np.array(highs, dtype)[pk[above]]
        return out
    # int16: -1 and values >= K; int32: negatives and 1 << 16 (label 0 in its low 16 bits); int64: K + 2^32, -2^63, 2^32 + 1
    a16 = with_holes(la, la_below, la_above, pick, np.int16, [-1, -2, -32768], [K, K + 5, 32767])
    b16 = with_holes(ot, ot_below, ot_above, opick, np.int16, [-1, -3, -32768], [M, M + 1, 32767])
    a32 = with_holes(la, la_below, la_above, pick, np.int32, [-1, -(1 << 31), -65536], [K, (1 << 31) - 1, 1 << 16])
    b32 = with_holes(ot, ot_below, ot_above, opick, np.int32, [-1, -(1 << 31), -65535], [M, (1 << 31) - 1, (1 << 16) + 1])
    a64 = with_holes(la, la_below, la_above, pick, np.int64, [-1, -(1 << 63), -(1 << 32)], [K + (1 << 32), (1 << 32) + 1, 1 << 16])
    b64 = with_holes(ot, ot_below, ot_above, opick, np.int64, [-1, -(1 << 63), -(1 << 40)], [M + (1 << 32), (1 << 32) + 1, 1 << 32])
    for name, a, b in (("int16", a16, b16), ("int32", a32, b32), ("int64", a64, b64), ("int16 x int64", a16, b64), ("int64 x int32", a64, b32)):
        assert np.array_equal(R.overlap(a, b, K, M)["count"], ref["count"]), name            # (the model reads the holes alike)
        assert_table(label_overlap(a, b, K, M), ref, K, M, name + ", numpy")
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        keep_a, keep_b = ta.clone(), tb.clone()
        assert_table(label_overlap(ta, tb, K, M), ref, K, M, name + ", torch")
        assert torch.equal(ta, keep_a) and torch.equal(tb, keep_b)                           # the inputs are unchanged
    assert_table(label_overlap(a16.view(np.uint16), tb, K, M), ref, K, M, "uint16 view x torch int32")


def test_a_frame_without_a_valid_pixel():
    H, W, K, M = 17, 65, 6, 5
    la = blocky(H, W, K, 9, np.int16, batch=3)
    ot = blocky(H, W, M, 10, np.int64, batch=3)
    la[1] = -1
    ot[1, ::2] = M + (1 << 32)
    ref = R.overlap(la, ot, K, M)
    assert ref["offsets"][1] == ref["offsets"][2] and 0 < ref["offsets"][1] < ref["offsets"][3]
    t = label_overlap(la, ot, K, M)
    assert_table(t, ref, K, M, "batch with an empty frame", batched=True)
    assert t.majority()[1].tolist() == [-1] * K and math.isnan(t.best_overlap()[1]) and math.isnan(t.undersegmentation_error()[1])
    assert not math.isnan(t.best_overlap()[0]) and not math.isnan(t.best_overlap()[2])
    assert int(t.count.sum()) == 2 * H * W


def test_largest_label_counts():
    K = M = 65534
    la = blocky(8, 8, 3, 11, np.int32) * 30000                                  # 0, 30000, 60000
    ot = blocky(8, 8, 2, 12, np.int32) * 65533
    la[0, 0], la[7, 7], ot[0, 0], ot[7, 7], ot[3, 3] = 65533, 0, 65533, 0, 65534
    la[4, 4] = 65534                                                            # K itself: no label
    ref = R.overlap(la, ot, K, M)
    assert ref["count"].sum() == 62 and [65533, 65533] in ref["pairs"].T.tolist() and [0, 0] in ref["pairs"].T.tolist()
    for dtype in (np.int32, np.int64):
        assert_table(label_overlap(la.astype(dtype), ot.astype(dtype), K, M), ref, K, M, dtype.__name__)
    a16, b16 = la.astype(np.uint16).view(np.int16), ot.astype(np.uint16).view(np.int16)     # Slic's map type holds them as negatives
    assert_table(label_overlap(a16, b16, K, M), ref, K, M, "int16")


# ---- noise: more distinct pairs a tile than its lanes hold; growth of the table ----
def test_noise_takes_the_direct_path_and_grows_the_table():
    rng = np.random.default_rng(13)
    la = rng.integers(0, 300, (48, 130)).astype(np.int32)
    ot = rng.integers(0, 300, (48, 130)).astype(np.int32)
    # the labels are below 300; K = M = 2048 sizes the first table (32768 slots) past what these maps need, so that the default
    # and the grown table differ in size
    K = M = 2048
    ref = R.overlap(la, ot, K, M)
    P = ref["pairs"].shape[1]
    assert P > 5000 and P > 64 * 2 * 3                                          # far more than 64 distinct pairs in each of the 9 tiles
    t = label_overlap(la, ot, K, M)
    assert_table(t, ref, K, M, "default capacity")
    assert t.capacity == first_capacity(K, M) == 32768
    g = label_overlap(la, ot, K, M, _start_capacity=64)
    assert_table(g, ref, K, M, "grown from 64 slots")
    assert 64 < g.capacity and 2 * P <= g.capacity < t.capacity
    assert_same(t, g)
    assert_table(label_overlap(la, ot, 300, 300), R.overlap(la, ot, 300, 300), 300, 300, "K = M = 300: the default table grows too")


# ---- batch, determinism, streams ----
def test_batch_equals_the_single_calls_and_two_calls_are_bitwise_equal():
    H, W, K, M = 33, 130, 30, 12
    la, ot = blocky(H, W, K, 14, np.int16, batch=3), blocky(H, W, M, 15, np.int32, batch=3)
    la[2, 5:9] = -1
    assert len({la[n].tobytes() for n in range(3)}) == 3
    dla, dot = torch.from_numpy(la).to(DEV), torch.from_numpy(ot).to(DEV)
    t = label_overlap(dla, dot, K, M)
    assert_table(t, R.overlap(la, ot, K, M), K, M, "batch", batched=True)
    assert_same(t, label_overlap(dla, dot, K, M))
    assert int(t.count.sum()) == int(((la >= 0) & (la < K) & (ot >= 0) & (ot < M)).sum())
    off = t.offsets.tolist()
    A, Bm = t.areas()
    for n in range(3):
        one = label_overlap(la[n], ot[n], K, M)
        assert torch.equal(t.pairs[:, off[n]:off[n + 1]], one.pairs) and torch.equal(t.count[off[n]:off[n + 1]], one.count)
        assert one.offsets.tolist() == [0, off[n + 1] - off[n]]
        assert torch.equal(one.majority(), t.majority()[n]) and torch.equal(one.best_overlap(), t.best_overlap()[n])
        assert torch.equal(one.areas()[0], A[n]) and torch.equal(one.areas()[1], Bm[n])
        assert torch.equal(one.undersegmentation_error(), t.undersegmentation_error()[n])


def test_majority_tie_takes_the_smallest_label():
    la = np.zeros((20, 128), np.int16)
    ot = np.zeros((20, 128), np.int16)
    ot[:, :32], ot[:, 32:64], ot[:, 64:96], ot[:, 96:] = 4, 2, 9, 2             # b = 2: 1280 pixels; b = 4 and b = 9: 640 each
    la[:, 64:] = 1                                                              # a = 0: 4 and 2 tie at 640; a = 1: 9 and 2 tie at 640
    t = label_overlap(la, ot, 3, 10)
    assert t.pairs.tolist() == [[0, 0, 1, 1], [2, 4, 2, 9]] and t.count.tolist() == [640] * 4
    assert t.majority().tolist() == [2, 2, -1] and t.best_overlap().item() == 0.5 and t.undersegmentation_error().item() == 1.0
    assert_table(t, R.overlap(la, ot, 3, 10), 3, 10, "tie")


def test_on_a_non_default_stream():
    H, W, K, M = 40, 150, 17, 11
    la, ot = blocky(H, W, K, 16, np.int16), blocky(H, W, M, 17, np.int16)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(DEV)
    with torch.cuda.stream(st):
        a, b = torch.from_numpy(la).to(DEV).clone(), torch.from_numpy(ot).to(DEV).clone()              # produced on st
        t = label_overlap(a, b, K, M)
        m = boundary_match(a, b, 3)
        bo = t.best_overlap()
    st.synchronize()
    assert_table(t, R.overlap(la, ot, K, M), K, M, "stream")
    assert m.tolist() == R.boundary_match(la, ot, 3).tolist() and bo.item() == R.best_overlap(R.overlap(la, ot, K, M), K, M)[0]


# ---- one real pair of maps ----
_maps = {}


def real_maps():
    if not _maps:
        from fast_slic_amd import LSC, Slic
        from fast_slic_amd.synth import variant
        img = variant("A", 240, 320)
        _maps["slic"], _maps["lsc"] = Slic(num_components=200).iterate(img), LSC(num_components=200).iterate(img)
    return _maps["slic"], _maps["lsc"]


def test_slic_against_lsc():
    la, ot = real_maps()
    ref = R.overlap(la, ot, 200, 200)
    t = label_overlap(la, ot, 200, 200)
    assert_table(t, ref, 200, 200, "Slic x LSC")
    assert t.capacity == first_capacity(200, 200)                               # two Slic-like maps: the first table holds them
    if la.min() >= 0 and ot.min() >= 0:
        assert t.best_overlap().item() == U.best_overlap(la, ot)
    for tol in (0, 2):
        m = boundary_match(la, ot, tol)
        assert m.tolist() == R.boundary_match(la, ot, tol).tolist()
    hits, nother, nlabels = boundary_match(la, ot).tolist()
    assert hits / max(1, nother + nlabels - hits) == U.boundary_iou(la, ot)


# ---- boundary match ----
MATCH_SHAPES = [(17, 65), (40, 150), (33, 130), (3, 3), (1, 50)]
TOLERANCES = [0, 1, 3, 15]


def match_maps(H, W, seed, batch=None):
    """Two blocky maps; the first is Slic's type with a region of -1."""
    la, ot = blocky(H, W, 9, seed, np.int16, batch), blocky(H, W, 6, seed + 1, np.int32, batch)
    la[..., H // 3:H // 2 + 1, W // 4:W // 2 + 1] = -1
    return la, ot


@pytest.mark.parametrize("H,W", MATCH_SHAPES)
def test_boundary_match_against_the_model(H, W):
    la3, ot3 = match_maps(H, W, 20 + H, batch=3)
    dla, dot = torch.from_numpy(la3).to(DEV), torch.from_numpy(ot3).to(DEV)
    for tol in TOLERANCES:
        want = R.boundary_match(la3, ot3, tol)
        got = boundary_match(dla, dot, tol)
        assert got.dtype == torch.int64 and got.device == DEV and tuple(got.shape) == (3, 3)
        assert got.tolist() == want.tolist(), "batch, tolerance %d" % tol
        assert torch.equal(got, boundary_match(dla, dot, tol))                  # two calls, bitwise
        swapped = boundary_match(dot, dla, tol)
        assert swapped.tolist() == R.boundary_match(ot3, la3, tol).tolist(), "swapped, tolerance %d" % tol
        assert swapped[:, 1].tolist() == got[:, 2].tolist() and swapped[:, 2].tolist() == got[:, 1].tolist()
        one = boundary_match(la3[1], ot3[1], tol)                               # a single frame, numpy
        assert tuple(one.shape) == (3,) and one.tolist() == want[1].tolist(), "single, tolerance %d" % tol
        for dtype in (np.int32, np.int64):
            assert boundary_match(la3.astype(dtype), ot3.astype(np.int64), tol).tolist() == want.tolist(), dtype.__name__
    hits, nother, nlabels = boundary_match(la3[0], ot3[0]).tolist()
    assert hits / max(1, nother + nlabels - hits) == U.boundary_iou(la3[0], ot3[0])
    assert hits <= min(nother, nlabels) and (H * W < 10 or nother > 0)


def chebyshev_threshold(ml, mo):
    """For every boundary pixel of `other` the distance to the nearest boundary pixel of `labels`, ascending."""
    pl, po = np.argwhere(ml), np.argwhere(mo)
    return sorted(int(np.abs(pl - q).max(1).min()) for q in po)


@pytest.mark.parametrize("H,W", [(12, 14), (16, 10), (3, 17), (17, 65), (40, 150)])
def test_lone_boundary_pixels_at_opposite_corners(H, W):
    """labels' only boundary pixel is (0, 0).  No map has (H - 2, W - 2) as its only boundary pixel (its right and lower neighbours
    would have to differ from it and from each other's neighbours alike); the nearest thing is a map whose one differing pixel is the
    corner (H - 1, W - 1): its boundary pixels are (H - 1, W - 2) and (H - 2, W - 1).  hits turns from 0 to 1 to 2 exactly at the
    tolerances the model names, max(H - 1, W - 2) and max(H - 2, W - 1), or stays 0 where they are beyond 15."""
    la = np.ones((H, W), np.int16)
    la[0, 0] = -1
    ot = np.zeros((H, W), np.int64)
    ot[H - 1, W - 1] = 1
    ml, mo = U.boundary_mask(la), U.boundary_mask(ot)
    assert ml.sum() == 1 and ml[0, 0] and mo.sum() == 2 and mo[H - 1, W - 2] and mo[H - 2, W - 1]
    dist = chebyshev_threshold(ml, mo)
    assert dist == sorted([max(H - 1, W - 2), max(H - 2, W - 1)])
    for tol in range(16):
        got = boundary_match(la, ot, tol).tolist()
        assert got == R.boundary_match(la, ot, tol).tolist() and got == [sum(d <= tol for d in dist), 2, 1], tol
        assert boundary_match(ot, la, tol).tolist() == [int(dist[0] <= tol), 1, 2], tol


def test_lone_pixels_across_the_tile_seams():
    """One differing pixel in either map, on either side of the seams at column 64 and row 32: every tolerance from 0 to 15."""
    H, W = 70, 200
    for (ya, xa), (yb, xb) in (((30, 60), (36, 70)), ((33, 66), (29, 55)), ((31, 63), (32, 64)), ((40, 127), (40, 142)), ((2, 3), (17, 3))):
        la, ot = np.zeros((H, W), np.int32), np.zeros((H, W), np.int16)
        la[ya, xa], ot[yb, xb] = 7, -1
        dist = chebyshev_threshold(U.boundary_mask(la), U.boundary_mask(ot))
        assert len(dist) == 3 and 0 < dist[-1] <= 16
        for tol in range(16):
            got = boundary_match(la, ot, tol).tolist()
            assert got == R.boundary_match(la, ot, tol).tolist() and got == [sum(d <= tol for d in dist), 3, 3], ((ya, xa), (yb, xb), tol)


def test_boundaries_on_the_tile_seams():
    """Boundaries at columns 63 | 64 and rows 15 | 16 and 31 | 32: a hit needs the neighbouring tile's bits."""
    H, W = 70, 200
    y, x = np.mgrid[0:H, 0:W]
    la = ((x >= 64).astype(np.int16) + 2 * (y >= 32) + 4 * (x >= 128)).astype(np.int16)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (0, -1), (-1, 0), (2, 3), (-3, -2), (15, 15), (-15, -15), (16, 0), (0, 16)):
        ot = ((x >= 64 + dx).astype(np.int32) + 2 * (y >= 32 + dy) + 4 * (x >= 128 + dx) + 8 * (y >= 16 + dy))
        for tol in TOLERANCES:
            assert boundary_match(la, ot, tol).tolist() == R.boundary_match(la, ot, tol).tolist(), (dy, dx, tol)
    ot = ((x >= 64 + 2).astype(np.int32) + 2 * (y >= 32 - 3))
    assert boundary_match(la, ot, 2).tolist()[0] < boundary_match(la, ot, 3).tolist()[0]        # (the tolerance matters here)
