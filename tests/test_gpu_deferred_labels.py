"""Label-free subsampled assign passes ("Deferred labels"; group.cpp: enqueue_frames, assign.hip: NOLAB).

A group whose launches leave the fused-bin path stores no labels in its subsampled passes: the full pass at the end writes the
whole plane.  Only a visited pixel that no cluster window covers ever needs the label of an earlier pass; such a frame raises
kFlagUncoveredPixel and is redone with storing passes (Engine.uncovered_redos counts them), and the slot keeps to the storing
passes for that work.  Everything must be the oracle's, bit for bit, on either path.

Small one-frame shapes take the fused cluster pass and never reach this code, so every case here is a multi-frame group sized by
the launch rules of assign.hip (assign_blocks8 > 640 to leave the fused cluster pass, > 2048 for 16 rows per wavefront with the
2-D table, > 3072 with the row-vector table, which tables.cpp builds from S ~ 45 on).  Every case asserts the form it was chosen
for as the LIBRARY recorded it (B.forms_seen, DESIGN.md "The form record"): a rule moved in C++ fails the case instead of silently
exercising another instantiation.  The pre-connectivity plane the library hands out is that of the group's first frame.
"""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as orc
from fast_slic_amd import _binding as B
from fast_slic_amd import make_params
from fast_slic_amd.synth import variant
from util import describe_mismatch, cluster_fields_equal

pytestmark = pytest.mark.gpu


def fused_forms(forms):
    """(table, rows per wavefront, label-free) of the fused passes of the block kernel among recorded form names."""
    out = set()
    for f in forms:
        w = f.split()
        if w[0] == "blk" and w[2] == "fused":
            out.add(("2d" if w[4] in ("2d", "tabs16") else w[4], int(w[1][1:]), w[5] == "nolab"))
    return out


@functools.lru_cache(maxsize=None)
def reference(kind, H, W, K, seed, stride, max_iter, scatter=None, jitter=0):
    """One frame's input and the oracle's results, computed once per distinct frame.  scatter: seed of centres scattered at random
    over the frame (any Cluster block is a legal input, cfast_slic.pyx:94-97); jitter: grid centres moved by up to that many pixels."""
    import ctypes
    img = variant(kind, H, W, seed=seed)
    cl0 = orc.initialize_clusters(img, K)
    if scatter is not None:
        rng = np.random.RandomState(scatter)
        if jitter:
            cl0["y"] = np.clip(cl0["y"] + rng.randint(-jitter, jitter + 1, K), 0, H - 1).astype(np.float32)
            cl0["x"] = np.clip(cl0["x"] + rng.randint(-jitter, jitter + 1, K), 0, W - 1).astype(np.float32)
        else:
            cl0["y"] = rng.randint(0, H, K).astype(np.float32)
            cl0["x"] = rng.randint(0, W, K).astype(np.float32)
    labels, cl, _, pre = orc.slic_iterate(img, cl0.copy(), stages=True, max_iter=max_iter, subsample_stride=stride)
    lib = orc.lib()
    lib.orc_last_stale_pixels.restype = ctypes.c_long
    stale = int(lib.orc_last_stale_pixels())
    for a in (img, cl0, labels, cl, pre):
        a.setflags(write=False)
    return img, cl0, labels, cl, pre, stale


def uncovered_in_some_pass(img, cl0, stride, max_iter):
    """Whether some pass of the call visits a pixel that lies outside every cluster window: pass m (subsampled rows m % stride for
    m < max_iter, every row for the full pass) works on the centres after m updates, which are the oracle's result of max_iter = m."""
    H, W = img.shape[:2]
    K = cl0.shape[0]
    S = orc.S_of(H, W, K)
    for m in range(max_iter + 1):
        cl = cl0 if m == 0 else orc.slic_iterate(img, cl0.copy(), max_iter=m, subsample_stride=stride)[1]
        cy = np.clip(cl["y"].astype(np.int64), 0, H - 1)
        cx = np.clip(cl["x"].astype(np.int64), 0, W - 1)
        cov = np.zeros((H + 1, W + 1), np.int64)
        y0, y1 = np.maximum(cy - S, 0), np.minimum(cy + S, H - 1) + 1
        x0, x1 = np.maximum(cx - S, 0), np.minimum(cx + S, W - 1) + 1
        np.add.at(cov, (y0, x0), 1); np.add.at(cov, (y1, x1), 1)
        np.add.at(cov, (y0, x1), -1); np.add.at(cov, (y1, x0), -1)
        cov = cov.cumsum(0).cumsum(1)[:H, :W]
        rows = slice(m % stride, H, stride) if m < max_iter else slice(0, H)
        if (cov[rows] == 0).any():
            return True
    return False


@pytest.fixture
def eng():
    """A fresh engine per case: its first sighting of a work is enqueued directly, which is when the form record is written (a replay
    of a recorded graph notes nothing), so a case asserts the same whether it runs alone, again or in suite order."""
    from fast_slic_amd import Engine
    e = Engine(0, 2)
    yield e
    e.close()


def run_group(e, refs, stride, max_iter, slot=0):
    """One group of len(refs) frames on `slot` (one launch sequence: submit_group takes up to 16 frames).  Returns the label maps, the
    Cluster blocks, the first frame's pre-connectivity plane and the launch mode."""
    import torch
    H, W = refs[0][0].shape[:2]
    K = refs[0][1].shape[0]
    n = len(refs)
    uniq = {}
    for r in refs:
        uniq.setdefault(id(r[0]), torch.from_numpy(np.array(r[0])).cuda())
    d_lab = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    cls = np.stack([r[1].copy().view(B.CLUSTER_DTYPE) for r in refs])
    torch.cuda.synchronize()
    a = (e.pointer_array([uniq[id(r[0])].data_ptr() for r in refs]),
         e.pointer_array([cls[i].ctypes.data for i in range(n)]),
         e.pointer_array([d_lab[i].data_ptr() for i in range(n)]))
    e.submit_group(slot, a[0], a[1], a[2], n, H, W, K, make_params(max_iter, 10.0, 0.25, stride))
    e.wait_group(slot)
    assert e.last_group_frames(slot) == n
    return d_lab.cpu().numpy().view(np.uint16), cls, e.last_prelabels(H, W, slot), e.last_launch_mode(slot)


def assert_group(tag, got, refs):
    labels, cls, pre, _ = got
    assert np.array_equal(pre, refs[0][4]), describe_mismatch(tag + "/prelabels of frame 0", pre, refs[0][4])
    for i, r in enumerate(refs):
        assert np.array_equal(labels[i], r[2]), describe_mismatch("%s/labels of frame %d" % (tag, i), labels[i], r[2])
        assert cls[i].tobytes() == r[3].tobytes(), "%s frame %d: %s" % (tag, i, "; ".join(cluster_fields_equal(cls[i], r[3])))


def two_images(H, W, K, n, stride, max_iter, scatter=None):
    a = reference("A", H, W, K, 11, stride, max_iter, scatter)
    b = reference("B", H, W, K, 12, stride, max_iter, None if scatter is None else scatter + 1)
    return [a, b] * (n // 2)


# (n, H, W, K): one case per instantiation of the label-free fused pass (table form x rows per wavefront)
SHAPES = {
    "2d_r8": (8, 540, 960, 900),
    "2d_r16": (16, 720, 1280, 1600),      # the launch bench.py times
    "rowvec_r8": (8, 768, 1024, 200),
    "rowvec_r16": (16, 960, 1280, 340),
}
FORMS = {"2d_r8": ("2d", 8), "2d_r16": ("2d", 16), "rowvec_r8": ("rowvec", 8), "rowvec_r16": ("rowvec", 16)}
# every shape at strides 3, 1 and 2 (each stride is an instantiation of its own) with max_iter 10, 1 and 4; max_iter 2 once more
CASES = [(name, st, mi) for name in SHAPES for st, mi in [(3, 10), (1, 1), (2, 4)]] + [("2d_r8", 3, 2)]


@pytest.mark.parametrize("name,stride,max_iter", CASES)
def test_parity_on_covered_inputs(eng, name, stride, max_iter):
    n, H, W, K = SHAPES[name]
    refs = two_images(H, W, K, n, stride, max_iter)
    assert not any((r[4] == 0xFFFF).any() or r[5] for r in refs), "grid-seeded centres were meant to cover every pixel"
    before = eng.uncovered_redos()
    B.forms_seen(clear=True)
    assert_group("%s stride %d max_iter %d" % (name, stride, max_iter), run_group(eng, refs, stride, max_iter), refs)
    forms = B.forms_seen()
    assert eng.uncovered_redos() == before
    # the group's first sighting is enqueued directly: the record is this call's -- label-free fused passes of the case's form alone
    # (the 16-row 2-D form reads its own table, `tabs16`), no cluster pass fused in, and a label-free full pass
    assert fused_forms(forms) == {FORMS[name] + (True,)}, sorted(forms)
    assert ("blk r16 fused s%d tabs16 nolab" % stride in forms) == (FORMS[name] == ("2d", 16)), sorted(forms)
    assert not any(f.startswith("bin") for f in forms) and any(f.startswith("blk") and " full " in f and f.endswith("nolab") for f in forms), sorted(forms)


@pytest.mark.parametrize("name", list(SHAPES))
def test_uncovered_inputs_are_redone_with_storing_passes(name):
    """Centres scattered at random leave visited pixels outside every window (inputs kept by a CPU search: the oracle's plane holds
    0xFFFF or it counted stale pixels): the frames are flagged and redone, everything is the oracle's, and the counter says so."""
    from fast_slic_amd import Engine
    n, H, W, K = SHAPES[name]
    refs = two_images(H, W, K, n, 3, 10, scatter=40)
    assert all((r[4] == 0xFFFF).any() or r[5] > 0 for r in refs), "the inputs were meant to leave uncovered pixels"
    e = Engine(0, 1)
    try:
        assert_group(name + " scattered", run_group(e, refs, 3, 10), refs)
        assert e.uncovered_redos() > 0
        assert e.uncovered_redos(0) == e.uncovered_redos()
    finally:
        e.close()


def test_mixed_group_redoes_exactly_the_uncovered_frames():
    from fast_slic_amd import Engine
    n, H, W, K = SHAPES["2d_r8"]
    stride, max_iter = 3, 4
    s1 = reference("A", H, W, K, 11, stride, max_iter, 50)
    s2 = reference("B", H, W, K, 12, stride, max_iter, 51)
    jit = reference("A", H, W, K, 11, stride, max_iter, 52, 4)      # moved centres that still cover every pixel
    grid = reference("B", H, W, K, 12, stride, max_iter)
    refs = [s1, grid, s2, jit, grid, s1, grid, jit]
    unc = {id(r): uncovered_in_some_pass(r[0], r[1], stride, max_iter) for r in (s1, s2, jit, grid)}
    assert unc[id(s1)] and unc[id(s2)] and not unc[id(grid)] and not unc[id(jit)]
    e = Engine(0, 1)
    try:
        assert_group("mixed", run_group(e, refs, stride, max_iter), refs)
        assert e.uncovered_redos() == sum(unc[id(r)] for r in refs) == 3
    finally:
        e.close()


def test_sticky_fallback_lasts_until_the_work_changes():
    from fast_slic_amd import Engine
    n, H, W, K = SHAPES["2d_r8"]
    stride, max_iter = 3, 4
    scattered = two_images(H, W, K, n, stride, max_iter, scatter=40)
    grid = two_images(H, W, K, n, stride, max_iter)
    e = Engine(0, 1)
    try:
        assert_group("scattered", run_group(e, scattered, stride, max_iter), scattered)
        redone = e.uncovered_redos()
        assert redone > 0
        # the same work on the same slot: storing passes, so even the scattered frames are not computed twice any more
        g2 = run_group(e, grid, stride, max_iter)
        assert_group("same work, grid", g2, grid)
        g3 = run_group(e, scattered, stride, max_iter)
        assert_group("same work, scattered again", g3, scattered)
        assert e.uncovered_redos() == redone
        # the group that caused the fallback counts as the first sighting of the storing sequence: recorded next, then replayed
        assert (g2[3], g3[3]) == (1, 2) or os.environ.get("FSLIC_GRAPH") == "0", (g2[3], g3[3])
        # another work: label-free again -- covered inputs leave the counter alone, scattered ones are found again
        other = two_images(H, W, K + 60, n, stride, max_iter)
        assert_group("other K, grid", run_group(e, other, stride, max_iter), other)
        assert e.uncovered_redos() == redone
        other_s = two_images(H, W, K + 60, n, stride, max_iter, scatter=60)
        assert_group("other K, scattered", run_group(e, other_s, stride, max_iter), other_s)
        assert e.uncovered_redos() > redone
    finally:
        e.close()


def test_three_sightings_direct_recorded_replayed():
    from fast_slic_amd import Engine
    n, H, W, K = SHAPES["2d_r8"]
    refs = two_images(H, W, K, n, 3, 10)
    e = Engine(0, 1)
    try:
        outs = [run_group(e, refs, 3, 10) for _ in range(3)]
        for o in outs:
            assert_group("sighting", o, refs)
            assert np.array_equal(o[0], outs[0][0]) and o[1].tobytes() == outs[0][1].tobytes() and np.array_equal(o[2], outs[0][2])
        modes = [o[3] for o in outs]
        assert modes == [0, 1, 2] or os.environ.get("FSLIC_GRAPH") == "0", modes
        assert e.uncovered_redos() == 0
    finally:
        e.close()


def test_arena_reuse_leaves_no_foreign_label_in_the_plane():
    """A scattered group fills the plane with labels of its K (and 0xFFFF); a covered label-free group of another geometry of the same
    size follows on the same slot and writes its plane in the full pass alone.  (Stride 1: the rows of a 200-row frame are too few
    blocks for these launches otherwise.)"""
    from fast_slic_amd import Engine
    stride, max_iter = 1, 3
    H1, W1, K1 = 200, 448, 90
    H2, W2, K2 = 192, 464, 60
    first = two_images(H1, W1, K1, 16, stride, max_iter, scatter=70)
    assert all((r[4] == 0xFFFF).any() or r[5] > 0 for r in first)
    second = two_images(H2, W2, K2, 16, stride, max_iter)
    e = Engine(0, 1)
    try:
        B.forms_seen(clear=True)
        assert_group("scattered 200x448", run_group(e, first, stride, max_iter), first)
        # (the group left the fused cluster pass and tried the label-free passes first, then was redone with storing ones)
        assert fused_forms(B.forms_seen()) == {("2d", 8, True), ("2d", 8, False)}, sorted(B.forms_seen())
        assert e.uncovered_redos() > 0
        B.forms_seen(clear=True)
        got = run_group(e, second, stride, max_iter)
        assert fused_forms(B.forms_seen()) == {("2d", 8, True)}, "the covered group was meant to take the label-free passes"
        pre = got[2]
        assert not ((pre >= K2) & (pre != 0xFFFF)).any(), "labels of the previous geometry in the plane"
        assert_group("covered 192x464", got, second)
    finally:
        e.close()
