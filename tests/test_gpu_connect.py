"""Connectivity on label tensors on the MI355X (fast_slic_amd/connect.py, csrc/connect.hip) against the model written from the five
rules (tests/connect_ref.py), with exact equality throughout.  The tile of the union-find is 64 columns x 16 rows and the rank passes
work on chunks of 1024 pixels: the shapes lie below, at and above both.  Blocky and noise maps at every label width, one component
across every tile edge next to a constant map, singletons, chains of unkept components, more than 65535 labels, -1 regions, batches,
more items than a launch has blocks, determinism, a side stream, the engine's host entry and the chain soft_slic -> soft_labels -> enforce_connectivity -> superpixel_pool."""
import functools

import numpy as np
import pytest
import torch

import connect_ref as R
from fast_slic_amd.connect import connected_components, enforce_connectivity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# 64 x 16 tiles: one below, at, one above in both directions; 1024-pixel chunks: (33, 31) = 1023, (16, 64) = 1024, (25, 41) = 1025
SHAPES = [(1, 1), (1, 200), (200, 1), (15, 63), (16, 64), (17, 65), (33, 130), (64, 257), (33, 31), (25, 41)]
DTYPES = [np.int16, np.int32, np.int64]


@functools.lru_cache(maxsize=None)
def case(kind, H, W):
    """(map int32, its components and their count, {min_size: (labels, n)}) of the model, computed once."""
    lab = R.blocky(H, W, 40, seed=H * 1000 + W) if kind == "blocky" else R.noise(H, W, 3, seed=H * 1000 + W + 1)
    comp, leaders, _ = R.components(lab)
    sizes = (0, 1, 2, 7, H * W, H * W + 1)
    return lab, comp, len(leaders), {s: R.enforce(lab, s) for s in sizes}


def check_types(out, n, shape):
    assert out.dtype == torch.int32 and n.dtype == torch.int32 and out.device == DEV and n.device == DEV
    assert tuple(out.shape) == tuple(shape) and tuple(n.shape) == tuple(shape[:-2])


def same(out, n, want, want_n):
    return np.array_equal(out.cpu().numpy(), want) and np.array_equal(n.cpu().numpy(), np.asarray(want_n, np.int32))


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("kind", ["blocky", "noise"])
def test_components_and_labels_equal_the_model(kind, H, W):
    lab, comp, ncomp, merged = case(kind, H, W)
    for dtype in DTYPES:
        t = torch.from_numpy(lab.astype(dtype)).to(DEV)
        c, n = connected_components(t)
        check_types(c, n, (H, W))
        assert same(c, n, comp, ncomp), (kind, H, W, dtype)
        assert int(c.max()) + 1 == int(n)
        for size, (want, want_n) in merged.items():
            out, n = enforce_connectivity(t, size)
            check_types(out, n, (H, W))
            assert same(out, n, want, want_n), (kind, H, W, dtype, size)
    out, n = enforce_connectivity(lab, 7, device=DEV)                    # a numpy map is uploaded
    assert same(out, n, *merged[7])


def comb(H, W):
    """Row 0 joins the even columns into one component that crosses every tile edge; every odd column below it is a component."""
    lab = np.zeros((H, W), np.int32)
    lab[1:, 1::2] = 1
    return lab


def serpentine(H, W):
    """Label 1: the even rows, joined at alternating ends: one component that winds through every tile, leader (0, 0)."""
    lab = np.zeros((H, W), np.int32)
    lab[0::2] = 1
    lab[1::4, W - 1] = 1
    lab[3::4, 0] = 1
    return lab


def test_one_component_across_every_seam_next_to_a_constant_map():
    H, W = 70, 200
    maps = np.stack([comb(H, W), np.full((H, W), 7, np.int32), serpentine(H, W)])
    comp, ncomp = R.components_batch(maps)
    assert list(ncomp) == [1 + W // 2, 1, 1 + H // 2]
    c, n = connected_components(torch.from_numpy(maps).to(DEV))
    check_types(c, n, maps.shape)
    assert same(c, n, comp, ncomp)
    for size in (0, H - 1, H, W, H * W, H * W + 1):                      # an odd column of the comb has H - 1 pixels
        out, n = enforce_connectivity(torch.from_numpy(maps).to(DEV), size)
        assert same(out, n, *R.enforce_batch(maps, size)), size
    big = np.full((130, 300), -5, np.int64)                              # 27 tiles: the areas of a constant map meet at one leader
    out, n = enforce_connectivity(big, 130 * 300)
    assert same(out, n, np.zeros((130, 300), np.int32), 1) and same(*connected_components(big), np.zeros((130, 300), np.int32), 1)


def test_all_singletons_merge_into_one():
    H, W = 96, 200
    y, x = np.mgrid[0:H, 0:W]
    for lab in (np.arange(H * W, dtype=np.int32).reshape(H, W), ((x + 2 * y) % 5).astype(np.int16)):
        assert (lab[:, 1:] != lab[:, :-1]).all() and (lab[1:] != lab[:-1]).all()
        out, n = enforce_connectivity(torch.from_numpy(lab).to(DEV), 2)
        assert same(out, n, np.zeros((H, W), np.int32), 1)                # every chain ends at component 0
        c, n = connected_components(torch.from_numpy(lab).to(DEV))
        assert same(c, n, np.arange(H * W, dtype=np.int32).reshape(H, W), H * W)


def test_staircase_of_unkept_components():
    """Singletons everywhere but one 3 x 3 block in a corner: a pixel's chain runs left to column 0 and up (or along row 0) to the
    block, or to component 0, across tile edges; each component adopts from the next."""
    H, W = 70, 150
    for by, bx in ((0, 0), (0, W - 3), (H - 3, 0), (40, 70)):
        lab = np.arange(H * W, dtype=np.int32).reshape(H, W)
        lab[by:by + 3, bx:bx + 3] = -1
        want, want_n = R.enforce(lab, 9)
        assert want_n == 1
        out, n = enforce_connectivity(torch.from_numpy(lab).to(DEV), 9)
        assert same(out, n, want, want_n), (by, bx)
    # steps of two pixels going down and right, a kept block at the far (upper left) end: 2 x 2 at (0, 0)
    lab = np.arange(H * W, dtype=np.int32).reshape(H, W) + 10
    lab[0:2, 0:2] = 1
    lab[30:60, 100:140] = 2                                              # a second kept component in the way of some chains
    for size in (3, 4, 5):
        out, n = enforce_connectivity(torch.from_numpy(lab).to(DEV), size)
        want, want_n = R.enforce(lab, size)
        assert want_n == (2 if size <= 4 else 1) and same(out, n, want, want_n), size


def test_more_than_65535_kept_components():
    H, W = 260, 256
    lab = torch.arange(H * W, dtype=torch.int32, device=DEV).view(H, W) * 3 - 70000
    want = np.arange(H * W, dtype=np.int32).reshape(H, W)
    for size in (0, 1):
        out, n = enforce_connectivity(lab, size)
        assert same(out, n, want, H * W) and int(out.max()) == 66559
    assert same(*connected_components(lab), want, H * W)


def test_more_items_than_blocks_in_a_launch():
    """A launch has at most 8192 blocks: 8200 frames are 8200 tiles, 8200 chunks and 8200 scans, so every kernel goes round its loop
    a second time (and a block's LDS serves a second tile); a frame of 260 chunks takes the scan of the chunk counts past its 256."""
    N, H, W = 8200, 3, 5
    maps = np.random.default_rng(11).integers(0, 2, (N, H, W)).astype(np.int16)
    t = torch.from_numpy(maps).to(DEV)
    assert same(*connected_components(t), *R.components_batch(maps))
    want, want_n = R.enforce_batch(maps, 3)
    assert len(set(want_n.tolist())) > 2 and same(*enforce_connectivity(t, 3), want, want_n)
    H, W = 300, 900                                                      # 264 chunks of 1024 pixels
    lab = R.noise(H, W, 3, seed=17)
    comp, leaders, _ = R.components(lab)
    t = torch.from_numpy(lab).to(DEV)
    assert same(*connected_components(t), comp, len(leaders))
    assert same(*enforce_connectivity(t, 5), *R.enforce(lab, 5))


def test_min_size_above_the_frame():
    lab, _, _, merged = case("blocky", 33, 130)
    t = torch.from_numpy(lab).to(DEV)
    for size in (33 * 130 + 1, 1 << 31, 1 << 40, 10 ** 30):
        assert same(*enforce_connectivity(t, size), np.zeros((33, 130), np.int32), 1)
    assert same(*enforce_connectivity(t, 33 * 130), *merged[33 * 130])


def test_minus_one_regions():
    lab, _, _, _ = case("blocky", 64, 257)
    for dtype in DTYPES:
        m = lab.astype(dtype)
        m[10:40, 50:200] = -1
        m[5, :] = -1
        m[m == 3] = -1
        comp, leaders, _ = R.components(m)
        assert same(*connected_components(torch.from_numpy(m).to(DEV)), comp, len(leaders))
        assert same(*enforce_connectivity(torch.from_numpy(m).to(DEV), 12), *R.enforce(m, 12))
    u = lab.astype(np.uint16)                                            # a numpy uint16 map is read like the int16 one
    u[20:30] = 0xFFFF
    assert same(*enforce_connectivity(u, 12, device=DEV), *R.enforce(u, 12))


def test_batch_equals_frame_by_frame():
    H, W = 33, 130
    maps = np.stack([case("blocky", H, W)[0], case("noise", H, W)[0], comb(H, W)])
    t = torch.from_numpy(maps).to(DEV)
    for size in (0, 5, 32):
        out, n = enforce_connectivity(t, size)
        check_types(out, n, (3, H, W))
        want, want_n = R.enforce_batch(maps, size)
        assert len(set(want_n.tolist())) == 3 and same(out, n, want, want_n)
        for i in (2, 0, 1):
            oi, ni = enforce_connectivity(t[i], size)
            assert torch.equal(oi, out[i]) and torch.equal(ni, n[i])
        back, nb = enforce_connectivity(t.flip(0), size)                 # the position in the batch changes nothing
        assert torch.equal(back.flip(0), out) and torch.equal(nb.flip(0), n)
    c, n = connected_components(t)
    want, want_n = R.components_batch(maps)
    assert same(c, n, want, want_n) and torch.equal(c.amax(dim=(1, 2)) + 1, n)


def test_determinism_and_input_untouched():
    maps = np.stack([case("noise", 64, 257)[0], case("blocky", 64, 257)[0]])
    t = torch.from_numpy(maps).to(DEV)
    keep = t.clone()
    first = [enforce_connectivity(t, 6), connected_components(t)]
    for _ in range(4):
        again = [enforce_connectivity(t, 6), connected_components(t)]
        assert all(torch.equal(a, b) for x, y in zip(first, again) for a, b in zip(x, y))
    assert torch.equal(t, keep)
    assert same(*first[0], *R.enforce_batch(maps, 6))


def test_side_stream():
    lab, comp, ncomp, merged = case("noise", 64, 257)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        t = torch.from_numpy(lab).to(DEV, non_blocking=True)
        out, n = enforce_connectivity(t, 7)
        c, nc = connected_components(t)
        again, n2 = enforce_connectivity(out, 7)                         # consumes the first result on the same stream
        s.synchronize()                                                  # this stream only
        assert same(out, n, *merged[7]) and same(c, nc, comp, ncomp)
        assert same(again, n2, *R.enforce(merged[7][0], 7))


def test_agrees_with_the_engine(engine):
    import fast_slic_amd
    from fast_slic_amd.synth import variant
    lab = fast_slic_amd.Slic(num_components=150).iterate(variant("A", 120, 160))
    assert lab.dtype == np.int16 and lab.shape == (120, 160)
    rng = np.random.default_rng(3)
    rough = np.where(rng.random(lab.shape) < 0.03, rng.integers(0, 150, lab.shape), lab).astype(np.int16)      # fragments to merge
    for m in (lab, rough):
        for size in (0, 1, 12, 60, 300):
            want = engine.enforce_connectivity(m.view(np.uint16), 65535, size)      # K above the number of candidates: no cut
            out, n = enforce_connectivity(torch.from_numpy(m).to(DEV), size)
            assert np.array_equal(out.cpu().numpy(), want.astype(np.int32)), size
            assert int(n) == int(want.max()) + 1
    host = fast_slic_amd.enforce_connectivity(lab.copy(), 300)           # K = max label + 1 there: above 120 * 160 // 300, no cut
    assert np.array_equal(enforce_connectivity(lab, 300, device=DEV)[0].cpu().numpy(), host.astype(np.int32))


def test_soft_chain():
    from fast_slic_amd.pool import superpixel_pool
    from fast_slic_amd.soft import soft_labels, soft_slic, with_coords
    N, H, W, grid, min_size = 2, 96, 128, (12, 16), 16
    g = torch.Generator().manual_seed(7)
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = torch.stack([torch.sin(x / 9.0) * torch.cos(y / 7.0), ((x // 5 + y // 3) % 2).float(), torch.sin((x + y) / 4.0)])
    F = (base.unsqueeze(0) * 3.0 + torch.randn(N, 3, H, W, generator=g)).to(DEV)
    q, _ = soft_slic(with_coords(F, grid, 0.3), grid, max_iter=3)
    lab = soft_labels(q, grid)
    out, n = enforce_connectivity(lab, min_size)
    check_types(out, n, (N, H, W))
    labn, outn = lab.cpu().numpy(), out.cpu().numpy()
    assert same(out, n, *R.enforce_batch(labn, min_size))
    for i in range(N):
        comp_in, _, areas_in = R.components(labn[i])
        assert len(areas_in) > grid[0] * grid[1] and (areas_in < min_size).any()        # the argmax map did fragment
        comp, leaders, areas = R.components(outn[i])
        label_of = outn[i].reshape(-1)[leaders]
        # every label is one 4-connected piece of at least min_size pixels; label 0 may hold a small component 0 as a second piece
        pieces = np.bincount(label_of, minlength=int(n[i]))
        assert (pieces[1:] == 1).all() and pieces[0] in (1, 2) and len(pieces) == int(n[i])
        small = areas < min_size
        assert not small[label_of != 0].any() and small.sum() <= 1 and (not small.any() or leaders[small][0] == 0)
        assert int(n[i]) <= H * W // min_size
    v, counts = superpixel_pool(F, out, H * W // min_size, "mean", return_counts=True)
    assert tuple(v.shape) == (N, 3, H * W // min_size)
    assert counts.sum(1).tolist() == [H * W] * N
    assert all(bool((counts[i, :int(n[i])] > 0).all()) and not bool(counts[i, int(n[i]):].any()) for i in range(N))
