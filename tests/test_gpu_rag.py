"""The region adjacency graph on the MI355X (fast_slic_amd/rag.py, csrc/rag.hip) against the numpy reference (tests/rag_ref.py), with
exact equality throughout: Slic maps, every tile seam (the kernel's tile is 64 columns x 16 rows), labels outside the range, tiny K,
a noise map that makes the pair table grow, batches, determinism, a non-default stream, SlicModel.get_connectivity as a subset, and
the CSR rows through SimpleCRFFrame."""
import numpy as np
import pytest
import torch

import rag_ref as R
from fast_slic_amd.rag import first_capacity, superpixel_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_slic_cache = {}


def slic_case(H, W, K, variant="A", seed=0):
    """(the Slic object, its label map of the synthetic frame, the frame), as test_gpu_pool.slic_labels makes the map."""
    key = (H, W, K, variant, seed)
    if key not in _slic_cache:
        from fast_slic_amd import Slic
        from fast_slic_amd.synth import variant as synth
        frame = synth(variant, H, W, seed=seed)
        slic = Slic(num_components=K)
        _slic_cache[key] = (slic, slic.iterate(frame), frame)
    return _slic_cache[key]


_ref_cache = {}


def slic_ref(H, W, K, connectivity):
    key = (H, W, K, connectivity)
    if key not in _ref_cache:
        _, lab, frame = slic_case(H, W, K)
        _ref_cache[key] = R.graph(lab, K, connectivity, frame)
    return _ref_cache[key]


def as_numpy(g):
    return dict(edge_index=g.edge_index.cpu().numpy(), boundary=g.boundary.cpu().numpy(),
                contrast=None if g.contrast is None else g.contrast.cpu().numpy(), offsets=g.offsets.cpu().numpy())


def assert_graph(g, ref, what=""):
    """Types, device, shapes and every value of a SuperpixelGraph against a reference dict."""
    assert g.edge_index.dtype == torch.int64 and g.boundary.dtype == torch.int32 and g.offsets.dtype == torch.int64, what
    assert g.edge_index.device == DEV and g.boundary.device == DEV and g.offsets.device == DEV, what
    got = as_numpy(g)
    E = ref["edge_index"].shape[1]
    assert got["edge_index"].shape == (2, E), "%s: %d edges, the reference has %d" % (what, got["edge_index"].shape[1], E)
    assert np.array_equal(got["offsets"], ref["offsets"]), what + ": offsets"
    assert np.array_equal(got["edge_index"], ref["edge_index"]), what + ": edge_index"
    assert np.array_equal(got["boundary"], ref["boundary"]), what + ": boundary"
    if ref["contrast"] is None:
        assert g.contrast is None, what
    else:
        assert g.contrast.dtype == torch.int64 and g.contrast.device == DEV, what
        assert got["contrast"].shape == ref["contrast"].shape and np.array_equal(got["contrast"], ref["contrast"]), what + ": contrast"


def assert_same(a, b):
    """Two SuperpixelGraphs, bitwise."""
    assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.boundary, b.boundary) and torch.equal(a.offsets, b.offsets)
    assert (a.contrast is None) == (b.contrast is None) and (a.contrast is None or torch.equal(a.contrast, b.contrast))


# ---- Slic map ----
@pytest.mark.parametrize("connectivity", [4, 8])
def test_slic_1280x720_k1600(connectivity):
    _, lab, frame = slic_case(720, 1280, 1600)
    ref = slic_ref(720, 1280, 1600, connectivity)
    g = superpixel_graph(lab, 1600, connectivity=connectivity, image=frame)
    assert_graph(g, ref, "numpy inputs")
    assert g.num_components == 1600 and g.capacity == first_capacity(1600) == 16384       # about 2.9 K edges: the first table holds them
    g = superpixel_graph(torch.from_numpy(lab).to(DEV), 1600, connectivity=connectivity)
    assert_graph(g, dict(ref, contrast=None), "device labels, no image")


# ---- seams ----
def seam_maps(H, W):
    """name -> (labels int64 [H, W], K)"""
    y, x = np.mgrid[0:H, 0:W]
    return {
        "vertical stripes": (x % 5, 5),
        "horizontal stripes": (y % 5, 5),
        "2x2 pattern": ((y % 2) * 2 + (x % 2), 4),                  # 0|3 and 1|2 touch on diagonals only
        "every pixel its own label": (y * W + x, H * W),          # more distinct pairs a tile than its lanes hold
    }


SEAM_SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2)] + [(h, w) for h in (15, 16, 17, 33) for w in (63, 64, 65, 129)]


@pytest.mark.parametrize("H,W", SEAM_SHAPES)
def test_seams(H, W):
    Cc = 1 + (H + W) % 4
    image = np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, Cc), dtype=np.uint8)
    image_dev = torch.from_numpy(image).to(DEV)
    for name, (lab, K) in seam_maps(H, W).items():
        for connectivity in (4, 8):
            ref = R.graph(lab, K, connectivity, image)
            for dtype in (np.int16, np.int32, np.int64):
                g = superpixel_graph(torch.from_numpy(lab.astype(dtype)).to(DEV), K, connectivity=connectivity, image=image_dev)
                assert_graph(g, ref, "%s, %dx%d, connectivity %d, %s, C=%d" % (name, H, W, connectivity, dtype.__name__, Cc))


# ---- labels outside the range ----
@pytest.mark.parametrize("connectivity", [4, 8])
def test_labels_outside_the_range(connectivity):
    _, lab, frame = slic_case(720, 1280, 1600)
    holes = np.random.default_rng(5).random(lab.shape)
    below, above, pick = holes < 0.02, holes > 0.98, (holes * 1e4).astype(np.int64) % 3      # where; which of three values
    lab16 = lab.copy()
    lab16[below] = np.array([-1, -2, -32768], np.int16)[pick[below]]
    lab16[above] = np.array([1600, 1605, 32767], np.int16)[pick[above]]
    ref = R.graph(lab16, 1600, connectivity, frame)
    assert_graph(superpixel_graph(lab16, 1600, connectivity=connectivity, image=frame), ref, "int16")
    lab32 = lab.astype(np.int32)
    lab32[below] = np.array([-1, -(1 << 31), -65536], np.int32)[pick[below]]
    lab32[above] = np.array([1600, (1 << 31) - 1, 1 << 16], np.int32)[pick[above]]          # 1 << 16: label 0 in its low 16 bits
    assert_graph(superpixel_graph(lab32, 1600, connectivity=connectivity, image=frame), ref, "int32")
    lab64 = lab.astype(np.int64)
    lab64[below] = np.array([-1, -(1 << 40), -(1 << 63)], np.int64)[pick[below]]
    lab64[above] = np.array([1600, (1 << 32) + 3, 1 << 16], np.int64)[pick[above]]          # (1 << 32) + 3: label 3 in its low 32 bits
    assert_graph(superpixel_graph(torch.from_numpy(lab64).to(DEV), 1600, connectivity=connectivity, image=frame), ref, "int64")


def test_labels_outside_the_range_differ_from_the_plain_map():
    """(the holes of the test above do change the graph: the test compares something)"""
    _, lab, frame = slic_case(720, 1280, 1600)
    lab16 = lab.copy()
    lab16[np.random.default_rng(5).random(lab.shape) < 0.02] = -1
    a, b = R.graph(lab16, 1600, 4, frame), slic_ref(720, 1280, 1600, 4)
    assert a["boundary"].sum() < b["boundary"].sum()


# ---- tiny K ----
def test_k1_gives_an_empty_graph():
    for lab, image in ((np.zeros((40, 70), np.int16), np.full((40, 70, 3), 9, np.uint8)), (np.zeros((2, 40, 70), np.int32), None)):
        g = superpixel_graph(lab, 1, connectivity=8, image=image)
        N = 1 if lab.ndim == 2 else 2
        assert g.edge_index.shape == (2, 0) and g.edge_index.dtype == torch.int64 and g.edge_index.device == DEV
        assert g.boundary.shape == (0,) and g.boundary.dtype == torch.int32
        assert g.offsets.tolist() == [0] * (N + 1) and g.offsets.dtype == torch.int64
        if image is None:
            assert g.contrast is None
        else:
            assert g.contrast.shape == (0, 3) and g.contrast.dtype == torch.int64
        off, idx = g.to_csr(N - 1)
        assert off.tolist() == [0, 0] and idx.shape == (0,) and idx.dtype == torch.int32


def test_k2_gives_one_edge():
    lab = np.zeros((40, 70), np.int64)
    lab[:, 33:] = 1
    g = superpixel_graph(lab, 2)
    assert g.edge_index.tolist() == [[0], [1]] and g.boundary.tolist() == [40] and g.offsets.tolist() == [0, 1]
    g = superpixel_graph(lab, 2, connectivity=8, image=np.full((40, 70, 1), 3, np.uint8) * lab[..., None].astype(np.uint8))
    assert g.edge_index.tolist() == [[0], [1]] and g.boundary.tolist() == [3 * 40 - 2] and g.contrast.tolist() == [[3 * (3 * 40 - 2)]]
    off, idx = g.to_csr()
    assert off.tolist() == [0, 1, 2] and idx.tolist() == [1, 0]


# ---- growth of the pair table ----
@pytest.mark.parametrize("connectivity", [4, 8])
def test_noise_map_grows_the_table(connectivity):
    K = 1024
    rng = np.random.default_rng(11)
    lab = rng.integers(0, K, (96, 96)).astype(np.int32)
    image = rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)
    ref = R.graph(lab, K, connectivity, image)
    assert first_capacity(K) == 8 * K
    assert ref["edge_index"].shape[1] > 8 * K                               # more pairs than the first table has slots
    g = superpixel_graph(lab, K, connectivity=connectivity, image=image)
    assert_graph(g, ref, "grown")
    assert g.capacity >= 4 * first_capacity(K) and g.capacity >= 2 * ref["edge_index"].shape[1]
    direct = superpixel_graph(lab, K, connectivity=connectivity, image=image, _start_capacity=g.capacity)
    assert direct.capacity == g.capacity
    assert_same(g, direct)
    larger = superpixel_graph(lab, K, connectivity=connectivity, image=image, _start_capacity=4 * g.capacity)
    assert larger.capacity == 4 * g.capacity
    assert_same(g, larger)


def test_small_start_capacity_grows_to_the_same_result():
    _, lab, frame = slic_case(240, 320, 150)
    ref = R.graph(lab, 150, 8, frame)
    g = superpixel_graph(lab, 150, connectivity=8, image=frame, _start_capacity=64)
    assert_graph(g, ref, "from 64 slots")
    assert 64 < g.capacity <= 2048


# ---- tables that end inside a chunk of the compact pass (1024 slots) ----
@pytest.mark.parametrize("H,W,K,connectivity,Cc,capacity", [
    (17, 65, 8, 8, 3, 64),         # 3 x 64 slots: one partial chunk that holds the three frames
    (33, 130, 20, 4, 4, 512),      # 3 x 512 slots: one chunk and a half, frame 1 straddles the chunks; C = 4: pixels read as words
])
def test_table_ends_inside_a_chunk(H, W, K, connectivity, Cc, capacity):
    rng = np.random.default_rng(H * 1000 + W)
    lab = rng.integers(0, K, (3, H, W)).astype(np.int16)
    image = rng.integers(0, 256, (3, H, W, Cc), dtype=np.uint8)
    ref = R.graph(lab, K, connectivity, image)
    pairs = K * (K - 1) // 2
    assert ref["offsets"].tolist() == [0, pairs, 2 * pairs, 3 * pairs] and 2 * pairs <= capacity      # every pair, in a table that holds them
    g = superpixel_graph(lab, K, connectivity=connectivity, image=image, _start_capacity=capacity)
    assert g.capacity == capacity
    assert_graph(g, ref, "%d slots a frame" % capacity)


# ---- batch ----
def test_batch_of_three_maps():
    cases = [slic_case(240, 320, 150, seed=s) for s in range(3)]
    labs = np.stack([c[1] for c in cases])
    frames = np.stack([c[2] for c in cases])
    ref = R.graph(labs, 150, 8, frames)
    g = superpixel_graph(torch.from_numpy(labs).to(DEV), 150, connectivity=8, image=torch.from_numpy(frames).to(DEV))
    assert_graph(g, ref, "batch")
    off = g.offsets.tolist()
    assert len(off) == 4 and off[0] == 0 and off[3] == g.edge_index.shape[1]
    assert len({tuple(labs[n].reshape(-1)[:4000]) for n in range(3)}) == 3         # three different maps
    for n in range(3):
        one = superpixel_graph(labs[n], 150, connectivity=8, image=frames[n])
        assert torch.equal(g.edge_index[:, off[n]:off[n + 1]], one.edge_index)
        assert torch.equal(g.boundary[off[n]:off[n + 1]], one.boundary)
        assert torch.equal(g.contrast[off[n]:off[n + 1]], one.contrast)
        assert one.offsets.tolist() == [0, off[n + 1] - off[n]]
        assert all(torch.equal(p, q) for p, q in zip(g.to_csr(n), one.to_csr()))


# ---- determinism ----
def test_two_calls_are_bitwise_equal():
    _, lab, frame = slic_case(720, 1280, 1600)
    lab_dev, frame_dev = torch.from_numpy(lab).to(DEV), torch.from_numpy(frame).to(DEV)
    a = superpixel_graph(lab_dev, 1600, connectivity=8, image=frame_dev)
    b = superpixel_graph(lab_dev, 1600, connectivity=8, image=frame_dev)
    assert_same(a, b)
    rng = np.random.default_rng(12)
    noise = torch.from_numpy(rng.integers(0, 300, (200, 333)).astype(np.int16)).to(DEV)
    nimg = torch.from_numpy(rng.integers(0, 256, (200, 333, 4), dtype=np.uint8)).to(DEV)
    assert_same(superpixel_graph(noise, 300, connectivity=8, image=nimg), superpixel_graph(noise, 300, connectivity=8, image=nimg))


# ---- streams ----
def test_on_a_non_default_stream():
    _, lab, frame = slic_case(720, 1280, 1600)
    ref = slic_ref(720, 1280, 1600, 8)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(DEV)
    with torch.cuda.stream(st):
        lab_s = torch.from_numpy(lab).to(DEV).clone()                               # produced on st
        frame_s = torch.from_numpy(frame).to(DEV).clone()
        g = superpixel_graph(lab_s, 1600, connectivity=8, image=frame_s)
        off, idx = g.to_csr()
    st.synchronize()
    assert_graph(g, ref, "stream")
    assert int(off[-1]) == 2 * ref["edge_index"].shape[1] == idx.shape[0]


# ---- against what exists ----
def test_get_connectivity_is_a_subset_of_the_8_connectivity_graph():
    slic, lab, _ = slic_case(720, 1280, 1600)
    g = superpixel_graph(lab, 1600, connectivity=8)
    edges = set(map(tuple, g.edge_index.t().tolist()))
    listed = slic.slic_model.get_connectivity(lab).tolist()
    pairs = {(min(k, v), max(k, v)) for k, row in enumerate(listed) for v in row}
    assert len(pairs) > 1600 and pairs <= edges
    # and the 4-connectivity graph is a subgraph of it with no longer boundaries
    g4 = superpixel_graph(lab, 1600, connectivity=4)
    e4 = {e: b for e, b in zip(map(tuple, g4.edge_index.t().tolist()), g4.boundary.tolist())}
    e8 = {e: b for e, b in zip(map(tuple, g.edge_index.t().tolist()), g.boundary.tolist())}
    assert set(e4) <= set(e8) and all(e8[e] >= b for e, b in e4.items())


# ---- CSR ----
def test_csr_rows_round_trip_through_the_crf_frame():
    from fast_slic_amd.crf import SimpleCRF
    K = 200
    slic, lab, frame = slic_case(240, 320, K, seed=1)
    g = superpixel_graph(lab, K, connectivity=8, image=frame)
    off, idx = g.to_csr()
    assert off.dtype == torch.int64 and idx.dtype == torch.int32 and off.shape == (K + 1,) and off.device == DEV and idx.device == DEV
    off, idx = off.tolist(), idx.tolist()
    rows = [idx[off[k]:off[k + 1]] for k in range(K)]
    assert off[0] == 0 and off[K] == 2 * g.edge_index.shape[1]
    assert all(row == sorted(set(row)) for row in rows)                            # ascending, no duplicates
    assert all(k in rows[v] for k, row in enumerate(rows) for v in row)            # symmetric
    assert {(k, v) for k, row in enumerate(rows) for v in row if k < v} == set(map(tuple, g.edge_index.t().tolist()))
    crf = SimpleCRF(3, K)
    f = crf.push_slic_frame(slic)
    f.set_connectivity(rows)
    assert f.get_connectivity() == rows
