"""Merging on the region adjacency graph on the MI355X (fast_slic_amd/merge.py, csrc/merge.hip) against the model written from the
rules (tests/merge_ref.py), with exact equality throughout.  merge_labels takes four pixels a thread (shapes around 4 and around a
block of 1024 pixels, every label width, unaligned maps and outputs); merge_components takes chunks of 256 nodes and at most 8192
blocks, its edge kernels at most 2048 blocks of 256 edges (graphs below and above both); contract_graph is held to its identity
against superpixel_graph of the relabelled map."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import connect_ref
import merge_ref as M
import rag_ref
from fast_slic_amd import _binding as B
from fast_slic_amd.merge import best_neighbour_edges, compose_mappings, contract_graph, merge_components, merge_labels
from fast_slic_amd.pool import superpixel_pool
from fast_slic_amd.rag import SuperpixelGraph, superpixel_graph
from test_gpu_connect import SHAPES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [np.int16, np.int32, np.int64]


# ---- graphs: the model's dict <-> a SuperpixelGraph on the GPU ----
def to_graph(d, K):
    return SuperpixelGraph(torch.from_numpy(np.ascontiguousarray(d["edge_index"], np.int64)).to(DEV),
                           torch.from_numpy(np.asarray(d["boundary"]).astype(np.int32)).to(DEV),
                           None if d["contrast"] is None else torch.from_numpy(np.ascontiguousarray(d["contrast"], np.int64)).to(DEV),
                           torch.from_numpy(np.asarray(d["offsets"], np.int64)).to(DEV), K, 1024)


def to_dict(g):
    return dict(edge_index=g.edge_index.cpu().numpy(), boundary=g.boundary.cpu().numpy().astype(np.int64),
                contrast=None if g.contrast is None else g.contrast.cpu().numpy(), offsets=g.offsets.cpu().numpy())


def graph_of(frames):
    """frames: per frame a sorted list of (a, b) -> the model's dict, every boundary 1."""
    edges = [e for fr in frames for e in fr]
    return dict(edge_index=np.array(edges, np.int64).reshape(-1, 2).T.copy(), boundary=np.ones(len(edges), np.int64), contrast=None,
                offsets=np.cumsum([0] + [len(fr) for fr in frames]).astype(np.int64))


def path(K):
    return [(i, i + 1) for i in range(K - 1)]


def star(K):
    return [(0, i) for i in range(1, K)]


def check_components(d, K, join, members=None):
    """merge_components of the graph `d` against the model; returns (mapping, n) as numpy."""
    want, want_n = M.components(d, join, K, members)
    mem = None if members is None else torch.from_numpy(np.asarray(members)).to(DEV)
    mapping, n = merge_components(to_graph(d, K), torch.from_numpy(np.asarray(join, bool)).to(DEV), mem)
    N = len(d["offsets"]) - 1
    assert mapping.dtype == torch.int32 and n.dtype == torch.int32 and mapping.device == DEV and n.device == DEV
    assert tuple(mapping.shape) == (N, K) and tuple(n.shape) == (N,)
    mapping, n = mapping.cpu().numpy(), n.cpu().numpy()
    assert np.array_equal(n, want_n) and np.array_equal(mapping, want)
    for f in range(N):                                                     # dense: the labels 0 .. n - 1 all occur
        assert np.array_equal(np.unique(mapping[f][mapping[f] >= 0]), np.arange(n[f]))
    return mapping, n


@functools.lru_cache(maxsize=None)
def map_case(kind, H, W, K=40, N=2):
    """(maps int32 [N, H, W] with labels of -1 and >= K, image uint8 [N, H, W, 3]), computed once."""
    rng = np.random.default_rng(H * 1000 + W)
    maps = np.stack([(connect_ref.blocky if kind == "blocky" else connect_ref.noise)(H, W, K + 2, seed=H * 1000 + W + i) for i in range(N)])
    maps[0][rng.random((H, W)) < 0.05] = -1
    return maps, rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)


# ---- merge_labels ----
def labels_case(shape, K, seed):
    rng = np.random.default_rng(seed)
    N = shape[0] if len(shape) == 3 else 1
    lab = rng.integers(-2, K + 3, shape).astype(np.int64)                  # -2, -1, K, K + 1, K + 2 are no labels
    mapping = rng.integers(0, max(K // 2, 1), (N, K)).astype(np.int32)
    mapping[rng.random((N, K)) < 0.2] = -1
    return lab, mapping


@pytest.mark.parametrize("pixels", [1, 3, 4, 5, 1023, 1024, 1025])
@pytest.mark.parametrize("N", [1, 3])
def test_labels_around_the_vector_width_and_a_block(pixels, N):
    for K in (1, 7, 65534):
        lab, mapping = labels_case((N, 1, pixels), K, pixels * 10 + N)
        if K == 65534:
            lab[..., :1] = 65533                                           # the last node, and 65534 next to it
            lab[..., -1:] = 65534
        mp = torch.from_numpy(mapping).to(DEV)
        for dtype in DTYPES:
            m = np.where((lab < -32768) | (lab > 32767), -1, lab).astype(dtype) if dtype == np.int16 else lab.astype(dtype)
            if dtype == np.int16 and K == 65534:
                m = lab.astype(np.uint16).view(np.int16)                   # labels above 32767 as Slic's int16 map holds them
            want = M.labels(m, mapping)
            out = merge_labels(torch.from_numpy(m).to(DEV), mp)
            assert out.dtype == torch.int32 and out.device == DEV and tuple(out.shape) == (N, 1, pixels)
            assert np.array_equal(out.cpu().numpy(), want), (pixels, N, K, dtype)
            if N == 1:                                                     # an [H, W] map with its [1, K] mapping
                assert np.array_equal(merge_labels(torch.from_numpy(m[0]).to(DEV), mp).cpu().numpy(), want[0])


@pytest.mark.parametrize("H,W", SHAPES)
def test_labels_shapes(H, W):
    lab, mapping = labels_case((3, H, W), 40, H * 1000 + W)
    mp = torch.from_numpy(mapping).to(DEV)
    for dtype in DTYPES:
        m = lab.astype(dtype)
        want = M.labels(m, mapping)
        assert np.array_equal(merge_labels(torch.from_numpy(m).to(DEV), mp).cpu().numpy(), want), (H, W, dtype)
    assert np.array_equal(merge_labels(lab.astype(np.int16), mp).cpu().numpy(), want)          # a numpy map is uploaded
    assert np.array_equal(merge_labels(lab[1].astype(np.uint16), mp[1:2], device=DEV).cpu().numpy(), M.labels(lab[1].astype(np.uint16), mapping[1]))


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32, torch.int64])
def test_labels_of_an_unaligned_view(dtype):
    H, W, K = 33, 31, 40
    lab, mapping = labels_case((H, W), K, 5)
    mp = torch.from_numpy(mapping).to(DEV)
    want = M.labels(lab, mapping)
    for shift in (1, 2, 3, 5):
        buf = torch.zeros(H * W + 8, dtype=dtype, device=DEV)
        view = buf[shift:shift + H * W].view(H, W)
        view.copy_(torch.from_numpy(lab).to(DEV))
        assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + shift * buf.element_size()
        assert view.data_ptr() % 16 != 0 or dtype == torch.int64 and shift == 2
        assert np.array_equal(merge_labels(view, mp).cpu().numpy(), want), (dtype, shift)


def test_labels_into_an_unaligned_output():
    """The C entry with `out` 4, 8 and 12 bytes past a 16-byte boundary: the single pixels before the first aligned four."""
    lib = B.load_library()
    K = 40
    for pixels in (1, 2, 3, 4, 7, 1030):
        lab, mapping = labels_case((1, pixels), K, pixels)
        want = M.labels(lab, mapping)
        mp = torch.from_numpy(mapping).to(DEV)
        for ltype, dtype in ((0, np.int16), (1, np.int32), (2, np.int64)):
            t = torch.from_numpy(lab.astype(dtype)).to(DEV)
            for shift in (0, 1, 2, 3):
                buf = torch.full((pixels + 8,), 77, dtype=torch.int32, device=DEV)
                out = buf[shift:shift + pixels]
                B._check(lib.fslic_hip_merge_labels(0, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream), 1, 1, pixels, K, t.data_ptr(),
                                                    ltype, mp.data_ptr(), out.data_ptr()))
                got = buf.cpu().numpy()
                assert np.array_equal(got[shift:shift + pixels], want[0]), (pixels, dtype, shift)
                assert (got[:shift] == 77).all() and (got[shift + pixels:] == 77).all()              # nothing outside `out`


# ---- merge_components ----
def test_components_of_no_join_and_of_every_join():
    maps, _ = map_case("blocky", 33, 130)
    d = rag_ref.graph(maps, 40)
    E = d["boundary"].shape[0]
    mapping, n = check_components(d, 40, np.zeros(E, bool))
    assert np.array_equal(mapping, np.tile(np.arange(40, dtype=np.int32), (2, 1))) and n.tolist() == [40, 40]
    check_components(d, 40, np.ones(E, bool))


def test_components_of_the_longest_path():
    K = 65534
    d = graph_of([path(K)])
    mapping, n = check_components(d, K, np.ones(K - 1, bool))
    assert not mapping.any() and n.tolist() == [1]
    join = np.ones(K - 1, bool)
    join[40000] = False                                                    # the edge (40000, 40001)
    mapping, n = check_components(d, K, join)
    assert n.tolist() == [2] and not mapping[0, :40001].any() and mapping[0, 40001:].all()
    rev = graph_of([path(K), path(K)])                                     # two frames, the second with members of its own
    members = np.ones((2, K), np.int64)
    members[1, 1000::1000] = 0
    mapping, n = check_components(rev, K, np.ones(2 * (K - 1), bool), members)
    assert n.tolist() == [1, 66]


def test_components_of_a_star():
    K = 300
    d = graph_of([star(K), star(K)])
    join = np.ones(2 * (K - 1), bool)
    join[K - 1 + 5:] = np.random.default_rng(3).random(K - 1 - 5) < 0.5
    mapping, n = check_components(d, K, join)
    assert n[0] == 1


@pytest.mark.parametrize("kind", ["blocky", "noise"])
def test_components_of_random_joins(kind):
    maps, _ = map_case(kind, 64, 257)
    rng = np.random.default_rng(7)
    for connectivity in (4, 8):
        d = rag_ref.graph(maps, 40, connectivity)
        E = d["boundary"].shape[0]
        for p in (0.02, 0.1, 0.5):
            check_components(d, 40, rng.random(E) < p)


def test_components_with_absent_nodes():
    maps, _ = map_case("blocky", 33, 130)
    K = 48                                                                 # the labels 42 .. 47 never occur
    d = rag_ref.graph(maps, K)
    E = d["boundary"].shape[0]
    members = np.stack([np.bincount(m[(m >= 0) & (m < K)], minlength=K) for m in maps])
    assert (members[:, 42:] == 0).all()
    members[0, [3, 10, 11]] = 0                                            # nodes with edges turned absent: their edges are ignored
    rng = np.random.default_rng(9)
    for dtype in (np.int32, np.int64):
        mapping, n = check_components(d, K, rng.random(E) < 0.3, members.astype(dtype))
        assert (mapping[members == 0] == -1).all() and (mapping[members > 0] >= 0).all()
    mapping, n = check_components(d, K, np.ones(E, bool), members)
    single = rag_ref.graph(maps[1], K)                                     # N = 1 with [K] members
    want, want_n = M.components(single, np.ones(single["boundary"].shape[0], bool), K, members[1])
    got, got_n = merge_components(to_graph(single, K), torch.ones(single["boundary"].shape[0], dtype=torch.bool, device=DEV),
                                  torch.from_numpy(members[1]).to(DEV))
    assert tuple(got.shape) == (1, K) and np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_n.cpu().numpy(), want_n)


def test_components_of_frames_without_edges():
    K = 9
    d = graph_of([path(K), [], star(K), []])
    assert d["offsets"].tolist() == [0, 8, 8, 16, 16]
    join = np.ones(16, bool)
    join[3] = join[12] = False
    mapping, n = check_components(d, K, join)
    assert n.tolist() == [2, 9, 2, 9] and mapping[1].tolist() == list(range(9))
    empty = graph_of([[], []])                                             # E = 0
    members = np.array([[1, 0, 2, 0, 1], [0, 0, 0, 0, 0]], np.int32)
    mapping, n = check_components(empty, 5, np.zeros(0, bool), members)
    assert mapping.tolist() == [[0, -1, 1, -1, 2], [-1] * 5] and n.tolist() == [3, 0]
    assert check_components(empty, 5, np.zeros(0, bool))[1].tolist() == [5, 5]
    g = to_graph(empty, 5)
    join = best_neighbour_edges(g, torch.zeros(0, device=DEV), 1.0)
    assert join.dtype == torch.bool and tuple(join.shape) == (0,) and join.device == DEV
    c = contract_graph(g, torch.zeros((2, 5), dtype=torch.int32, device=DEV), 3)
    assert tuple(c.edge_index.shape) == (2, 0) and c.offsets.tolist() == [0, 0, 0] and c.contrast is None and c.num_components == 3


def test_components_of_more_items_than_a_launch_has_threads():
    """A near complete graph of K = 400 in 8 frames has more edges than the 2048 x 256 threads of an edge launch; 8200 frames have
    more chunks, and more scans, than a node launch has blocks."""
    maps = np.stack([connect_ref.noise(256, 256, 400, seed=i) for i in range(8)])
    g = superpixel_graph(torch.from_numpy(maps).to(DEV), 400, connectivity=8)
    d = to_dict(g)
    E = d["boundary"].shape[0]
    assert E > 2048 * 256
    rng = np.random.default_rng(1)
    join = rng.random(E) < 0.003
    mapping, n = check_components(d, 400, join)
    assert 1 < n.min() and n.max() < 400
    w = rng.integers(0, 1000, E).astype(np.float32)
    got = best_neighbour_edges(g, torch.from_numpy(w).to(DEV), 500.0)
    assert np.array_equal(got.cpu().numpy(), M.best_edges(d, w, 500.0))
    N, K = 8200, 5
    many = graph_of([path(K)] * N)
    mapping, n = check_components(many, K, np.random.default_rng(2).random(N * (K - 1)) < 0.5)
    assert len(set(n.tolist())) == 5


# ---- best_neighbour_edges ----
def check_best(d, K, w, threshold=None):
    w = np.asarray(w, np.float32)
    want = M.best_edges(d, w, threshold)
    got = best_neighbour_edges(to_graph(d, K), torch.from_numpy(w).to(DEV), threshold)
    assert got.dtype == torch.bool and got.device == DEV and tuple(got.shape) == w.shape
    assert np.array_equal(got.cpu().numpy(), want)
    return want


def test_best_edges_of_equal_weights():
    maps, _ = map_case("blocky", 33, 130)
    d = rag_ref.graph(maps, 40, 8)
    E = d["boundary"].shape[0]
    join = check_best(d, 40, np.full(E, 2.5, np.float32))                  # the lowest position wins at every node
    a, b = d["edge_index"]
    for f, (lo, hi) in enumerate(M.frames_of(d)):
        first = {}
        for e in range(lo, hi):
            first.setdefault(int(a[e]), e)
            first.setdefault(int(b[e]), e)
        assert np.array_equal(np.flatnonzero(join[lo:hi]) + lo, sorted(set(first.values())))
    assert np.array_equal(check_best(d, 40, np.full(E, 2.5, np.float32), None), join)
    assert not check_best(d, 40, np.full(E, 2.5, np.float32), 2.5).any()              # a threshold equal to the weight excludes it
    assert np.array_equal(check_best(d, 40, np.full(E, 2.5, np.float32), 2.5000001), join)


def test_best_edges_thresholds_and_zeros():
    maps, _ = map_case("noise", 33, 130, 12)
    d = rag_ref.graph(maps, 12, 4)
    E = d["boundary"].shape[0]
    rng = np.random.default_rng(4)
    w = rng.integers(0, 5, E).astype(np.float32)
    for threshold in (None, 0.0, 1.0, 3.0, 4.0, 4.5, float("inf")):
        check_best(d, 12, w, threshold)
    w = (rng.random(E) * 10).astype(np.float32)
    for threshold in (None, float(w[5]), 2.0, 1e-3):
        check_best(d, 12, w, threshold)
    signed = np.where(rng.random(E) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    assert np.signbit(signed).any() and not np.signbit(signed).all()
    join = check_best(d, 12, signed)                                       # -0.0 against +0.0: equal, the position decides
    assert np.array_equal(join, check_best(d, 12, np.zeros(E, np.float32)))
    check_best(d, 12, signed, 1e-30)
    tiny = (rng.integers(0, 3, E) * np.float32(1e-45)).astype(np.float32)  # subnormals order like any other value
    check_best(d, 12, tiny)


def test_best_edges_of_a_node_without_an_eligible_edge():
    d = graph_of([[(0, 1), (0, 2), (1, 2), (2, 3)]])
    join = check_best(d, 4, [1.0, 5.0, 5.0, 7.0], 6.0)                     # node 3's only edge is not eligible
    assert join.tolist() == [True, True, False, False]
    assert check_best(d, 4, [9.0, 9.0, 9.0, 1.0], 6.0).tolist() == [False, False, False, True]
    assert check_best(d, 5, [9.0, 9.0, 9.0, 9.0], 6.0).tolist() == [False] * 4        # and node 4 has no edge at all


def test_best_edges_take_positions_per_frame():
    maps, _ = map_case("blocky", 33, 130)
    one = rag_ref.graph(maps[1], 40, 8)
    E = one["boundary"].shape[0]
    two = dict(edge_index=np.concatenate([one["edge_index"]] * 2, axis=1), boundary=np.concatenate([one["boundary"]] * 2), contrast=None,
               offsets=np.array([0, E, 2 * E], np.int64))
    w = np.random.default_rng(6).integers(0, 3, E).astype(np.float32)
    join = check_best(two, 40, np.concatenate([w, w]))
    assert np.array_equal(join[:E], join[E:]) and np.array_equal(join[:E], check_best(one, 40, w))


# ---- contract_graph ----
def same(g, h):
    return (torch.equal(g.edge_index, h.edge_index) and torch.equal(g.boundary, h.boundary) and torch.equal(g.offsets, h.offsets)
            and (g.contrast is None) == (h.contrast is None) and (g.contrast is None or torch.equal(g.contrast, h.contrast))
            and g.num_components == h.num_components)


@pytest.mark.parametrize("H,W", SHAPES)
def test_contraction_identity(H, W):
    K = 40
    rng = np.random.default_rng(H * 1000 + W)
    for kind in ("blocky", "noise"):
        maps, image = map_case(kind, H, W)
        lab, img = torch.from_numpy(maps).to(DEV), torch.from_numpy(image).to(DEV)
        for connectivity in (4, 8):
            for im in (None, img):
                g = superpixel_graph(lab, K, connectivity, im)
                for groups, K2 in ((K, K), (11, 11), (7, 4), (1, 1)):       # (7, 4): a bound below n drops the groups 4 .. 6
                    mapping = rng.integers(0, groups, (2, K)).astype(np.int32)
                    mapping[rng.random((2, K)) < 0.1] = -1
                    mp = torch.from_numpy(mapping).to(DEV)
                    got = contract_graph(g, mp, K2)
                    want = superpixel_graph(merge_labels(lab, mp), K2, connectivity, im)
                    assert same(got, want), (kind, H, W, connectivity, im is not None, groups, K2)
                    assert got.boundary.dtype == torch.int32 and got.edge_index.dtype == torch.int64 and got.offsets.dtype == torch.int64
                    assert M.same_graph(to_dict(got), M.contract(to_dict(g), mapping, K2))
        one = superpixel_graph(lab[0], K, 8, img[0])                        # an [H, W] map: N = 1
        assert same(contract_graph(one, mp[:1], 4), superpixel_graph(merge_labels(lab[0], mp[:1]), 4, 8, img[0]))


def test_contraction_grows_its_table():
    K = 300
    maps = np.stack([connect_ref.noise(96, 96, K, seed=i) for i in range(2)])
    lab = torch.from_numpy(maps).to(DEV)
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (2, 96, 96, 2)).astype(np.uint8)).to(DEV)
    g = superpixel_graph(lab, K, 8, img)
    mapping = torch.from_numpy((np.arange(2 * K).reshape(2, K) % 150).astype(np.int32)).to(DEV)
    want = superpixel_graph(merge_labels(lab, mapping), 150, 8, img)
    assert want.edge_index.shape[1] > 2 * 2048                            # more pairs than half of the tables below
    for cap in (64, 1024, None):
        got = contract_graph(g, mapping, 150, _start_capacity=cap)
        assert same(got, want) and got.capacity >= 8192 and (cap is None or got.capacity > cap)


def test_contraction_adds_64_bit_contrast():
    """Rows near 2^40 do not fit the 32-bit addends of the pixel pass: two of them merging into one."""
    base = 1 << 40
    d = graph_of([[(0, 1), (0, 2), (1, 2), (2, 3)], [(0, 3)]])
    d["boundary"] = np.array([5, 7, 11, 13, 2 ** 31 - 1], np.int64)
    d["contrast"] = np.array([[base + 1, 3], [base + 5, base - 1], [7 * base, 2 ** 62], [0, 9], [2 ** 62 + 5, 1]], np.int64)
    mapping = np.array([[0, 0, 1, 2], [1, -1, -1, 0]], np.int32)
    got = contract_graph(to_graph(d, 4), torch.from_numpy(mapping).to(DEV), 3)
    assert got.offsets.tolist() == [0, 2, 3] and got.edge_index.tolist() == [[0, 1, 0], [1, 2, 1]]
    assert got.boundary.tolist() == [18, 13, 2 ** 31 - 1]
    assert got.contrast.tolist() == [[8 * base + 5, 2 ** 62 + base - 1], [0, 9], [2 ** 62 + 5, 1]]
    assert M.same_graph(to_dict(got), M.contract(d, mapping, 3))


def test_contraction_by_the_identity_and_into_one():
    maps, image = map_case("blocky", 64, 257)
    lab, img = torch.from_numpy(maps).to(DEV), torch.from_numpy(image).to(DEV)
    g = superpixel_graph(lab, 40, 8, img)
    ident = torch.arange(40, dtype=torch.int32, device=DEV).repeat(2, 1)
    assert same(contract_graph(g, ident, 40), g)
    wider = contract_graph(g, ident, 50)
    assert wider.num_components == 50 and torch.equal(wider.edge_index, g.edge_index) and torch.equal(wider.contrast, g.contrast)
    one = contract_graph(g, torch.zeros((2, 40), dtype=torch.int32, device=DEV), 40)
    assert tuple(one.edge_index.shape) == (2, 0) and one.offsets.tolist() == [0, 0, 0] and tuple(one.contrast.shape) == (0, 3)
    assert tuple(one.boundary.shape) == (0,)


# ---- the loop of the README ----
def test_three_rounds_of_the_loop():
    N, H, W, K, threshold, rounds = 2, 64, 130, 60, 3.0, 3
    rng = np.random.default_rng(12)
    maps = np.stack([connect_ref.blocky(H, W, K, seed=50 + i) for i in range(N)]).astype(np.int16)
    image = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    feat = (maps.astype(np.int64) * 7 % 11 + (rng.random((N, H, W)) < 0.1)).astype(np.float32)[:, None]      # [N, 1, H, W], small integers
    labels, img, features = torch.from_numpy(maps).to(DEV), torch.from_numpy(image).to(DEV), torch.from_numpy(feat).to(DEV)

    # the device
    g = superpixel_graph(labels, K, image=img)
    sums, counts = superpixel_pool(features, labels, K, reduce="sum", return_counts=True)
    total, ns = None, []
    for _ in range(rounds):
        a, b = g.edge_index
        frame = torch.searchsorted(g.offsets[1:].contiguous(), torch.arange(a.numel(), device=a.device), right=True)
        mean = sums / counts.clamp_min(1).unsqueeze(1)                      # [N, C, K]
        w = (mean[frame, :, a] - mean[frame, :, b]).norm(dim=1)
        mapping, n = merge_components(g, best_neighbour_edges(g, w, threshold), members=counts)
        total = mapping if total is None else compose_mappings(total, mapping)
        g = contract_graph(g, mapping, K)
        idx = mapping.clamp_min(0).long()                                  # (an absent node has no members and no sum: it adds nothing)
        sums = torch.zeros_like(sums).scatter_add_(2, idx.unsqueeze(1), sums)
        counts = torch.zeros_like(counts).scatter_add_(1, idx, counts)
        ns.append(n.cpu().numpy())
    coarse = merge_labels(labels, total)

    # the model
    d = rag_ref.graph(maps, K, 4, image)
    msums = np.stack([np.bincount(maps[f].reshape(-1), weights=feat[f, 0].reshape(-1), minlength=K) for f in range(N)]).astype(np.float32)
    mcounts = np.stack([np.bincount(maps[f].reshape(-1), minlength=K) for f in range(N)]).astype(np.int32)
    mtotal = None
    for r in range(rounds):
        a, b = d["edge_index"]
        frame = np.searchsorted(d["offsets"][1:], np.arange(a.shape[0]), side="right")
        mean = msums / np.maximum(mcounts, 1).astype(np.float32)
        w = np.abs(mean[frame, a] - mean[frame, b]).astype(np.float32)
        mapping, n = M.components(d, M.best_edges(d, w, threshold), K, mcounts)
        assert np.array_equal(n, ns[r]), r
        mtotal = mapping if mtotal is None else M.compose(mtotal, mapping)
        d = M.contract(d, mapping, K)
        nsums, ncounts = np.zeros_like(msums), np.zeros_like(mcounts)
        for f in range(N):
            np.add.at(nsums[f], np.maximum(mapping[f], 0), msums[f])
            np.add.at(ncounts[f], np.maximum(mapping[f], 0), mcounts[f])
        msums, mcounts = nsums, ncounts
    assert ns[0].max() < K and (ns[2] < ns[0]).all() and ns[2].min() > 1     # the rounds did merge, and did not merge everything
    assert np.array_equal(total.cpu().numpy(), mtotal)
    assert np.array_equal(coarse.cpu().numpy(), M.labels(maps, mtotal))
    assert M.same_graph(to_dict(g), d)
    assert same(g, superpixel_graph(coarse, K, image=img))
    assert np.array_equal(counts.cpu().numpy(), mcounts) and np.array_equal(sums[:, 0].cpu().numpy(), msums)


# ---- determinism and synchronisation ----
def round_of_calls(g, w, counts, labels):
    join = best_neighbour_edges(g, w, 2.0)
    mapping, n = merge_components(g, join, counts)
    return join, mapping, n, merge_labels(labels, mapping), compose_mappings(mapping, mapping)


def round_inputs():
    maps, image = map_case("noise", 64, 257, 12)
    labels = torch.from_numpy(maps).to(DEV)
    g = superpixel_graph(labels, 12, 8, torch.from_numpy(image).to(DEV))
    w = torch.from_numpy(np.random.default_rng(8).integers(0, 4, g.boundary.shape[0]).astype(np.float32)).to(DEV)
    counts = torch.from_numpy(np.stack([np.bincount(m[(m >= 0) & (m < 12)], minlength=12) for m in maps])).to(DEV)
    return maps, g, w, counts, labels


def test_determinism_and_inputs_untouched():
    maps, g, w, counts, labels = round_inputs()
    keep = [t.clone() for t in (g.edge_index, g.boundary, g.contrast, g.offsets, w, counts, labels)]
    first = round_of_calls(g, w, counts, labels)
    graph = contract_graph(g, first[1], 12)
    for _ in range(3):
        again = round_of_calls(g, w, counts, labels)
        assert all(torch.equal(x, y) for x, y in zip(first, again))
        assert same(contract_graph(g, first[1], 12), graph)
    assert all(torch.equal(x, y) for x, y in zip(keep, (g.edge_index, g.boundary, g.contrast, g.offsets, w, counts, labels)))
    d = to_dict(g)
    want, want_n = M.components(d, M.best_edges(d, w.cpu().numpy(), 2.0), 12, counts.cpu().numpy())
    assert np.array_equal(first[1].cpu().numpy(), want) and np.array_equal(first[2].cpu().numpy(), want_n)


def test_side_stream():
    maps, g, w, counts, labels = round_inputs()
    want = round_of_calls(g, w, counts, labels)
    want_graph = contract_graph(g, want[1], 12)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        w2 = w.clone()
        got = round_of_calls(g, w2, counts, labels)
        graph = contract_graph(g, got[1], 12)                              # consumes the mapping on the same stream
        s.synchronize()                                                    # this stream only
        assert all(torch.equal(x, y) for x, y in zip(want, got)) and same(graph, want_graph)


def test_no_host_synchronisation():
    maps, g, w, counts, labels = round_inputs()
    want = round_of_calls(g, w, counts, labels)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            got = round_of_calls(g, w, counts, labels)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error')")
    assert all(torch.equal(x, y) for x, y in zip(want, got))
