"""CPU tests of merging on the region adjacency graph (fast_slic_amd/merge.py, the fslic_hip_merge* entries): the model
(tests/merge_ref.py) by hand on tiny graphs, the contraction identity as the model against tests/rag_ref.py, and every argument error
refused before any device work -- ValueError in Python, FSLIC_E_INVALID from the C ABI before its first HIP call.  No kernel is
launched here."""
import ctypes as C

import numpy as np
import pytest
import torch

import connect_ref
import merge_ref as M
import rag_ref
from fast_slic_amd import _binding as B
from fast_slic_amd.merge import (best_neighbour_edges, compose_mappings, contract_capacity_limit, contract_graph, merge_components,
                                 merge_labels)
from fast_slic_amd.rag import SuperpixelGraph


def graph_of(frames, contrast=None):
    """frames: per frame a list of (a, b, boundary), sorted -> the graph dict of rag_ref."""
    edges = [e for fr in frames for e in fr]
    offsets = np.cumsum([0] + [len(fr) for fr in frames])
    return dict(edge_index=np.array([[e[0] for e in edges], [e[1] for e in edges]], np.int64).reshape(2, -1),
                boundary=np.array([e[2] for e in edges], np.int64), contrast=contrast, offsets=offsets.astype(np.int64))


TRIANGLE = [(0, 1, 2), (0, 2, 3), (1, 2, 4)]
PATH = [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1)]


# ---- the model, by hand ----
def test_triangle_with_equal_weights():
    g = graph_of([TRIANGLE])
    # every node's best edge is its edge of the lowest position: 0 -> (0,1), 1 -> (0,1), 2 -> (0,2)
    assert M.best_edges(g, [1.0, 1.0, 1.0]).tolist() == [True, True, False]
    assert M.best_edges(g, [1.0, 1.0, 0.5]).tolist() == [True, False, True]          # 0 -> (0,1); 1 and 2 -> (1,2)
    assert M.best_edges(g, [1.0, 1.0, 0.5], threshold=1.0).tolist() == [False, False, True]      # strictly below; node 0 has none
    assert M.best_edges(g, [1.0, 1.0, 0.5], threshold=0.5).tolist() == [False, False, False]
    assert M.best_edges(g, [0.0, -0.0, 0.0]).tolist() == [True, True, False]         # -0.0 is +0.0: the position decides
    mapping, n = M.components(g, [True, True, False], 3)
    assert mapping.tolist() == [[0, 0, 0]] and n.tolist() == [1]
    mapping, n = M.components(g, [False, False, True], 4)                            # node 3 has no edge
    assert mapping.tolist() == [[0, 1, 1, 2]] and n.tolist() == [3]


def test_path():
    g = graph_of([PATH])
    w = [3.0, 1.0, 2.0, 5.0]
    # 0 -> (0,1); 1 -> (1,2); 2 -> (1,2); 3 -> (2,3); 4 -> (3,4)
    assert M.best_edges(g, w).tolist() == [True, True, True, True]
    assert M.best_edges(g, w, threshold=3.0).tolist() == [False, True, True, False]
    mapping, n = M.components(g, [True, False, True, True], 5)
    assert mapping.tolist() == [[0, 0, 1, 1, 1]] and n.tolist() == [2]
    mapping, n = M.components(g, [True, True, True, True], 5, members=[[4, 0, 1, 1, 9]])       # node 1 is absent: its edges are ignored
    assert mapping.tolist() == [[0, -1, 1, 1, 1]] and n.tolist() == [2]
    c = M.contract(g, [[0, 0, 1, 1, 1]], 2)
    assert c["edge_index"].tolist() == [[0], [1]] and c["boundary"].tolist() == [1] and c["offsets"].tolist() == [0, 1]
    c = M.contract(g, [[1, 0, 1, 0, -1]], 2)                                         # (0,1), (1,2), (2,3) all become (0, 1); (3,4) is dropped
    assert c["edge_index"].tolist() == [[0], [1]] and c["boundary"].tolist() == [3]
    assert M.contract(g, [[1, 0, 1, 0, -1]], 1)["offsets"].tolist() == [0, 0]        # K2 = 1: group 1 is outside


def test_two_frames():
    g = graph_of([TRIANGLE, PATH], contrast=np.arange(14, dtype=np.int64).reshape(7, 2) + (1 << 40))
    w = [1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 2.0]
    # positions are taken per frame: the path's edges are 0 .. 3, so every node takes its lower edge
    join = M.best_edges(g, w)
    assert join.tolist() == [True, True, False, True, True, True, True]
    mapping, n = M.components(g, [True, False, False, False, True, False, True], 5, members=None)
    assert mapping.tolist() == [[0, 0, 1, 2, 3], [0, 1, 1, 2, 2]] and n.tolist() == [4, 3]
    c = M.contract(g, mapping, 5)
    assert c["offsets"].tolist() == [0, 1, 3] and c["edge_index"].tolist() == [[0, 0, 1], [1, 1, 2]]
    assert c["boundary"].tolist() == [3 + 4, 1, 1]
    base = 1 << 40
    assert c["contrast"].tolist() == [[2 * base + 2 + 4, 2 * base + 3 + 5], [base + 6, base + 7], [base + 10, base + 11]]
    then = np.array([[0, 0, 1, 1, -1], [2, 2, 0, 9, 9]], np.int32)
    assert M.compose(mapping, then).tolist() == [[0, 0, 0, 1, 1], [2, 2, 2, 0, 0]]
    assert M.compose(np.array([[3, -1, 7]], np.int32), then[:1]).tolist() == [[1, -1, -1]]
    lab = np.array([[[0, 1, 4], [5, -1, 2]], [[4, 4, 0], [3, 2, 1]]], np.int16)
    assert M.labels(lab, mapping).tolist() == [[[0, 0, 3], [-1, -1, 1]], [[2, 2, 0], [2, 1, 1]]]
    assert M.labels(lab[0], np.array([7, -1, 8, 9, 9], np.int32)).tolist() == [[7, -1, 9], [-1, -1, 8]]


# ---- the contraction identity: contract(graph(labels), mapping, K2) == graph(labels(labels, mapping), K2) ----
def random_mapping(rng, N, K, groups):
    mapping = rng.integers(0, groups, (N, K)).astype(np.int32)
    mapping[rng.random((N, K)) < 0.1] = -1
    return mapping


@pytest.mark.parametrize("kind,H,W,K", [("blocky", 23, 37, 40), ("noise", 17, 19, 12), ("blocky", 1, 50, 9), ("noise", 31, 1, 5)])
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("with_image", [False, True])
def test_contraction_identity(kind, H, W, K, connectivity, with_image):
    rng = np.random.default_rng(H * 100 + W + connectivity)
    maps = np.stack([(connect_ref.blocky if kind == "blocky" else connect_ref.noise)(H, W, K + 3, seed=H * 1000 + W + i) for i in range(2)])
    maps[0][rng.random((H, W)) < 0.05] = -1                                          # labels of -1 and >= K (K + 3 labels were drawn)
    image = rng.integers(0, 256, (2, H, W, 3)).astype(np.uint8) if with_image else None
    g = rag_ref.graph(maps, K, connectivity, image)
    for groups, K2 in ((K, K), (max(K // 3, 1), max(K // 3, 1)), (7, 4), (1, 1)):    # (7, 4): a K2 below n drops the groups 4 .. 6
        mapping = random_mapping(rng, 2, K, groups)
        got = M.contract(g, mapping, K2)
        want = rag_ref.graph(M.labels(maps, mapping), K2, connectivity, image)
        assert M.same_graph(got, want), (groups, K2)
    # the mappings of a round: the identity holds for them as for any other
    w = rng.integers(0, 4, g["boundary"].shape[0]).astype(np.float32)
    members = np.stack([np.bincount(m[(m >= 0) & (m < K)], minlength=K) for m in maps])
    mapping, n = M.components(g, M.best_edges(g, w, 3.0), K, members)
    assert all(np.array_equal(np.unique(mapping[f][mapping[f] >= 0]), np.arange(n[f])) for f in range(2))
    assert M.same_graph(M.contract(g, mapping, K), rag_ref.graph(M.labels(maps, mapping), K, connectivity, image))
    single = rag_ref.graph(maps[1], K, connectivity, None if image is None else image[1])      # an [H, W] map: N = 1
    assert M.same_graph(M.contract(single, mapping[1:], K), rag_ref.graph(M.labels(maps[1], mapping[1]), K, connectivity,
                                                                          None if image is None else image[1]))


def test_capacities():
    assert contract_capacity_limit(1600, 4700) == 16384                              # the first table holds every edge
    assert contract_capacity_limit(1600, 1 << 20) == 1 << 21
    assert contract_capacity_limit(400, 1 << 20) == 1 << 18                          # 2 * 400 * 399 / 2 label pairs
    assert contract_capacity_limit(65534, (1 << 31) - 1) == 1 << 31


# ---- argument errors: all before any device work (a CPU tensor is the last thing refused) ----
def cpu_graph(N=2, K=5, E=7, Cc=2):
    off = torch.zeros(N + 1, dtype=torch.int64)
    off[-1] = E
    return SuperpixelGraph(torch.zeros((2, E), dtype=torch.int64), torch.zeros(E, dtype=torch.int32),
                           torch.zeros((E, Cc), dtype=torch.int64) if Cc else None, off, K, 1024)


def broken(**fields):
    g = cpu_graph()
    for k, v in fields.items():
        setattr(g, k, v)
    return g


BAD_GRAPHS = [
    (None, "SuperpixelGraph"), ({"edge_index": 0}, "SuperpixelGraph"),
    (broken(num_components=0), "num_components"), (broken(num_components=65535), "num_components"), (broken(num_components=5.0), "num_components"),
    (broken(edge_index=torch.zeros((2, 7), dtype=torch.int32)), "edge_index must be int64"),
    (broken(edge_index=torch.zeros((7, 2), dtype=torch.int64)), r"edge_index must be \[2, E\]"),
    (broken(edge_index=np.zeros((2, 7), np.int64)), "edge_index must be a torch tensor"),
    (broken(offsets=torch.zeros(3, dtype=torch.int32)), "offsets must be int64"),
    (broken(offsets=torch.zeros((3, 1), dtype=torch.int64)), "offsets must be"), (broken(offsets=torch.zeros(1, dtype=torch.int64)), "offsets must be"),
    (broken(boundary=torch.zeros(7, dtype=torch.int64)), "boundary must be int32"), (broken(boundary=torch.zeros(6, dtype=torch.int32)), "boundary must be"),
    (broken(contrast=torch.zeros((7, 2), dtype=torch.int32)), "contrast must be int64"),
    (broken(contrast=torch.zeros((7, 5), dtype=torch.int64)), "contrast must be"), (broken(contrast=torch.zeros((6, 2), dtype=torch.int64)), "contrast must be"),
    (broken(contrast=torch.zeros(7, dtype=torch.int64)), "contrast must be"),
]
W7, J7, MAP = torch.zeros(7), torch.zeros(7, dtype=torch.bool), torch.zeros((2, 5), dtype=torch.int32)


@pytest.mark.parametrize("graph,match", BAD_GRAPHS)
def test_bad_graphs(graph, match):
    for call in (lambda: best_neighbour_edges(graph, W7), lambda: merge_components(graph, J7), lambda: contract_graph(graph, MAP, 5)):
        with pytest.raises(ValueError, match=match):
            call()


@pytest.mark.parametrize("weight,match", [
    (torch.zeros(6), r"weight must be \[E\]"), (torch.zeros(8), r"weight must be \[E\]"), (torch.zeros((7, 1)), r"weight must be \[E\]"),
    (torch.zeros(7, dtype=torch.float64), "weight must be float32"), (torch.zeros(7, dtype=torch.int32), "weight must be float32"),
    (np.zeros(7, np.float32), "weight must be a torch tensor"), (None, "weight must be a torch tensor"),
])
def test_bad_weight(weight, match):
    with pytest.raises(ValueError, match=match):
        best_neighbour_edges(cpu_graph(), weight)


@pytest.mark.parametrize("threshold", [True, "1", [1.0], torch.zeros(()), 1j])
def test_bad_threshold(threshold):
    with pytest.raises(ValueError, match="threshold"):
        best_neighbour_edges(cpu_graph(), W7, threshold)


@pytest.mark.parametrize("join,match", [
    (torch.zeros(6, dtype=torch.bool), r"join must be \[E\]"), (torch.zeros((1, 7), dtype=torch.bool), r"join must be \[E\]"),
    (torch.zeros(7, dtype=torch.uint8), "join must be bool"), (torch.zeros(7), "join must be bool"), ([False] * 7, "join must be a torch tensor"),
])
def test_bad_join(join, match):
    with pytest.raises(ValueError, match=match):
        merge_components(cpu_graph(), join)


@pytest.mark.parametrize("members,N,match", [
    (torch.zeros((2, 4), dtype=torch.int32), 2, "members must be"), (torch.zeros((1, 5), dtype=torch.int32), 2, "members must be"),
    (torch.zeros(5, dtype=torch.int32), 2, "members must be"), (torch.zeros(4, dtype=torch.int64), 1, "members must be"),
    (torch.zeros((1, 1, 5), dtype=torch.int32), 1, "members must be"),
    (torch.zeros((2, 5), dtype=torch.int16), 2, "members must be int32 or int64"), (torch.zeros((2, 5)), 2, "members must be int32 or int64"),
    (np.zeros((2, 5), np.int32), 2, "members must be a torch tensor"),
])
def test_bad_members(members, N, match):
    with pytest.raises(ValueError, match=match):
        merge_components(cpu_graph(N=N), J7, members)


@pytest.mark.parametrize("mapping,match", [
    (torch.zeros((2, 4), dtype=torch.int32), "mapping must be"), (torch.zeros((3, 5), dtype=torch.int32), "mapping must be"),
    (torch.zeros(5, dtype=torch.int32), "mapping must be"), (torch.zeros((2, 5), dtype=torch.int64), "mapping must be int32"),
    (np.zeros((2, 5), np.int32), "mapping must be a torch tensor"),
])
def test_bad_mapping_of_a_contraction(mapping, match):
    with pytest.raises(ValueError, match=match):
        contract_graph(cpu_graph(), mapping, 5)


@pytest.mark.parametrize("K2", [0, -1, 65535, 2.0, True, "4", None])
def test_bad_bound_of_a_contraction(K2):
    with pytest.raises(ValueError, match="num_components"):
        contract_graph(cpu_graph(), MAP, K2)


@pytest.mark.parametrize("cap", [0, 32, 1000, 1 << 32, 2048.0, True])
def test_bad_start_capacity(cap):
    with pytest.raises(ValueError, match="_start_capacity"):
        contract_graph(cpu_graph(), MAP, 5, _start_capacity=cap)


LAB = np.zeros((2, 4, 6), np.int16)


@pytest.mark.parametrize("labels,mapping,match", [
    (LAB.astype(np.float32), MAP, "int16"), (LAB.astype(np.uint8), MAP, "int16"), ([[0]], MAP, "numpy array or a torch tensor"),
    (np.zeros(6, np.int16), MAP, r"\[H, W\]"), (np.zeros((2, 0, 6), np.int16), MAP, "empty"),
    (np.broadcast_to(np.zeros((), np.int16), (1 << 11, 1 << 10, 1 << 10)), MAP, r"2\^31"),
    (LAB, torch.zeros((3, 5), dtype=torch.int32), "mapping must be"), (LAB, torch.zeros(5, dtype=torch.int32), "mapping must be"),
    (LAB[0], torch.zeros((2, 5), dtype=torch.int32), "mapping must be"), (LAB, torch.zeros((2, 5), dtype=torch.int64), "mapping must be int32"),
    (LAB, np.zeros((2, 5), np.int32), "mapping must be a torch tensor"), (LAB, torch.zeros((2, 65535), dtype=torch.int32), "num_components"),
    (LAB, torch.zeros((2, 0), dtype=torch.int32), "mapping must be"),
])
def test_bad_arguments_of_merge_labels(labels, mapping, match):
    with pytest.raises(ValueError, match=match):
        merge_labels(labels, mapping)


@pytest.mark.parametrize("first,then,match", [
    (MAP.long(), MAP, "first must be int32"), (MAP, MAP.long(), "then must be int32"), (MAP[0], MAP, "first must be"),
    (MAP, torch.zeros((3, 5), dtype=torch.int32), "then must be"), (MAP, MAP[0], "then must be"), (MAP.numpy(), MAP, "first must be a torch tensor"),
])
def test_bad_arguments_of_compose_mappings(first, then, match):
    with pytest.raises(ValueError, match=match):
        compose_mappings(first, then)


def test_cpu_tensors_are_refused_after_every_other_check():
    g = cpu_graph()
    with pytest.raises(ValueError, match="graph.edge_index must be on a ROCm GPU"):
        best_neighbour_edges(g, W7, 0.5)
    with pytest.raises(ValueError, match="no CPU fallback"):
        merge_components(g, J7, torch.ones((2, 5), dtype=torch.int64))
    with pytest.raises(ValueError, match="no CPU fallback"):
        merge_components(cpu_graph(N=1, E=0, Cc=0), torch.zeros(0, dtype=torch.bool), torch.ones(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="no CPU fallback"):
        contract_graph(g, MAP, 5, _start_capacity=64)
    with pytest.raises(ValueError, match="mapping must be on a ROCm GPU"):
        merge_labels(LAB, MAP)
    with pytest.raises(ValueError, match="labels must be on a ROCm GPU"):
        merge_labels(torch.from_numpy(LAB[0]), MAP[:1])
    with pytest.raises(ValueError, match="first must be on a ROCm GPU"):
        compose_mappings(MAP, MAP)


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
P = C.c_void_p(0x1000)
NUL = None
BIG = 1 << 40


def lib():
    lib = B.load_library()
    assert hasattr(lib, "fslic_hip_merge_components")
    return lib


def test_exports_and_workspace_sizes():
    names = ["fslic_hip_merge_best_workspace_size", "fslic_hip_merge_best_edges", "fslic_hip_merge_components_workspace_size",
             "fslic_hip_merge_components", "fslic_hip_merge_labels", "fslic_hip_merge_contract_accumulate"]
    assert sorted(n for n in B.EXPORTS if "_merge_" in n) == sorted(names) and all(hasattr(lib(), n) for n in names)
    n = C.c_size_t()
    assert lib().fslic_hip_merge_best_workspace_size(8, 1600, C.byref(n)) == 0 and n.value == 8 * 1600 * 8
    assert lib().fslic_hip_merge_components_workspace_size(8, 1600, C.byref(n)) == 0 and n.value == 2 * 8 * 1600 * 4 + 8 * 7 * 4
    assert lib().fslic_hip_merge_components_workspace_size(1, 1, C.byref(n)) == 0 and n.value == 16 + 16 + 16
    assert lib().fslic_hip_merge_components_workspace_size(3, 65534, C.byref(n)) == 0 and n.value == 2 * (3 * 65534 * 4 + 8) + 3 * 256 * 4
    for f in (lib().fslic_hip_merge_best_workspace_size, lib().fslic_hip_merge_components_workspace_size):
        for N, K in ((0, 4), (-1, 4), (1, 0), (1, 65535), (1 << 16, 1 << 15)):
            assert f(N, K, C.byref(n)) == B.FSLIC_E_INVALID, (N, K)
        assert f(1, 4, None) == B.FSLIC_E_INVALID


GRAPH_REFUSALS = [dict(device=-1), dict(N=0), dict(K=0), dict(K=65535), dict(N=1 << 16, K=1 << 15), dict(E=-1), dict(E=1 << 31), dict(ei=NUL),
                  dict(off=NUL), dict(ws=NUL), dict(nbytes=0)]


@pytest.mark.parametrize("kw", GRAPH_REFUSALS + [dict(weight=NUL), dict(join=NUL), dict(nbytes=2 * 5 * 8 - 1)])
def test_capi_best_edges_refuses(kw):
    a = dict(device=0, N=2, K=5, E=7, ei=P, off=P, weight=P, join=P, ws=P, nbytes=BIG)
    a.update(kw)
    assert lib().fslic_hip_merge_best_edges(a["device"], NUL, a["N"], a["K"], a["E"], a["ei"], a["off"], a["weight"], 1, 0.5, a["join"],
                                            a["ws"], a["nbytes"]) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", GRAPH_REFUSALS + [dict(join=NUL), dict(mtype=0), dict(mtype=3), dict(mapping=NUL), dict(counts=NUL),
                                                 dict(nbytes=48 + 48 + 16 - 1)])
def test_capi_components_refuses(kw):
    a = dict(device=0, N=2, K=5, E=7, ei=P, off=P, join=P, members=P, mtype=1, mapping=P, counts=P, ws=P, nbytes=BIG)
    a.update(kw)
    assert lib().fslic_hip_merge_components(a["device"], NUL, a["N"], a["K"], a["E"], a["ei"], a["off"], a["join"], a["members"], a["mtype"],
                                            a["mapping"], a["counts"], a["ws"], a["nbytes"]) == B.FSLIC_E_INVALID
    if "nbytes" in kw and kw["nbytes"]:
        assert b"workspace too small: 112 bytes" in lib().fslic_hip_last_error()


@pytest.mark.parametrize("kw", [dict(device=-1), dict(N=0), dict(K=0), dict(K=65535), dict(H=0), dict(W=-2), dict(H=1 << 16, W=1 << 15),
                                dict(N=2, H=1 << 15, W=1 << 15), dict(ltype=3), dict(ltype=-1), dict(lab=NUL), dict(mapping=NUL), dict(out=NUL),
                                dict(out=C.c_void_p(0x1002))])
def test_capi_labels_refuses(kw):
    a = dict(device=0, N=1, H=4, W=6, K=5, lab=P, ltype=0, mapping=P, out=P)
    a.update(kw)
    assert lib().fslic_hip_merge_labels(a["device"], NUL, a["N"], a["H"], a["W"], a["K"], a["lab"], a["ltype"], a["mapping"],
                                        a["out"]) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", GRAPH_REFUSALS + [dict(K2=0), dict(K2=65535), dict(boundary=NUL), dict(mapping=NUL), dict(contrast=NUL), dict(Cc=0),
                                                 dict(Cc=5), dict(Cc=-1), dict(cap=0), dict(cap=32), dict(cap=1000), dict(cap=1 << 32),
                                                 dict(nbytes=32 + 2 * 1024 * 24 - 1)])
def test_capi_contract_refuses(kw):
    a = dict(device=0, N=2, K=5, K2=5, E=7, ei=P, off=P, boundary=P, contrast=P, Cc=2, mapping=P, cap=1024, ws=P, nbytes=BIG)
    a.update(kw)
    assert lib().fslic_hip_merge_contract_accumulate(a["device"], NUL, a["N"], a["K"], a["K2"], a["E"], a["ei"], a["off"], a["boundary"],
                                                     a["contrast"], a["Cc"], a["mapping"], a["cap"], a["ws"], a["nbytes"]) == B.FSLIC_E_INVALID
