"""CPU tests of merging regions by similarity (fast_slic_amd/regions.py, the fslic_hip_region* entries): the model
(tests/region_ref.py) by hand on a triangle, a path and two frames; the forest property of joined edges and what a quota makes of it;
the model's driver with a target; and every argument error refused before any device work -- ValueError in Python, FSLIC_E_INVALID
from the C ABI before its first HIP call.  No kernel is launched here."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import connect_ref
import merge_ref as M
import rag_ref
import region_ref as R
from fast_slic_amd import _binding as B
from fast_slic_amd.rag import SuperpixelGraph
from fast_slic_amd.regions import MergeResult, edge_weights, group_sums, limit_joins, merge_hierarchical
from test_merge_cpu import BAD_GRAPHS, PATH, TRIANGLE, cpu_graph, graph_of

F32 = np.float32
INF = float("inf")


def f32(*v):
    return np.array(v, F32)


# ---- the rules, by hand ----
def test_triangle():
    g = graph_of([TRIANGLE])                                               # (0,1), (0,2), (1,2)
    sums, counts = f32(2, 6, 20).reshape(1, 1, 3), np.array([[2, 3, 5]], np.int32)      # means 1, 2, 4
    assert R.edge_weights(g, sums, counts).tolist() == [1.0, 3.0, 2.0]
    assert R.edge_weights(g, sums, counts, "ward").tolist() == [F32(6) / F32(5) * F32(1), F32(10) / F32(7) * F32(9), F32(15) / F32(8) * F32(4)]
    two = np.concatenate([sums, f32(0, 12, 20).reshape(1, 1, 3)], axis=1)  # a second channel: means 0, 4, 4
    assert R.edge_weights(g, two, counts).tolist() == [np.sqrt(F32(17)), F32(5), F32(2)]
    assert R.edge_weights(g, two[0], counts[0]).tolist() == [np.sqrt(F32(17)), F32(5), F32(2)]      # [C, K] and [K] with N = 1
    counts[0, 2] = 0                                                       # a node without members: its edges are +inf
    assert R.edge_weights(g, sums, counts).tolist() == [1.0, INF, INF]
    counts[0, 2] = -4
    assert R.edge_weights(g, sums, counts, "ward").tolist() == [F32(6) / F32(5), INF, INF]
    s, c = R.group_sums(sums, [[0, 0, 1]], 2, np.array([[2, 3, 5]], np.int64))
    assert s.tolist() == [[[8.0, 20.0]]] and c.tolist() == [[5, 5]] and c.dtype == np.int64
    s = R.group_sums(sums, [[1, -1, 7]], 4)                                # -1 and a group >= K2 add nothing; empty groups are +0.0
    assert s.tolist() == [[[0.0, 2.0, 0.0, 0.0]]] and not np.signbit(s).any()


def test_group_sums_round_once():
    """2^24 + 1 + 1: added one after the other in float32 the ones are lost; the exact sum rounds 2^24 + 2 once.  And a sum that
    cancels to zero is +0.0, a tie goes to even, a value below 2^-96 is truncated away."""
    big = F32(2 ** 24)
    vals = f32(big, 1, 1, -3, 3, 2 ** 24, 1, 2.0 ** -97, -2.0 ** -97).reshape(1, 1, 9)
    assert (big + F32(1)) + F32(1) == big
    s = R.group_sums(vals, [[0, 0, 0, 1, 1, 2, 2, 3, 3]], 4)
    assert s.tolist() == [[[2.0 ** 24 + 2, 0.0, 2.0 ** 24, 0.0]]] and not np.signbit(s).any()
    assert R.group_sums(f32(1, 2.0 ** -96 * 1.5).reshape(1, 1, 2), [[0, 1]], 2).view(np.uint32)[0, 0, 1] == struct.unpack("<I", struct.pack("<f", 2.0 ** -96))[0]


def test_path_and_quota():
    g = graph_of([PATH])                                                   # (0,1), (1,2), (2,3), (3,4)
    w = f32(3, 1, 2, 5)
    join = M.best_edges(g, w)                                              # all four (test_merge_cpu.test_path)
    assert R.limit_joins(g, w, join, [0]).tolist() == [False] * 4
    assert R.limit_joins(g, w, join, [-3]).tolist() == [False] * 4
    assert R.limit_joins(g, w, join, [1]).tolist() == [False, True, False, False]
    assert R.limit_joins(g, w, join, [3]).tolist() == [True, True, True, False]
    assert R.limit_joins(g, w, join, [4]).tolist() == [True] * 4 and R.limit_joins(g, w, join, [99]).tolist() == [True] * 4
    assert R.limit_joins(g, w, [True, False, True, True], [2]).tolist() == [True, False, True, False]      # only joined edges are kept
    assert R.limit_joins(g, f32(1, 1, 1, 1), join, [2]).tolist() == [True, True, False, False]             # equal weights: the position
    assert R.limit_joins(g, f32(0.0, -0.0, 0.0, -0.0), join, [3]).tolist() == [True, True, True, False]     # -0.0 is +0.0
    assert R.limit_joins(g, f32(INF, 1, INF, 2), join, [4]).tolist() == [False, True, False, True]          # +inf is never kept


def test_two_frames():
    g = graph_of([TRIANGLE, PATH])
    w = f32(1, 1, 1, 2, 2, 2, 2)
    join = M.best_edges(g, w)                                              # [T, T, F, T, T, T, T]: positions are per frame
    assert R.limit_joins(g, w, join, [1, 2]).tolist() == [True, False, False, True, True, False, False]
    assert R.limit_joins(g, w, join, [5, 0]).tolist() == [True, True, False, False, False, False, False]
    sums = np.stack([f32(1, 2, 4, 0, 0), f32(0, 10, 0, 10, 0)]).reshape(2, 1, 5)
    counts = np.array([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1]], np.int32)
    assert R.edge_weights(g, sums, counts).tolist() == [1.0, 3.0, 2.0, 10.0, 10.0, 10.0, 10.0]
    # one round, no threshold: frame 0's nodes all join (0-1 is best of 0 and 1, 1-2 of 2); frame 1: all four edges tie, every node
    # takes its lower edge, which joins everything
    r = R.merge_hierarchical(g, sums, counts, max_rounds=1)
    assert r["mapping"].tolist() == [[0, 0, 0, -1, -1], [0, 0, 0, 0, 0]] and r["n"].tolist() == [1, 1]
    assert r["sums"].tolist() == [[[7.0, 0, 0, 0, 0]], [[20.0, 0, 0, 0, 0]]] and r["counts"].tolist() == [[3, 0, 0, 0, 0], [5, 0, 0, 0, 0]]
    assert r["graph"]["offsets"].tolist() == [0, 0, 0]
    # a target of 2: frame 0 has 3 regions and may join once (its lightest edge, 0-1), frame 1 has 5 and joins its first three edges
    r = R.merge_hierarchical(g, sums, counts, target=2)
    assert r["mapping"].tolist() == [[0, 0, 1, -1, -1], [0, 0, 0, 0, 1]] and r["n"].tolist() == [2, 2]
    # a threshold of 1.5 lets only frame 0's edge 0-1 (1.0), and after that none (means 1.5 and 4), join
    r = R.merge_hierarchical(g, sums, counts, threshold=1.5)
    assert r["mapping"].tolist() == [[0, 0, 1, -1, -1], [0, 1, 2, 3, 4]] and r["n"].tolist() == [2, 5] and r["rounds"] == 2
    assert r["sums"][0, 0].tolist() == [3.0, 4.0, 0, 0, 0] and r["graph"]["edge_index"].tolist() == [[0, 0, 1, 2, 3], [1, 1, 2, 3, 4]]


# ---- the forest property: the joined edges of distinct keys close no cycle, so each kept edge removes exactly one group ----
def random_graph(rng, N, K, p):
    frames = []
    for _ in range(N):
        pairs = [(a, b, 1) for a in range(K) for b in range(a + 1, K) if rng.random() < p]
        frames.append(pairs)
    return graph_of(frames)


@pytest.mark.parametrize("seed,K,p,levels", [(0, 12, 0.5, 1), (1, 30, 0.2, 2), (2, 30, 0.5, 3), (3, 60, 0.08, 2), (4, 9, 1.0, 1)])
def test_joined_edges_are_a_forest(seed, K, p, levels):
    rng = np.random.default_rng(seed)
    N = 3
    g = random_graph(rng, N, K, p)
    E = g["boundary"].shape[0]
    w = rng.integers(0, levels, E).astype(F32)                             # heavy ties: the position decides most of them
    w[rng.random(E) < 0.3] *= F32(-0.0) if levels == 1 else F32(1)
    join = M.best_edges(g, w)
    a, b = g["edge_index"]
    for f, (lo, hi) in enumerate(M.frames_of(g)):
        parent = list(range(K))

        def find(v):
            while parent[v] != v:
                v = parent[v]
            return v

        for e in range(lo, hi):
            if join[e]:
                ra, rb = find(int(a[e])), find(int(b[e]))
                assert ra != rb, "a joined edge closes a cycle"
                parent[ra] = rb
    joined = np.array([join[lo:hi].sum() for lo, hi in M.frames_of(g)])
    assert np.array_equal(M.components(g, join, K)[1], K - joined)
    for quota in ([0, 1, 2], joined, joined + 1, joined // 2):
        kept = R.limit_joins(g, w, join, quota)
        assert not (kept & ~join).any()
        assert np.array_equal(M.components(g, kept, K)[1], K - np.minimum(np.asarray(quota), joined))


# ---- the driver with a target ----
@pytest.mark.parametrize("kind,H,W,K,mode", [("blocky", 23, 37, 40, "mean"), ("noise", 17, 19, 12, "ward"), ("blocky", 40, 50, 25, "ward")])
def test_driver_reaches_its_target(kind, H, W, K, mode):
    rng = np.random.default_rng(H + W)
    maps = np.stack([(connect_ref.blocky if kind == "blocky" else connect_ref.noise)(H, W, K + 3, seed=H * 1000 + W + i) for i in range(2)])
    half = (K + 3) // 2                                                    # frame 0: the labels below `half` left of a wall of no label,
    maps[0][:, :W // 2] %= half                                            # the others right of it: its graph falls apart
    maps[0][:, W // 2:] = half + maps[0][:, W // 2:] % (K + 3 - half)
    maps[0][:, W // 2] = -1
    g = rag_ref.graph(maps, K + 5, 4)                                      # the nodes K + 3 .. K + 4 have no pixel
    K = K + 5
    counts = np.stack([np.bincount(m[(m >= 0) & (m < K)], minlength=K) for m in maps]).astype(np.int32)
    sums = (rng.integers(0, 50, (2, 3, K)) * counts[:, None]).astype(F32)
    comps = R.graph_components(g, K, counts)
    assert comps[0] > 1 and (counts == 0).any()
    for target in (1, 2, 7, int((counts > 0).sum(1).min()), K + 1):
        r = R.merge_hierarchical(g, sums, counts, target=target, max_rounds=32, mode=mode)
        assert r["n"].tolist() == np.minimum(np.maximum(target, comps), (counts > 0).sum(1)).tolist(), target
        assert (r["n"] >= np.minimum(target, (counts > 0).sum(1))).all()
        for f in range(2):
            assert np.array_equal(np.unique(r["mapping"][f][r["mapping"][f] >= 0]), np.arange(r["n"][f]))
        s, c = R.group_sums(sums, r["mapping"], K, counts)                 # the invariant of rule 4
        assert np.array_equal(s.view(np.uint32), r["sums"].view(np.uint32)) and np.array_equal(c, r["counts"])
        assert c.sum() == counts.sum() and M.same_graph(r["graph"], M.contract(g, r["mapping"], K))
    short = R.merge_hierarchical(g, sums, counts, target=1, max_rounds=1, mode=mode)        # the rounds ran out
    assert (short["n"] > comps).all() and short["rounds"] == 1


# ---- argument errors: all before any device work (a CPU tensor is the last thing refused) ----
S, CN, W7, J7, Q = torch.zeros((2, 3, 5)), torch.ones((2, 5), dtype=torch.int32), torch.zeros(7), torch.zeros(7, dtype=torch.bool), torch.ones(2, dtype=torch.int32)
MAP = torch.zeros((2, 5), dtype=torch.int32)


@pytest.mark.parametrize("graph,match", BAD_GRAPHS)
def test_bad_graphs(graph, match):
    for call in (lambda: edge_weights(graph, S, CN), lambda: limit_joins(graph, W7, J7, Q), lambda: merge_hierarchical(graph, S, CN)):
        with pytest.raises(ValueError, match=match):
            call()


BAD_SUMS = [
    (torch.zeros((2, 3, 4)), r"must be \[N, C, K\]"), (torch.zeros((3, 3, 5)), r"must be \[N, C, K\]"), (torch.zeros((3, 5)), r"must be \[N, C, K\]"),
    (torch.zeros((2, 0, 5)), r"must be \[N, C, K\]"), (torch.zeros((2, 3, 5, 1)), r"must be \[N, C, K\]"),
    (torch.zeros((2, 3, 5), dtype=torch.float64), "must be float32"), (torch.zeros((2, 3, 5), dtype=torch.float16), "must be float32"),
    (torch.zeros((2, 3, 5), dtype=torch.int32), "must be float32"), (np.zeros((2, 3, 5), np.float32), "must be a torch tensor"), (None, "must be a torch tensor"),
]
BAD_COUNTS = [
    (torch.ones((2, 4), dtype=torch.int32), "counts must be"), (torch.ones((1, 5), dtype=torch.int32), "counts must be"), (torch.ones(5, dtype=torch.int32), "counts must be"),
    (torch.ones((2, 5, 1), dtype=torch.int64), "counts must be"), (torch.ones((2, 5), dtype=torch.int16), "counts must be int32 or int64"),
    (torch.ones((2, 5)), "counts must be int32 or int64"), (np.ones((2, 5), np.int32), "counts must be a torch tensor"),
]


@pytest.mark.parametrize("sums,match", BAD_SUMS)
def test_bad_sums(sums, match):
    for call in (lambda: edge_weights(cpu_graph(), sums, CN), lambda: merge_hierarchical(cpu_graph(), sums, CN)):
        with pytest.raises(ValueError, match="sums " + match):
            call()
    with pytest.raises(ValueError, match="values " + match):
        group_sums(sums, MAP, 5)


@pytest.mark.parametrize("counts,match", BAD_COUNTS + [(None, "counts must be a torch tensor")])
def test_bad_counts(counts, match):
    for call in (lambda: edge_weights(cpu_graph(), S, counts), lambda: merge_hierarchical(cpu_graph(), S, counts)):
        with pytest.raises(ValueError, match=match):
            call()


@pytest.mark.parametrize("counts,match", BAD_COUNTS)
def test_bad_counts_of_group_sums(counts, match):
    with pytest.raises(ValueError, match=match):
        group_sums(S, MAP, 5, counts)


def test_single_frame_shapes_are_allowed_only_with_one_frame():
    one = cpu_graph(N=1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        edge_weights(one, torch.zeros((3, 5)), torch.ones(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="no CPU fallback"):
        merge_hierarchical(one, torch.zeros((3, 5)), torch.ones(5, dtype=torch.int64), target=2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        group_sums(torch.zeros((3, 5)), MAP[:1], 7, torch.ones(5, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"values must be \[N, C, K\]"):
        group_sums(torch.zeros((3, 5)), MAP, 7)


@pytest.mark.parametrize("mode", ["Mean", "", "l2", None, 0, b"mean", ["mean"]])
def test_bad_mode(mode):
    for call in (lambda: edge_weights(cpu_graph(), S, CN, mode), lambda: merge_hierarchical(cpu_graph(), S, CN, mode=mode)):
        with pytest.raises(ValueError, match="mode must be 'mean' or 'ward'"):
            call()


@pytest.mark.parametrize("mapping,match", [
    (torch.zeros(5, dtype=torch.int32), r"mapping must be \[N, K\]"), (torch.zeros((2, 0), dtype=torch.int32), r"mapping must be \[N, K\]"),
    (torch.zeros((0, 5), dtype=torch.int32), r"mapping must be \[N, K\]"), (torch.zeros((2, 65535), dtype=torch.int32), r"mapping must be \[N, K\]"),
    (torch.zeros((2, 5), dtype=torch.int64), "mapping must be int32"), (np.zeros((2, 5), np.int32), "mapping must be a torch tensor"),
])
def test_bad_mapping_of_group_sums(mapping, match):
    with pytest.raises(ValueError, match=match):
        group_sums(S, mapping, 5)


@pytest.mark.parametrize("K2", [0, -1, 65535, 2.0, True, "4", None])
def test_bad_num_groups(K2):
    with pytest.raises(ValueError, match="num_groups"):
        group_sums(S, MAP, K2)


def test_group_sums_refuses_2_to_the_31_cells():
    big = torch.zeros((1, 1, 1)).expand(1, 1 << 16, 1 << 15)
    with pytest.raises(ValueError, match=r"N \* C \* K must be below 2\^31"):
        group_sums(big, torch.zeros((1, 1 << 15), dtype=torch.int32), 1)
    with pytest.raises(ValueError, match=r"N \* C \* num_groups must be below 2\^31"):
        group_sums(torch.zeros((1, 1, 1)).expand(1, 1 << 16, 4), torch.zeros((1, 4), dtype=torch.int32), 1 << 15)


@pytest.mark.parametrize("weight,match", [
    (torch.zeros(6), r"weight must be \[E\]"), (torch.zeros((7, 1)), r"weight must be \[E\]"), (torch.zeros(7, dtype=torch.float64), "weight must be float32"),
    (np.zeros(7, np.float32), "weight must be a torch tensor"),
])
def test_bad_weight(weight, match):
    with pytest.raises(ValueError, match=match):
        limit_joins(cpu_graph(), weight, J7, Q)


@pytest.mark.parametrize("join,match", [
    (torch.zeros(6, dtype=torch.bool), r"join must be \[E\]"), (torch.zeros(7, dtype=torch.uint8), "join must be bool"), ([False] * 7, "join must be a torch tensor"),
])
def test_bad_join(join, match):
    with pytest.raises(ValueError, match=match):
        limit_joins(cpu_graph(), W7, join, Q)


@pytest.mark.parametrize("quota,match", [
    (torch.ones(3, dtype=torch.int32), r"quota must be \[N\]"), (torch.ones((2, 1), dtype=torch.int32), r"quota must be \[N\]"),
    (torch.ones((), dtype=torch.int64), r"quota must be \[N\]"), (torch.ones(2), "quota must be int32 or int64"), (torch.ones(2, dtype=torch.int16), "quota must be int32 or int64"),
    ([1, 1], "quota must be a torch tensor"), (1, "quota must be a torch tensor"),
])
def test_bad_quota(quota, match):
    with pytest.raises(ValueError, match=match):
        limit_joins(cpu_graph(), W7, J7, quota)


@pytest.mark.parametrize("kw,match", [
    (dict(threshold=True), "threshold"), (dict(threshold="1"), "threshold"), (dict(threshold=torch.zeros(())), "threshold"), (dict(threshold=1j), "threshold"),
    (dict(target=0), "target must be None or an integer >= 1"), (dict(target=-2), "target"), (dict(target=2.0), "target"), (dict(target=True), "target"),
    (dict(target="3"), "target"), (dict(target=torch.ones(2, dtype=torch.int32)), "target"),
    (dict(max_rounds=0), "max_rounds must be an integer >= 1"), (dict(max_rounds=-1), "max_rounds"), (dict(max_rounds=2.0), "max_rounds"),
    (dict(max_rounds=None), "max_rounds"), (dict(max_rounds=True), "max_rounds"),
])
def test_bad_options_of_merge_hierarchical(kw, match):
    with pytest.raises(ValueError, match=match):
        merge_hierarchical(cpu_graph(), S, CN, **kw)


def test_cpu_tensors_are_refused_after_every_other_check():
    g = cpu_graph()
    with pytest.raises(ValueError, match="graph.edge_index must be on a ROCm GPU"):
        edge_weights(g, S, CN, "ward")
    with pytest.raises(ValueError, match="no CPU fallback"):
        limit_joins(g, W7, J7, Q.long())
    with pytest.raises(ValueError, match="graph.edge_index must be on a ROCm GPU"):
        merge_hierarchical(g, S, CN.long(), threshold=0.5, target=3, max_rounds=2, mode="ward")
    with pytest.raises(ValueError, match="values must be on a ROCm GPU"):
        group_sums(S, MAP, 65534, CN)
    with pytest.raises(ValueError, match="no CPU fallback"):
        group_sums(S, MAP, 1)
    assert MergeResult(1, 2, 3, 4, 5).graph == 3


def test_mismatched_devices_are_named_before_a_cpu_tensor():
    """No GPU here, let alone two: the device check is exercised through the helpers with stand-ins that have a device and nothing else."""
    from fast_slic_amd._tensors import one_device as _one_device
    from fast_slic_amd.rag import graph_device as _graph_device

    class On(object):
        def __init__(self, device):
            self.device = torch.device(device)

    with pytest.raises(ValueError, match=r"values, mapping, counts must be on one GPU, got \['cuda:0', 'cuda:1'\]"):
        _one_device(((On("cuda:0"), "values"), (On("cuda:1"), "mapping"), (On("cpu"), "counts")))
    with pytest.raises(ValueError, match="counts must be on a ROCm GPU"):
        _one_device(((On("cuda:1"), "values"), (On("cuda:1"), "mapping"), (On("cpu"), "counts")))
    assert _one_device(((On("cuda:1"), "values"), (None, "counts"))) == torch.device("cuda:1")
    g = SuperpixelGraph(On("cuda:0"), On("cuda:0"), None, On("cuda:0"), 5, 1024)      # the graph's route (edge_weights, limit_joins, the loop)
    with pytest.raises(ValueError, match=r"graph.edge_index, graph.offsets, graph.boundary, sums, counts must be on one GPU"):
        _graph_device(g, ((On("cuda:0"), "sums"), (On("cuda:2"), "counts")))


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
P = C.c_void_p(0x1000)
NUL = None
BIG = 1 << 40


def lib():
    lib = B.load_library()
    assert hasattr(lib, "fslic_hip_region_sums")
    return lib


def test_exports_and_workspace_size():
    names = ["fslic_hip_region_sums_workspace_size", "fslic_hip_region_sums", "fslic_hip_region_edge_weights"]
    assert sorted(n for n in B.EXPORTS if "_region_" in n) == sorted(names) and all(hasattr(lib(), n) for n in names)
    n = C.c_size_t()
    f = lib().fslic_hip_region_sums_workspace_size
    assert f(8, 3, 1600, C.byref(n)) == 0 and n.value == 56 * 8 * 3 * 1600                 # seven 64-bit words per (frame, channel, group)
    assert f(1, 1, 1, C.byref(n)) == 0 and n.value == 56
    assert f(3, 2, 65534, C.byref(n)) == 0 and n.value == 56 * 3 * 2 * 65534
    for N, Cc, K2 in ((0, 3, 4), (-1, 3, 4), (1, 0, 4), (1, -1, 4), (1, 3, 0), (1, 3, 65535), (1 << 16, 1, 1 << 15), (1 << 8, 1 << 8, 1 << 15)):
        assert f(N, Cc, K2, C.byref(n)) == B.FSLIC_E_INVALID, (N, Cc, K2)
    assert f(1, 3, 4, None) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", [dict(device=-1), dict(N=0), dict(Cc=0), dict(Cc=-3), dict(K=0), dict(K=65535), dict(K2=0), dict(K2=65535),
                                dict(N=1 << 16, K=1 << 15), dict(N=1 << 8, Cc=1 << 8, K=1 << 15), dict(N=1 << 8, Cc=1 << 8, K2=1 << 15),
                                dict(values=NUL), dict(mapping=NUL), dict(ctype=0), dict(ctype=3), dict(counts=NUL), dict(counts_out=NUL),
                                dict(sums=NUL), dict(ws=NUL), dict(nbytes=0), dict(nbytes=56 * 2 * 3 * 4 - 1)])
def test_capi_sums_refuses(kw):
    a = dict(device=0, N=2, Cc=3, K=5, K2=4, values=P, mapping=P, counts=P, ctype=1, sums=P, counts_out=P, ws=P, nbytes=BIG)
    a.update(kw)
    assert lib().fslic_hip_region_sums(a["device"], NUL, a["N"], a["Cc"], a["K"], a["K2"], a["values"], a["mapping"], a["counts"], a["ctype"],
                                       a["sums"], a["counts_out"], a["ws"], a["nbytes"]) == B.FSLIC_E_INVALID
    if kw.get("nbytes"):
        assert b"workspace too small: 1344 bytes" in lib().fslic_hip_last_error()


@pytest.mark.parametrize("kw", [dict(device=-1), dict(N=0), dict(Cc=0), dict(K=0), dict(K=65535), dict(N=1 << 16, K=1 << 15), dict(E=-1), dict(E=1 << 31),
                                dict(ei=NUL), dict(off=NUL), dict(sums=NUL), dict(counts=NUL), dict(ctype=0), dict(ctype=3), dict(mode=2), dict(mode=-1),
                                dict(weight=NUL)])
def test_capi_edge_weights_refuses(kw):
    a = dict(device=0, N=2, Cc=3, K=5, E=7, ei=P, off=P, sums=P, counts=P, ctype=2, mode=1, weight=P)
    a.update(kw)
    assert lib().fslic_hip_region_edge_weights(a["device"], NUL, a["N"], a["Cc"], a["K"], a["E"], a["ei"], a["off"], a["sums"], a["counts"],
                                               a["ctype"], a["mode"], a["weight"]) == B.FSLIC_E_INVALID
