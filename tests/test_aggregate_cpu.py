"""CPU tests of propagation along the graph (fast_slic_amd/propagate.py, the fslic_hip_aggregate* entries): neighbour_lists on CPU
tensors against SuperpixelGraph.to_batch_csr and crf_torch.transpose_batch_csr; the float32 model (tests/aggregate_ref.py) by hand and
against its float64 restatement within the standard bound of a fold; and every argument error refused before any device work --
ValueError in Python, FSLIC_E_INVALID from the C ABI before its first HIP call.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest
import torch

import aggregate_ref as A
from fast_slic_amd import _binding as B
from fast_slic_amd.crf_torch import transpose_batch_csr
from fast_slic_amd.propagate import NeighbourLists, graph_aggregate, neighbour_lists
from fast_slic_amd.rag import SuperpixelGraph

F32 = np.float32


# ---- graphs: per frame a collection of node pairs -> a SuperpixelGraph as superpixel_graph gives it (the GPU tests use these too) ----
def make_graph(frames, K, device="cpu", seed=0):
    frames = [sorted({(min(a, b), max(a, b)) for a, b in fr if a != b}) for fr in frames]
    edges = np.array([e for fr in frames for e in fr], np.int64).reshape(-1, 2).T
    offsets = np.cumsum([0] + [len(fr) for fr in frames]).astype(np.int64)
    boundary = np.random.default_rng(seed).integers(1, 50, edges.shape[1]).astype(np.int32)
    return SuperpixelGraph(torch.from_numpy(np.ascontiguousarray(edges)).to(device), torch.from_numpy(boundary).to(device), None,
                           torch.from_numpy(offsets).to(device), K, 1024)


def path(K):
    return [(i, i + 1) for i in range(K - 1)]


def star(K, degree, hub=None):
    """A hub (the middle node unless given) joined to the `degree` nodes next in number, wrapping round."""
    hub = K // 2 if hub is None else hub
    assert degree < K
    return [(hub, (hub + 1 + i) % K) for i in range(degree)]


def random_pairs(rng, K, mean_degree, isolated=()):
    n = int(K * mean_degree / 2)
    pairs = rng.integers(0, K, (n, 2))
    return [(int(a), int(b)) for a, b in pairs if a != b and a not in isolated and b not in isolated]


def numpy_lists(nl):
    return nl.offsets.cpu().numpy(), nl.indices.cpu().numpy()


# ---- neighbour_lists ----
def check_lists(g):
    nl = neighbour_lists(g)
    N, K, E = g.num_frames, g.num_components, g.edge_index.shape[1]
    offsets, indices = g.to_batch_csr()
    assert isinstance(nl, NeighbourLists) and (nl.num_frames, nl.num_components) == (N, K)
    assert nl.offsets.dtype == torch.int64 and nl.indices.dtype == torch.int32 and nl.edge.dtype == torch.int64 and nl.rows.dtype == torch.int32
    assert torch.equal(nl.offsets, offsets) and torch.equal(nl.indices, indices) and tuple(nl.indices.shape) == (2 * E,)
    # every entry names its undirected edge, and every edge is named by exactly two entries: (a <- b) and (b <- a)
    frame = np.searchsorted(g.offsets.numpy()[1:], np.arange(E), side="right")
    a, b = g.edge_index.numpy()
    rows, idx, edge = nl.rows.numpy().astype(np.int64), nl.indices.numpy().astype(np.int64), nl.edge.numpy()
    assert np.array_equal(np.bincount(edge, minlength=E), np.full(E, 2))
    lo, hi = np.minimum(rows % K, idx), np.maximum(rows % K, idx)
    assert np.array_equal(lo, a[edge]) and np.array_equal(hi, b[edge]) and np.array_equal(rows // K, frame[edge])
    assert np.array_equal(rows, A.rows_of(offsets.numpy(), 2 * E))
    deg = nl.degree()
    assert deg.dtype == torch.int32 and tuple(deg.shape) == (N, K)
    assert np.array_equal(deg.numpy().ravel(), np.bincount(rows, minlength=N * K))
    want = transpose_batch_csr(offsets, indices, N, K)
    got = nl.transposed()
    assert all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(got, want)) and nl.transposed() is got      # computed once and kept
    t = torch.arange(E, dtype=torch.float32) * 0.5
    assert torch.equal(nl.entry_values(t), t[nl.edge]) and tuple(nl.entry_values(torch.zeros((E, 3))).shape) == (2 * E, 3)
    assert torch.equal(nl.entry_values(g.boundary), g.boundary[nl.edge])
    return nl


def test_lists_of_graphs():
    rng = np.random.default_rng(1)
    check_lists(make_graph([path(5)], 5))
    check_lists(make_graph([star(40, 30), path(40), random_pairs(rng, 40, 5)], 40))
    check_lists(make_graph([random_pairs(rng, 17, 3, isolated=(0, 5, 16)), [], random_pairs(rng, 17, 8)], 17))      # a frame with no edge
    check_lists(make_graph([[], path(3)], 3))
    check_lists(make_graph([path(2)], 2))
    nl = check_lists(make_graph([[], []], 4))                                                                       # E = 0
    assert nl.offsets.tolist() == [0] * 9 and nl.indices.numel() == 0 and nl.degree().tolist() == [[0] * 4] * 2
    assert check_lists(make_graph([[]], 1)).offsets.tolist() == [0, 0]


def test_lists_by_hand():
    nl = neighbour_lists(make_graph([[(0, 1), (0, 2), (1, 2)], [(1, 3)]], 4))
    assert nl.offsets.tolist() == [0, 2, 4, 6, 6, 6, 7, 7, 8] and nl.indices.tolist() == [1, 2, 0, 2, 0, 1, 3, 1]
    assert nl.edge.tolist() == [0, 1, 0, 2, 1, 2, 3, 3] and nl.rows.tolist() == [0, 0, 1, 1, 2, 2, 5, 7]
    assert nl.degree().tolist() == [[2, 2, 2, 0], [0, 1, 0, 1]]


def test_lists_of_a_raw_pair():
    offsets, indices = torch.tensor([0, 2, 2, 5, 5, 6, 6]), torch.tensor([1, -1, 0, 3, 1, 2], dtype=torch.int32)
    nl = neighbour_lists((offsets, indices), num_frames=2, num_components=3)
    assert nl.edge is None and nl.rows.tolist() == [0, 0, 2, 2, 2, 4] and nl.rows.dtype == torch.int32
    assert nl.offsets is offsets and nl.indices is indices and nl.degree().tolist() == [[2, 0, 3], [0, 1, 0]]
    assert all(torch.equal(x, y) for x, y in zip(nl.transposed(), transpose_batch_csr(offsets, indices, 2, 3)))
    with pytest.raises(ValueError, match="a raw pair has no edges"):
        nl.entry_values(torch.zeros(3))
    for bad, match in (((offsets, indices.long()), "graph indices must be int32"), ((offsets.int(), indices), "graph offsets must be int64"),
                       ((offsets[:-1], indices), r"graph offsets must be \[N \* K \+ 1\]"), ((offsets, indices.view(2, 3)), r"graph indices must be \[nnz\]"),
                       ((offsets,), "a pair"), (None, "a pair")):
        with pytest.raises(ValueError, match=match):
            neighbour_lists(bad, num_frames=2, num_components=3)
    for kw in (dict(), dict(num_frames=2), dict(num_frames=0, num_components=3), dict(num_frames=2, num_components=True)):
        with pytest.raises(ValueError, match="num_frames|num_components"):
            neighbour_lists((offsets, indices), **kw)
    g = make_graph([path(3)], 3)
    with pytest.raises(ValueError, match="1 frames of 3 nodes"):
        neighbour_lists(g, num_components=4)
    with pytest.raises(ValueError, match="t must be a torch tensor"):
        neighbour_lists(g).entry_values(torch.zeros(3))


# ---- the model, by hand ----
def test_model_by_hand():
    # one frame of K = 3: row 0 <- {1, 2}, row 1 <- {0, -1 (invalid)}, row 2 empty
    offsets, indices = np.array([0, 2, 4, 4]), np.array([1, 2, 0, -1], np.int32)
    x = np.array([[[1, 2, 4], [-8, 3, 3]]], F32)
    w = np.array([0.5, 2, 3, 100], F32)
    y, arg, deg = A.forward(x, offsets, indices)
    assert y.tolist() == [[[6, 1, 0], [6, -8, 0]]] and arg is None and deg.tolist() == [2, 1, 0]
    assert A.forward(x, offsets, indices, w)[0].tolist() == [[[9, 3, 0], [7.5, -24, 0]]]
    assert A.forward(x, offsets, indices, reduce="mean")[0].tolist() == [[[3, 1, 0], [3, -8, 0]]]
    y, arg, _ = A.forward(x, offsets, indices, reduce="max")
    assert y.tolist() == [[[4, 1, 0], [3, -8, 0]]] and arg.tolist() == [[[1, 2, -1], [0, 2, -1]]]      # the tie 3 == 3 goes to the smaller entry
    assert not np.signbit(y[..., 2]).any()                                 # an empty row is +0.0
    g = np.array([[[1, 10, 100], [2, 20, 200]]], F32)
    assert A.backward_values(g, offsets, indices).tolist() == [[[10, 1, 1], [20, 2, 2]]]
    assert A.backward_values(g, offsets, indices, w).tolist() == [[[30, 0.5, 2], [60, 1, 4]]]
    assert A.backward_values(g, offsets, indices, reduce="mean", degree=deg).tolist() == [[[10, 0.5, 0.5], [20, 1, 1]]]
    assert A.backward_values(g, offsets, indices, reduce="max", argmax=arg).tolist() == [[[10, 0, 1], [20, 2, 0]]]
    assert A.backward_weight(x, g, offsets, indices).tolist() == [2 * 1 + 3 * 2, 4 * 1 + 3 * 2, 1 * 10 + -8 * 20, 0]
    # the fold is a left fold: 2^24 + 1 + 1 loses both ones, 1 + 1 + 2^24 keeps them
    big = np.array([[[0, 2.0 ** 24, 1, 1]]], F32)
    assert A.forward(big, np.array([0, 3, 3, 3, 3]), np.array([1, 2, 3], np.int32))[0][0, 0, 0] == 2.0 ** 24
    assert A.forward(big, np.array([0, 3, 3, 3, 3]), np.array([2, 3, 1], np.int32))[0][0, 0, 0] == 2.0 ** 24 + 2


@pytest.mark.parametrize("seed,N,K,C,degree", [(0, 1, 9, 1, 3), (1, 2, 40, 3, 6), (2, 3, 64, 5, 20), (3, 1, 301, 2, 4)])
def test_float32_model_against_float64(seed, N, K, C, degree):
    """|float32 fold - float64 value| <= gamma * sum |terms|, gamma = (d + 1) u / (1 - (d + 1) u) with d the terms of the fold: the
    standard bound of a product plus d - 1 additions (the float64 side's own error is 2^-29 of that and inside the bound's slack:
    gamma is stated for d + 1, not d, roundings)."""
    rng = np.random.default_rng(seed)
    frames = [random_pairs(rng, K, degree) + (star(K, 300) if K > 300 else []) for _ in range(N)]
    offsets, indices = numpy_lists(neighbour_lists(make_graph(frames, K)))
    x, g = rng.standard_normal((N, C, K)).astype(F32), rng.standard_normal((N, C, K)).astype(F32)
    w = rng.standard_normal(len(indices)).astype(F32)
    row_terms = np.diff(offsets).reshape(N, 1, K)
    col_terms = np.bincount(np.asarray(A.rows_of(offsets, len(indices)) // K * K + indices, np.int64), minlength=N * K).reshape(N, 1, K)
    for weight in (None, w):
        (y64, gx64, gw64), (ya, gxa, gwa) = A.sum64(x, g, offsets, indices, weight)
        y = A.forward(x, offsets, indices, weight)[0]
        assert (np.abs(y - y64) <= A.gamma(row_terms) * ya).all() and np.abs(y64).max() > 0
        gx = A.backward_values(g, offsets, indices, weight)
        assert (np.abs(gx - gx64) <= A.gamma(col_terms) * gxa).all()
        gw = A.backward_weight(x, g, offsets, indices)
        assert (np.abs(gw - gw64) <= A.gamma(C) * gwa).all()
    # mean and max against float64: the mean is the sum's fold and one more rounding, the max is exact
    d = np.maximum(row_terms, 1)
    y64 = A.sum64(x, g, offsets, indices)[0][0] / d
    ya = A.sum64(x, g, offsets, indices)[1][0] / d
    ym, _, deg = A.forward(x, offsets, indices, reduce="mean")
    assert (np.abs(ym - y64) <= A.gamma(row_terms + 1) * ya).all() and np.array_equal(deg, row_terms.ravel())
    yx, arg, _ = A.forward(x, offsets, indices, reduce="max")
    for r in range(N * K):
        f, i = divmod(r, K)
        nb = indices[offsets[r]:offsets[r + 1]]
        assert np.array_equal(yx[f, :, i], x[f][:, nb].max(1) if len(nb) else np.zeros(C, F32))


# ---- argument errors: all before any device work (a CPU tensor is the last thing refused) ----
G = make_graph([path(5), star(5, 3)], 5)                                   # N = 2, K = 5, E = 7, nnz = 14
X = torch.zeros((2, 3, 5))
W = torch.zeros(14)


@pytest.mark.parametrize("values,match", [
    (torch.zeros((2, 3, 5), dtype=torch.float64), "values must be float32"), (torch.zeros((2, 3, 5), dtype=torch.float16), "values must be float32"),
    (torch.zeros((2, 3, 5), dtype=torch.int32), "values must be float32"), (torch.zeros(5), r"values must be \[C, K\] or \[N, C, K\]"),
    (torch.zeros((1, 2, 3, 5)), r"values must be \[C, K\] or \[N, C, K\]"), (torch.zeros((2, 0, 5)), "values must not be empty"),
    (np.zeros((2, 3, 5), F32), "values must be a torch tensor"), (None, "values must be a torch tensor"),
    (torch.zeros((2, 3, 4)), "the graph has 2 frames of 5 nodes, the values have 2 of 4"), (torch.zeros((3, 3, 5)), "the values have 3 of 5"),
    (torch.zeros((3, 5)), "the values have 1 of 5"), (torch.zeros((1, 1, 65535)), "K, the last dimension of values, must be in"),
])
def test_bad_values(values, match):
    for lists in (G, neighbour_lists(G)):
        with pytest.raises(ValueError, match=match):
            graph_aggregate(values, lists)


@pytest.mark.parametrize("lists,match", [
    (None, "a pair"), ((G.offsets,), "a pair"), ({"offsets": 0}, "a pair"),
    ((torch.zeros(11, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)), "graph offsets must be int64"),
    ((torch.zeros(10, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)), r"graph offsets must be \[N \* K \+ 1\] = \[11\]"),
    ((torch.zeros(11, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)), "graph indices must be int32"),
    ((torch.zeros(11, dtype=torch.int64), torch.zeros((4, 1), dtype=torch.int32)), r"graph indices must be \[nnz\]"),
    ((np.zeros(11, np.int64), torch.zeros(4, dtype=torch.int32)), "graph offsets must be a torch tensor"),
    (SuperpixelGraph(G.edge_index.int(), G.boundary, None, G.offsets, 5, 1024), "edge_index must be int64"),
    (SuperpixelGraph(G.edge_index, G.boundary, None, G.offsets, 0, 1024), "num_components"),
])
def test_bad_lists(lists, match):
    with pytest.raises(ValueError, match=match):
        graph_aggregate(X, lists)


def test_bad_weight_and_reduce():
    nl = neighbour_lists(G)
    for weight, match in ((torch.zeros(13), r"weight must be \[nnz\] with nnz = 14"), (torch.zeros(7), r"weight must be \[nnz\]"),
                          (torch.zeros((14, 1)), r"weight must be \[nnz\]"), (torch.zeros(14, dtype=torch.float64), "weight must be float32"),
                          (np.zeros(14, F32), "weight must be a torch tensor"), (2.0, "weight must be a torch tensor")):
        for lists in (G, nl, (nl.offsets, nl.indices)):
            with pytest.raises(ValueError, match=match):
                graph_aggregate(X, lists, weight)
    for reduce in ("mean", "max"):
        with pytest.raises(ValueError, match="a weight goes with reduce='sum' only"):
            graph_aggregate(X, nl, W, reduce)
        with pytest.raises(ValueError, match="a weight goes with reduce='sum' only"):
            graph_aggregate(X, nl, weight=torch.zeros(3, dtype=torch.int8), reduce=reduce)      # refused whatever the weight is
    for reduce in ("Sum", "", "min", None, 0, b"sum", ["sum"]):
        with pytest.raises(ValueError, match="reduce must be 'sum', 'mean' or 'max'"):
            graph_aggregate(X, nl, reduce=reduce)
    for reduce in ("sum", "mean"):
        with pytest.raises(ValueError, match="return_argmax goes with reduce='max' only"):
            graph_aggregate(X, nl, reduce=reduce, return_argmax=True)


def test_2_to_the_31_limits():
    """Tensors of the sizes in question without their memory: one element expanded."""
    K = 1 << 15
    lists = (torch.zeros(1, dtype=torch.int64).expand(K + 1), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"N \* C \* K and the number of neighbour entries must be below 2\^31"):
        graph_aggregate(torch.zeros((1, 1, 1)).expand(1, 1 << 16, K), lists)
    lists = (torch.zeros(11, dtype=torch.int64), torch.zeros(1, dtype=torch.int32).expand(1 << 31))
    with pytest.raises(ValueError, match=r"N \* C \* K and the number of neighbour entries must be below 2\^31"):
        graph_aggregate(X, lists)
    with pytest.raises(ValueError, match="no CPU fallback"):                # just below both: the next refusal is the device's
        graph_aggregate(torch.zeros((1, 1, 1)).expand(1, (1 << 16) - 1, K), (torch.zeros(1, dtype=torch.int64).expand(K + 1), lists[1][:(1 << 31) - 1]))


def test_cpu_tensors_are_refused_after_every_other_check():
    nl = neighbour_lists(G)
    for lists in (G, nl, (nl.offsets, nl.indices)):
        for kw in (dict(), dict(weight=W), dict(reduce="mean"), dict(reduce="max", return_argmax=True)):
            with pytest.raises(ValueError, match="values must be on a ROCm GPU, got device cpu .there is no CPU fallback."):
                graph_aggregate(X, lists, **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):
        graph_aggregate(X[0], neighbour_lists(make_graph([path(5)], 5)))    # [C, K] with N = 1


def test_mismatched_devices_are_named_before_a_cpu_tensor():
    """No GPU here, let alone two: graph_aggregate hands its tensors to _tensors.one_device in this order."""
    from fast_slic_amd._tensors import one_device

    class On(object):
        def __init__(self, device):
            self.device = torch.device(device)

    with pytest.raises(ValueError, match=r"values, weight, nl.offsets, nl.indices must be on one GPU, got \['cuda:0', 'cuda:1'\]"):
        one_device([(On("cpu"), "values"), (On("cuda:0"), "weight"), (On("cuda:1"), "nl.offsets"), (On("cuda:1"), "nl.indices")])
    with pytest.raises(ValueError, match="values must be on a ROCm GPU"):
        one_device([(On("cpu"), "values"), (None, "weight"), (On("cuda:1"), "nl.offsets"), (On("cuda:1"), "nl.indices")])


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
P = C.c_void_p(0x1000)
NUL = None
SIZES = [dict(device=-1), dict(N=0), dict(N=-1), dict(Cc=0), dict(Cc=-3), dict(K=0), dict(K=65535), dict(N=1 << 16, K=1 << 15),
         dict(N=1 << 8, Cc=1 << 8, K=1 << 15), dict(nnz=-1), dict(nnz=1 << 31)]


def lib():
    lib = B.load_library()
    assert hasattr(lib, "fslic_hip_aggregate_forward")
    return lib


def test_exports():
    names = ["fslic_hip_aggregate_forward", "fslic_hip_aggregate_backward_values", "fslic_hip_aggregate_backward_weight"]
    assert sorted(n for n in B.EXPORTS if "_aggregate_" in n) == sorted(names) and all(hasattr(lib(), n) for n in names)


@pytest.mark.parametrize("kw", SIZES + [dict(reduce=3), dict(reduce=-1), dict(reduce=1), dict(reduce=2), dict(reduce=1, weight=NUL, argmax=NUL, degree=NUL),
                                dict(reduce=2, weight=NUL, argmax=NUL), dict(off=NUL), dict(idx=NUL), dict(values=NUL), dict(out=NUL)])
def test_capi_forward_refuses(kw):
    a = dict(device=0, N=2, Cc=3, K=5, nnz=14, reduce=0, off=P, idx=P, weight=P, values=P, out=P, argmax=P, degree=P)
    a.update(kw)
    assert lib().fslic_hip_aggregate_forward(a["device"], NUL, a["N"], a["Cc"], a["K"], a["nnz"], a["reduce"], a["off"], a["idx"], a["weight"],
                                             a["values"], a["out"], a["argmax"], a["degree"]) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", SIZES + [dict(reduce=3), dict(reduce=1), dict(reduce=1, weight=NUL, degree=NUL), dict(reduce=2, weight=NUL, argmax=NUL),
                                dict(off=NUL), dict(entries=NUL), dict(rows=NUL), dict(g=NUL), dict(dx=NUL)])
def test_capi_backward_values_refuses(kw):
    a = dict(device=0, N=2, Cc=3, K=5, nnz=14, reduce=0, off=P, entries=P, rows=P, weight=P, argmax=P, degree=P, g=P, dx=P)
    a.update(kw)
    assert lib().fslic_hip_aggregate_backward_values(a["device"], NUL, a["N"], a["Cc"], a["K"], a["nnz"], a["reduce"], a["off"], a["entries"], a["rows"],
                                                     a["weight"], a["argmax"], a["degree"], a["g"], a["dx"]) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", SIZES + [dict(rows=NUL), dict(idx=NUL), dict(values=NUL), dict(g=NUL), dict(dw=NUL)])
def test_capi_backward_weight_refuses(kw):
    a = dict(device=0, N=2, Cc=3, K=5, nnz=14, rows=P, idx=P, values=P, g=P, dw=P)
    a.update(kw)
    assert lib().fslic_hip_aggregate_backward_weight(a["device"], NUL, a["N"], a["Cc"], a["K"], a["nnz"], a["rows"], a["idx"], a["values"], a["g"],
                                                     a["dw"]) == B.FSLIC_E_INVALID


def test_capi_backward_weight_without_entries_launches_nothing():
    assert lib().fslic_hip_aggregate_backward_weight(0, NUL, 2, 3, 5, 0, NUL, NUL, P, P, NUL) == B.FSLIC_OK
