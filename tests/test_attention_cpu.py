"""CPU tests of attention over neighbour lists (fast_slic_amd/attention.py, the fslic_hip_attend_* entries): the float32 model
(tests/attention_ref.py) by hand on a path of three nodes, against its float64 restatement (dense masked attention) within the bounds
its docstring derives, its backward formulas against torch's float64 autograd of that restatement, and every argument error refused
before any device work -- ValueError in Python, FSLIC_E_INVALID from the C ABI before its first HIP call, with the words and the order
of csrc/attendapi.cpp.  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import aggregate_ref as A
import attention_ref as M
from fast_slic_amd import _binding as B
from fast_slic_amd import attention, propagate
from fast_slic_amd.attention import graph_attention, head_aggregate, neighbour_dot, neighbour_softmax
from fast_slic_amd.propagate import neighbour_lists
from test_aggregate_cpu import make_graph, numpy_lists, path, random_pairs, star
from test_stream_refusals_cpu import DEVICE, NUL, NULL_ARG, P, rows_of

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ---- the model, by hand ----
def test_model_by_hand_on_a_path_of_three():
    # 0 - 1 - 2: row 0 <- {1}, row 1 <- {0, 2}, row 2 <- {1}
    offsets, indices = numpy_lists(neighbour_lists(make_graph([path(3)], 3)))
    assert offsets.tolist() == [0, 1, 3, 4] and indices.tolist() == [1, 0, 2, 1]
    ent = M.Entries(offsets, indices, 1, 3)
    a, b = np.array([[[1, 2, 3], [0, 1, 0]]], F32), np.array([[[1, 1, 2], [4, 0, 4]]], F32)
    assert M.dot(a, b, ent, 1).tolist() == [[1 * 1 + 0 * 0, 2 * 1 + 1 * 4, 2 * 2 + 1 * 4, 3 * 1 + 0 * 0]]
    assert M.dot(a, b, ent, 2).tolist() == [[1, 2, 4, 3], [0, 4, 4, 0]]
    # a single entry is 1 exactly, a tie is a half each, and the fold is e / (e + 1) with e = expf(6 - 8)
    al = M.softmax(np.array([[1, 6, 8, 3], [0, 4, 4, 0]], F32), ent)
    e = M.expf(np.array([-2], F32))[0]
    assert e == F32(np.exp(-2.0)) and M.expf(np.array([0, -np.inf], F32)).tolist() == [1, 0]
    assert al.tolist() == [[1, e / (e + F32(1)), F32(1) / (e + F32(1)), 1], [1, 0.5, 0.5, 1]]
    # alpha (g - t): t = 0.5 * 1 + 0.5 * 3 = 2 in the middle row; a single entry gives 1 * (g - g) = +0.0
    gs = M.softmax_backward(np.array([[1, 0.5, 0.5, 1]], F32), np.array([[5, 1, 3, -7]], F32), ent)
    assert gs.tolist() == [[0, -0.5, 0.5, 0]] and not np.signbit(gs[0, [0, 3]]).any()
    # rule A with two heads: channel 0 takes the weights of head 0, channel 1 those of head 1
    x = np.array([[[1, 2, 4], [-8, 3, 3]]], F32)
    w = np.array([[0.5, 2, 3, 10], [1, -1, 0.25, 2]], F32)
    assert M.apply(x, w, ent).tolist() == [[[0.5 * 2, 2 * 1 + 3 * 4, 10 * 2], [1 * 3, -1 * -8 + 0.25 * 3, 2 * 3]]]
    g = np.array([[[1, 10, 100], [2, 20, 200]]], F32)
    assert M.apply_transposed(g, w, ent).tolist() == [[[2 * 10, 0.5 * 1 + 10 * 100, 3 * 10], [-1 * 20, 1 * 2 + 2 * 200, 0.25 * 20]]]
    # an invalid entry and the entries behind the last row: +0.0 everywhere, and nothing counts into Z
    ent = M.Entries(np.array([0, 2, 3, 3]), np.array([1, -1, 3, 0, 1], np.int32), 1, 3)
    assert ent.valid.tolist() == [True, False, False, False, False] and ent.valid_degree.tolist() == [1, 0, 0]
    assert M.dot(a, b, ent, 1).tolist() == [[1, 0, 0, 0, 0]] and M.softmax(np.array([[3, 9, 9, 9, 9]], F32), ent).tolist() == [[1, 0, 0, 0, 0]]
    assert M.apply(x, np.full((1, 5), 2, F32), ent).tolist() == [[[4, 0, 0], [6, 0, 0]]]


def case(seed, N, K, Hd, D, degree):
    rng = np.random.default_rng(seed)
    frames = []
    for pairs in [random_pairs(rng, K, degree) for _ in range(N - 1)] + [path(K) + star(K, min(10, K - 1))]:
        count, kept = np.zeros(K, int), set()
        for a, b in pairs:                                                 # no node with more than 12 neighbours
            if count[a] < 12 and count[b] < 12 and (min(a, b), max(a, b)) not in kept:
                kept.add((min(a, b), max(a, b)))
                count[a], count[b] = count[a] + 1, count[b] + 1
        frames.append(sorted(kept))
    offsets, indices = numpy_lists(neighbour_lists(make_graph(frames, K)))
    ent = M.Entries(offsets, indices, N, K)
    assert ent.valid_degree.max() <= 12
    return rng, ent, offsets, indices


CASES = [(0, 1, 9, 1, 1, 3), (1, 2, 40, 2, 5, 6), (2, 3, 64, 3, 16, 8), (3, 1, 130, 4, 8, 4)]


def test_one_head_is_graph_aggregate():
    """With Hd = 1 the model is aggregate_ref's, forward and both gradients: the same folds."""
    rng, ent, offsets, indices = case(5, 2, 40, 1, 6, 6)
    x, g = rng.standard_normal((2, 6, 40)).astype(F32), rng.standard_normal((2, 6, 40)).astype(F32)
    w = rng.standard_normal(ent.nnz).astype(F32)
    assert np.array_equal(M.apply(x, w[None], ent), A.forward(x, offsets, indices, w)[0])
    assert np.array_equal(M.apply_transposed(g, w[None], ent), A.backward_values(g, offsets, indices, w))
    assert np.array_equal(M.dot(g, x, ent, 1)[0], A.backward_weight(x, g, offsets, indices))


@pytest.mark.parametrize("seed,N,K,Hd,D,degree", CASES)
def test_float32_model_against_float64(seed, N, K, Hd, D, degree):
    """Every step and the composition within the bounds of attention_ref's docstring; |s| <= 8, D <= 16, degree <= 12."""
    rng, ent, offsets, indices = case(seed, N, K, Hd, D, degree)
    Cc = Hd * D
    a, b, x = (rng.standard_normal((N, Cc, K)).astype(F32) for _ in range(3))
    s = rng.uniform(-8, 8, (Hd, ent.nnz)).astype(F32)
    # dot: D terms
    got, want = M.dot(a, b, ent, Hd), M.dot64(t64(a), t64(b), ent, Hd).numpy()
    assert (np.abs(got - want) <= A.gamma(D) * M.dot64(t64(np.abs(a)), t64(np.abs(b)), ent, Hd).numpy()).all() and np.abs(want).max() > 0
    # softmax, from the same scores
    al, al64 = M.softmax(s, ent), M.softmax64(t64(s), ent).numpy()
    rel = M.alpha_bound(s, ent)
    assert (np.abs(al - al64) <= rel * al64).all() and rel.max() < 2e-5
    assert np.allclose(M.row_sum(al64, ent)[:, ent.valid_degree > 0], 1.0, atol=1e-12)
    # rule A: d terms
    want, terms = M.apply64(t64(x), t64(al), ent).numpy(), M.apply64(t64(np.abs(x)), t64(al), ent).numpy()
    assert (np.abs(M.apply(x, al, ent) - want) <= A.gamma(ent.valid_degree.reshape(N, 1, K)) * terms).all()
    # the composition, with a scale that rounds
    for scale in (None, 0.3):
        y, alpha = M.attention(a, b, x, ent, Hd, scale)
        y64, alpha64, bound = M.attention_bound(a, b, x, ent, Hd, scale)
        assert (np.abs(y - y64) <= bound).all() and bound.max() < 1e-3 * max(np.abs(y64).max(), 1e-3)
        assert alpha.shape == alpha64.shape == (Hd, ent.nnz)


@pytest.mark.parametrize("seed,N,K,Hd,D,degree", CASES)
def test_backward_formulas_against_float64_autograd(seed, N, K, Hd, D, degree):
    """grad_s = alpha (g - sum alpha g), and the dot and the sum as each other's gradients, against torch's autograd of the dense
    float64 restatement: each within the bound of its fold (attention_ref's docstring)."""
    rng, ent, offsets, indices = case(seed + 10, N, K, Hd, D, degree)
    Cc = Hd * D
    a, b, g = (rng.standard_normal((N, Cc, K)).astype(F32) for _ in range(3))
    s, gs = rng.uniform(-8, 8, (Hd, ent.nnz)).astype(F32), rng.standard_normal((Hd, ent.nnz)).astype(F32)
    w = rng.standard_normal((Hd, ent.nnz)).astype(F32)
    row_terms = ent.valid_degree.reshape(N, 1, K)
    col_terms = np.bincount((ent.f * K + ent.jj)[ent.valid], minlength=N * K).reshape(N, 1, K)

    def grads(fn, inputs, grad_out):
        leaves = [t64(v).requires_grad_() for v in inputs]
        fn(*leaves).backward(t64(grad_out))
        return [leaf.grad.numpy() for leaf in leaves]

    # softmax
    want, = grads(lambda t: M.softmax64(t, ent), [s], gs)
    al, al64 = M.softmax(s, ent), M.softmax64(t64(s), ent).numpy()
    bound = M.softmax_backward_bound(al64, gs.astype(np.float64), M.alpha_bound(s, ent), ent)
    assert (np.abs(M.softmax_backward(al, gs, ent) - want) <= bound).all() and np.abs(want).max() > 0
    # the dot's gradients are rule A and its transposed form
    dot64 = lambda u, v: M.dot64(u, v, ent, Hd)
    (ga, gb), (ta, tb) = grads(dot64, [a, b], gs), grads(dot64, [np.abs(a), np.abs(b)], np.abs(gs))
    assert (np.abs(M.apply(b, gs, ent) - ga) <= A.gamma(row_terms) * ta).all() and np.abs(ga).max() > 0
    assert (np.abs(M.apply_transposed(a, gs, ent) - gb) <= A.gamma(col_terms) * tb).all() and np.abs(gb).max() > 0
    # the sum's gradients are its transposed form and the dot
    apply64 = lambda u, v: M.apply64(u, v, ent)
    (gx, gw), (tx, tw) = grads(apply64, [a, w], g), grads(apply64, [np.abs(a), np.abs(w)], np.abs(g))
    assert (np.abs(M.apply_transposed(g, w, ent) - gx) <= A.gamma(col_terms) * tx).all()
    assert (np.abs(M.dot(g, a, ent, Hd) - gw) <= A.gamma(D) * tw).all() and np.abs(gw).max() > 0
    # and the composition chains the three steps in the right order, the scale included: a check of the model's wiring, two decimal
    # orders above the steps' bounds (which the assertions above carry); the kernels are held to the model bit for bit on the GPU
    y, alpha, (gq, gk, gv) = M.attention(a, b, g, ent, Hd, None, gy=a)
    wq, wk, wv = grads(lambda q, k, v: M.attention64(q, k, v, ent, Hd)[0], [a, b, g], a)
    for got, want in ((gq, wq), (gk, wk), (gv, wv)):
        assert np.abs(got - want).max() <= 1e-4 * max(np.abs(want).max(), 1.0)


# ---- argument errors: all before any device work (a CPU tensor is the last thing refused) ----
G = make_graph([path(5), star(5, 3)], 5)                                   # N = 2, K = 5, E = 7, nnz = 14
NL = neighbour_lists(G)
PAIR = (NL.offsets, NL.indices)
X = torch.zeros((2, 4, 5))
S = torch.zeros((2, 14))


def refused(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def test_bad_maps_heads_and_entries():
    for lists in (G, NL, PAIR):
        refused("a must be float32", neighbour_dot, X.double(), X, lists)
        refused(r"a must be \[C, K\] or \[N, C, K\]", neighbour_dot, torch.zeros(5), X, lists)
        refused("a must be a torch tensor", neighbour_dot, None, X, lists)
        refused(r"b must be the shape of a, \(2, 4, 5\)", neighbour_dot, X, torch.zeros((2, 3, 5)), lists)
        refused("b must be float32", neighbour_dot, X, X.half(), lists)
        refused(r"the values have 3 of 5|graph offsets must be \[N \* K \+ 1\] = \[16\]", neighbour_dot, torch.zeros((3, 4, 5)), torch.zeros((3, 4, 5)), lists)
        refused("K, the last dimension of a, must be in", neighbour_dot, torch.zeros((1, 1, 65535)), torch.zeros((1, 1, 65535)), lists)
        for heads in (0, -1, True, 2.0, None, "2"):
            refused("heads must be a positive integer", neighbour_dot, X, X, lists, heads)
        refused("C = 4 is not a multiple of heads = 3", neighbour_dot, X, X, lists, 3)
        refused(r"weight must be \[Hd, nnz\] or \[nnz\] with nnz = 14", head_aggregate, X, lists, torch.zeros((2, 13)))
        refused(r"weight must be \[Hd, nnz\]", head_aggregate, X, lists, torch.zeros((0, 14)))
        refused(r"weight must be \[Hd, nnz\]", head_aggregate, X, lists, torch.zeros((1, 2, 14)))
        refused("weight must be float32", head_aggregate, X, lists, S.double())
        refused("weight must be a torch tensor", head_aggregate, X, lists, None)
        refused("C = 4 is not a multiple of heads = 3", head_aggregate, X, lists, torch.zeros((3, 14)))
        refused("values must be float32", head_aggregate, X.int(), lists, S)
        refused(r"the values have 1 of 5|graph offsets must be \[N \* K \+ 1\] = \[6\]", head_aggregate, X[0], lists, S)
    refused(r"scores must be \[Hd, nnz\] or \[nnz\] with nnz = 14", neighbour_softmax, torch.zeros(13), NL)
    refused("scores must be float32", neighbour_softmax, S.double(), G)
    refused("num_frames must be an integer", neighbour_softmax, S, PAIR)
    refused("num_components must be an integer", neighbour_softmax, S, PAIR, num_frames=2)
    refused(r"graph offsets must be \[N \* K \+ 1\] = \[13\]", neighbour_softmax, S, PAIR, num_frames=2, num_components=6)
    refused("the graph has 2 frames of 5 nodes, not 2 of 6", neighbour_softmax, S, NL, num_frames=2, num_components=6)
    refused("a pair", neighbour_softmax, S, None, num_frames=2, num_components=5)
    refused("a pair", neighbour_dot, X, X, None)
    refused("graph indices must be int32", head_aggregate, X, (NL.offsets, NL.indices.long()), S)


def test_bad_attention_arguments():
    V = torch.zeros((2, 6, 5))
    for lists in (G, NL, PAIR):
        refused("query must be float32", graph_attention, X.double(), X, V, lists)
        refused("key must be the shape of query", graph_attention, X, V, V, lists)
        refused("values must have the frames and nodes of query", graph_attention, X, X, torch.zeros((2, 6, 4)), lists)
        refused("values must have the frames and nodes of query", graph_attention, X, X, torch.zeros((1, 6, 5)), lists)
        refused("C = 4 is not a multiple of heads = 3", graph_attention, X, X, V, lists, 3)
        refused("Cv = 6 is not a multiple of heads = 4", graph_attention, X, X, V, lists, 4)
        for scale in (float("inf"), float("nan"), "1", True, 1j):
            refused("scale must be None or a finite number", graph_attention, X, X, V, lists, 2, scale)
        refused("query must be on a ROCm GPU, got device cpu .there is no CPU fallback.", graph_attention, X, X, V, lists, 2, 0.5, True)


def test_2_to_the_31_limits():
    """Tensors of the sizes in question without their memory: one element expanded."""
    text = r"N \* C \* K, the number of neighbour entries and heads \* entries must be below 2\^31"
    K = 1 << 15
    offsets = torch.zeros(1, dtype=torch.int64).expand(K + 1)
    big = torch.zeros((1, 1, 1)).expand(1, 1 << 16, K)
    few = torch.zeros(4, dtype=torch.int32)
    refused(text, neighbour_dot, big, big, (offsets, few))
    refused(text, head_aggregate, big, (offsets, few), torch.zeros(4))
    refused(text, graph_attention, X, X, torch.zeros((1, 1, 1)).expand(2, 1 << 28, 5), PAIR, 2)
    small = torch.zeros(11, dtype=torch.int64)
    for nnz, heads, ok in ((1 << 31, 1, False), (1 << 29, 4, False), ((1 << 29) - 1, 4, True), ((1 << 31) - 1, 1, True)):
        lists = (small, torch.zeros(1, dtype=torch.int32).expand(nnz))
        scores = torch.zeros((1, 1)).expand(heads, nnz)
        match = "no CPU fallback" if ok else text                          # just below: the next refusal is the device's
        refused(match, neighbour_dot, X, X, lists, heads)
        refused(match, neighbour_softmax, scores, lists, num_frames=2, num_components=5)
        refused(match, head_aggregate, X, lists, scores)
        refused(match, graph_attention, X, X, X, lists, heads)
    refused("no CPU fallback", neighbour_dot, big[:, :-1], big[:, :-1], (offsets, few))


def test_cpu_tensors_are_refused_after_every_other_check():
    for lists in (G, NL, PAIR):
        refused("a must be on a ROCm GPU, got device cpu .there is no CPU fallback.", neighbour_dot, X, X, lists, 2)
        refused("values must be on a ROCm GPU, got device cpu", head_aggregate, X, lists, S)
        refused("values must be on a ROCm GPU", head_aggregate, X[0], neighbour_lists(make_graph([path(5)], 5)), torch.zeros(8))      # [C, K], [nnz]
        refused("query must be on a ROCm GPU", graph_attention, X, X, X, lists, 4)
    refused("scores must be on a ROCm GPU", neighbour_softmax, S, G)
    refused("scores must be on a ROCm GPU", neighbour_softmax, S[0], NL)
    refused("scores must be on a ROCm GPU", neighbour_softmax, S, PAIR, num_frames=2, num_components=5)


def test_the_tensors_are_handed_to_one_device_in_this_order(monkeypatch):
    """No GPU here, let alone two: _tensors.one_device refuses two GPUs first and a CPU tensor last (tests/test_aggregate_cpu.py)."""
    seen = []

    def one_device(tensors):
        seen.append([name for _, name in tensors])
        raise ValueError("stop")

    monkeypatch.setattr(attention.T, "one_device", one_device)
    refused("stop", neighbour_dot, X, X, NL)
    refused("stop", neighbour_softmax, S, G)
    refused("stop", head_aggregate, X, PAIR, S)
    refused("stop", graph_attention, X, X, X, NL)
    assert seen == [["a", "b", "nl.offsets", "nl.indices"], ["scores", "graph.edge_index", "graph.offsets"],
                    ["values", "weight", "graph offsets", "graph indices"], ["query", "key", "values", "nl.offsets", "nl.indices"]]


def test_neighbour_lists_is_unchanged():
    assert attention.neighbour_lists is propagate.neighbour_lists and attention.NeighbourLists is propagate.NeighbourLists
    nl = neighbour_lists(make_graph([[(0, 1), (0, 2), (1, 2)], [(1, 3)]], 4))
    assert nl.offsets.tolist() == [0, 2, 4, 6, 6, 6, 7, 7, 8] and nl.indices.tolist() == [1, 2, 0, 2, 0, 1, 3, 1]
    assert nl.edge.tolist() == [0, 1, 0, 2, 1, 2, 3, 3] and nl.rows.tolist() == [0, 0, 1, 1, 2, 2, 5, 7]
    assert "attention" in propagate.__doc__ and propagate.__all__ == ["neighbour_lists", "graph_aggregate", "NeighbourLists"]


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
NAMES = ["fslic_hip_attend_dot", "fslic_hip_attend_softmax", "fslic_hip_attend_softmax_backward", "fslic_hip_attend_apply"]


def lib():
    return B.load_library()


def test_exports():
    header = open(os.path.join(ROOT, "include", "fslic_hip.h")).read()
    assert [n for n in B.EXPORTS if "_attend_" in n] == NAMES and all(hasattr(lib(), n) and "int %s(" % n in header for n in NAMES)
    assert B.EXPORTS.index(NAMES[-1]) < B.EXPORTS.index("fslic_hip_pool_workspace_size")      # in front of the pinned tail of the table
    assert not any(part in n for n in NAMES for part in ("_aggregate_", "_merge_", "_region_", "_connect", "fslic_hip_soft_"))


# streamapi.h's checks of a [N][C][K] call (N = 0 leaves no way to N * C * K >= 2^31), then check_heads: the three head checks need
# three values of `heads`, so the later ones are violated with a value that passes the earlier
HEADS = [("attend:1", dict(heads=0), b"heads must be positive"), ("attend:2", dict(heads=2), b"C must be a multiple of heads"),
         ("attend:3", dict(heads=3, nnz=1 << 30), b"heads * nnz must be below 2^31")]
CELLS = [("stream", dict(device=-1), b"device must be >= 0"), ("stream", dict(N=0), b"N must be positive"), ("stream", dict(C=0), b"C must be positive"),
         ("stream", dict(K=65535), b"K must be in [1, 65534]"), ("stream", dict(N=1 << 16, K=1 << 15), b"N * C * K must be below 2^31"),
         ("stream", dict(nnz=-1), b"nnz must be in [0, 2^31)")] + HEADS
# the softmax has no channels: "C must be a multiple of heads" cannot be reached
ROWS = [("stream", dict(device=-1), b"device must be >= 0"), ("attend:4", dict(N=0), b"N must be positive"), ("stream", dict(K=65535), b"K must be in [1, 65534]"),
        ("attend:5", dict(N=1 << 16, K=1 << 15), b"N * K must be below 2^31"), ("stream", dict(nnz=-1), b"nnz must be in [0, 2^31)"), HEADS[0], HEADS[2]]
CALL = dict(device=DEVICE, stream=NUL, N=2, C=3, K=5, nnz=14, heads=1)
ROWS_CALL = dict(device=DEVICE, stream=NUL, N=2, K=5, nnz=14, heads=1)

# (entry, valid arguments, checks in source order, argument sets answered with FSLIC_OK before any HIP call, the pointers refused alone)
TABLE = [
    ("fslic_hip_attend_dot", dict(CALL, rows=P, indices=P, a=P, b=P, out=P),
     CELLS + [("attend:6", dict(a=NUL, b=NUL, rows=NUL, indices=NUL, out=NUL), NULL_ARG)],
     [dict(nnz=0), dict(nnz=0, rows=NUL, indices=NUL, out=NUL)], ["rows", "indices", "a", "b", "out"]),
    ("fslic_hip_attend_softmax", dict(ROWS_CALL, offsets=P, indices=P, scores=P, out=P),
     ROWS + [("attend:7", dict(offsets=NUL, indices=NUL, scores=NUL, out=NUL), NULL_ARG)],
     [dict(nnz=0), dict(nnz=0, indices=NUL, scores=NUL, out=NUL)], ["offsets", "indices", "scores", "out"]),
    ("fslic_hip_attend_softmax_backward", dict(ROWS_CALL, offsets=P, indices=P, alpha=P, grad_out=P, grad_scores=P),
     ROWS + [("attend:8", dict(offsets=NUL, indices=NUL, alpha=NUL, grad_out=NUL, grad_scores=NUL), NULL_ARG)],
     [dict(nnz=0), dict(nnz=0, indices=NUL, alpha=NUL, grad_out=NUL, grad_scores=NUL)], ["offsets", "indices", "alpha", "grad_out", "grad_scores"]),
    # (without entries the sum is still a launch, of zeros: no row of FSLIC_OK)
    ("fslic_hip_attend_apply", dict(CALL, transposed=1, offsets=P, ia=P, ib=P, weight=P, src=P, dst=P),
     CELLS + [("attend:9", dict(transposed=2), b"transposed must be 0 or 1"),
              ("attend:10", dict(offsets=NUL, ia=NUL, ib=NUL, weight=NUL, src=NUL, dst=NUL), NULL_ARG)],
     [], ["offsets", "ia", "ib", "weight", "src", "dst"]),
]
REFUSALS = [pytest.param(name, args, text, id="%s-%d-%s" % (name[len("fslic_hip_"):], i, site))
            for name, valid, checks, _, _ in TABLE for i, (site, args, text) in enumerate(rows_of(valid, checks))]
ALONE = [pytest.param(name, dict(valid, **{p: NUL}), id="%s-%s" % (name[len("fslic_hip_"):], p)) for name, valid, _, _, ps in TABLE for p in ps]
NOTHING_TO_DO = [pytest.param(name, dict(valid, **kw), id="%s-%d" % (name[len("fslic_hip_"):], i)) for name, valid, _, oks, _ in TABLE for i, kw in enumerate(oks)]


def test_the_table_holds_every_entry_and_reaches_every_site():
    assert [name for name, _, _, _, _ in TABLE] == NAMES
    for name, valid, _, _, _ in TABLE:
        assert len(valid) == len(dict((n, a) for n, _, a in B.SIGNATURES)[name]), name
    source = open(os.path.join(ROOT, "fast_slic_amd", "csrc", "attendapi.cpp")).read()
    sites = source.count("fail(FSLIC_E_INVALID")
    reached = {site for _, _, checks, _, _ in TABLE for site, _, _ in checks if site != "stream"}
    assert sites == 10 and reached == {"attend:%d" % (i + 1) for i in range(sites)}


@pytest.mark.parametrize("name,args,text", REFUSALS)
def test_refused_with_these_words(name, args, text):
    assert (getattr(lib(), name)(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, text)


@pytest.mark.parametrize("name,args", ALONE)
def test_every_pointer_is_refused_alone(name, args):
    assert (getattr(lib(), name)(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, NULL_ARG)


@pytest.mark.parametrize("name,args", NOTHING_TO_DO)
def test_nothing_to_do_is_ok_before_any_hip_call(name, args):
    assert getattr(lib(), name)(*args.values()) == B.FSLIC_OK

