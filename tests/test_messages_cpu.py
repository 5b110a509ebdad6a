"""CPU tests of the messages over neighbour lists (fast_slic_amd/messages.py, the fslic_hip_message_* entries): the float32 model
(tests/messages_ref.py) by hand on a path of three nodes, the three identities that tie it to aggregate_ref and attention_ref bit for
bit, its forward and backward formulas against torch's float64 autograd of a dense restatement (index_select / index_add_ /
scatter_reduce), and every argument error refused before any device work -- ValueError in Python, FSLIC_E_INVALID from the C ABI
before its first HIP call, with the words and the order of csrc/messageapi.cpp.  No kernel is launched here."""
import os

import numpy as np
import pytest
import torch

import aggregate_ref as A
import attention_ref as M
import messages_ref as R
from fast_slic_amd import _binding as B
from fast_slic_amd import messages
from fast_slic_amd.messages import entry_gather, entry_reduce
from fast_slic_amd.propagate import neighbour_lists
from test_aggregate_cpu import make_graph, numpy_lists, path, random_pairs, star
from test_stream_refusals_cpu import DEVICE, NUL, NULL_ARG, P, rows_of

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def positive_zeros(a, where=None):
    z = np.asarray(a)[where] if where is not None else np.asarray(a)
    return not z.any() and not np.signbit(z).any()


# ---- the model, by hand ----
def test_model_by_hand_on_a_path_of_three():
    # 0 - 1 - 2: row 0 <- {1}, row 1 <- {0, 2}, row 2 <- {1}; transposed: node 0 <- entry 1, node 1 <- entries 0 and 3, node 2 <- entry 2
    offsets, indices = numpy_lists(neighbour_lists(make_graph([path(3)], 3)))
    assert offsets.tolist() == [0, 1, 3, 4] and indices.tolist() == [1, 0, 2, 1]
    ent = R.Entries(offsets, indices, 1, 3)
    x = np.array([[[1, 2, 4], [-8, 3, 5]]], F32)
    assert R.gather(x, ent, "target").tolist() == [[1, 2, 2, 4], [-8, 3, 3, 5]]
    assert R.gather(x, ent, "source").tolist() == [[2, 1, 4, 2], [3, -8, 5, 3]]
    # feature 1 ties in row 1 (entries 1 and 2), feature 2 ties in row 1 and at node 1 of the transposed lists (entries 0 and 3)
    m = np.array([[1, 6, 8, 3], [0, 4, 4, -2], [5, 1, 1, 5]], F32)
    want = {("sum", "target"): ([[1, 14, 3], [0, 8, -2], [5, 2, 5]], None),
            ("mean", "target"): ([[1, 7, 3], [0, 4, -2], [5, 1, 5]], None),
            ("max", "target"): ([[1, 8, 3], [0, 4, -2], [5, 1, 5]], [[0, 2, 3], [0, 1, 3], [0, 1, 3]]),
            ("min", "target"): ([[1, 6, 3], [0, 4, -2], [5, 1, 5]], [[0, 1, 3], [0, 1, 3], [0, 1, 3]]),
            ("sum", "source"): ([[6, 4, 8], [4, -2, 4], [1, 10, 1]], None),
            ("mean", "source"): ([[6, 2, 8], [4, -1, 4], [1, 5, 1]], None),
            ("max", "source"): ([[6, 3, 8], [4, 0, 4], [1, 5, 1]], [[1, 3, 2], [1, 0, 2], [1, 0, 2]]),
            ("min", "source"): ([[6, 1, 8], [4, -2, 4], [1, 5, 1]], [[1, 0, 2], [1, 3, 2], [1, 0, 2]])}
    for (how, to), (y, arg) in want.items():
        got_y, got_arg, deg = R.reduce(m, ent, how, to)
        assert got_y.dtype == F32 and got_y.tolist() == [y] and deg.tolist() == [1, 2, 1], (how, to)
        assert (got_arg is None) if arg is None else (got_arg.dtype == np.int32 and got_arg.tolist() == [arg]), (how, to)
    # the backwards: the sum's is the gather, the mean's the gather of g / d, the extremum's g at the entry its argmax names
    g = np.array([[[1, 10, 100], [2, 20, 200], [3, 30, 300]]], F32)
    assert R.reduce_backward(g, ent, "sum", "target").tolist() == [[1, 10, 10, 100], [2, 20, 20, 200], [3, 30, 30, 300]]
    assert R.reduce_backward(g, ent, "sum", "source").tolist() == [[10, 1, 100, 10], [20, 2, 200, 20], [30, 3, 300, 30]]
    assert R.reduce_backward(g, ent, "mean", "target", degree=[1, 2, 1]).tolist() == [[1, 5, 5, 100], [2, 10, 10, 200], [3, 15, 15, 300]]
    _, arg, _ = R.reduce(m, ent, "max", "target")
    assert R.reduce_backward(g, ent, "max", "target", argmax=arg).tolist() == [[1, 0, 10, 100], [2, 20, 0, 200], [3, 30, 0, 300]]
    _, arg, _ = R.reduce(m, ent, "min", "source")
    assert R.reduce_backward(g, ent, "min", "source", argmax=arg).tolist() == [[10, 1, 100, 0], [0, 2, 200, 20], [30, 3, 300, 0]]
    gm = np.array([[1, 2, 4, 8], [16, 32, 64, 128]], F32)
    assert R.gather_backward(gm, ent, "target").tolist() == [[[1, 6, 8], [16, 96, 128]]]
    assert R.gather_backward(gm, ent, "source").tolist() == [[[2, 9, 4], [32, 144, 64]]]


def test_model_on_invalid_entries_and_empty_rows():
    # row 0 holds entry 0 (valid) and entry 1 (index -1), row 1 entry 2 (index K), row 2 nothing; entries 3 and 4 lie behind the last row
    ent = R.Entries(np.array([0, 2, 3, 3]), np.array([1, -1, 3, 0, 1], np.int32), 1, 3)
    assert ent.valid.tolist() == [True, False, False, False, False]
    x = np.array([[[-0.0, np.nan, 3]]], F32)
    xi, xj = R.gather(x, ent, "target"), R.gather(x, ent, "source")
    assert np.signbit(xi[0, 0]) and xi[0, 0] == 0 and np.isnan(xj[0, 0])       # a copy: the sign of zero and NaN pass through
    assert positive_zeros(xi[:, 1:]) and positive_zeros(xj[:, 1:])
    m = np.array([[-5, 9, 9, 9, 9]], F32)
    for how in R.REDUCES:
        y, arg, deg = R.reduce(m, ent, how, "target")
        assert y.tolist() == [[[-5, 0, 0]]] and positive_zeros(y[0, 0, 1:]) and deg.tolist() == [1, 0, 0], how
        assert arg is None or arg.tolist() == [[[0, -1, -1]]]
        y, arg, deg = R.reduce(m, ent, how, "source")
        assert y.tolist() == [[[0, -5, 0]]] and positive_zeros(y[0, 0, [0, 2]]) and deg.tolist() == [0, 1, 0], how
        assert arg is None or arg.tolist() == [[[-1, 0, -1]]]
        g = np.array([[[7, 8, 9]]], F32)
        gm = R.reduce_backward(g, ent, how, "target", arg if how in ("max", "min") else None, [1, 0, 0])
        assert positive_zeros(gm[:, 1:]) and gm[0, 0] == (0 if how in ("max", "min") else 7), how      # (this argmax is the source's: it names no row)
    # -0.0 stays -0.0 only where it is copied; a sum starts from +0.0
    assert not np.signbit(R.reduce(np.array([[-0.0, 0, 0, 0, 0]], F32), ent, "sum")[0][0, 0, 0])
    assert np.signbit(R.reduce(np.array([[-0.0, 0, 0, 0, 0]], F32), ent, "max")[0][0, 0, 0])


# ---- the identities with the aggregation and the attention models ----
def case(seed, N, K, degree):
    rng = np.random.default_rng(seed)
    frames = [random_pairs(rng, K, degree) for _ in range(N - 1)] + [path(K) + star(K, min(10, K - 1))]
    offsets, indices = numpy_lists(neighbour_lists(make_graph(frames, K)))
    return rng, R.Entries(offsets, indices, N, K), offsets, indices


CASES = [(0, 1, 9, 3, 1), (1, 2, 40, 6, 5), (2, 3, 64, 8, 4), (3, 1, 130, 4, 3)]      # seed, N, K, mean degree, channels


@pytest.mark.parametrize("seed,N,K,degree,C", CASES)
def test_reduce_of_the_source_gather_is_graph_aggregate(seed, N, K, degree, C):
    rng, ent, offsets, indices = case(seed, N, K, degree)
    x, g = (rng.standard_normal((N, C, K)).astype(F32) for _ in range(2))
    x[0, 0, : K // 2] = F32(0.5)                                               # ties for the max
    xj = R.gather(x, ent, "source")
    for how in ("sum", "mean", "max"):
        y, arg, deg = R.reduce(xj, ent, how)
        want, want_arg, want_deg = A.forward(x, offsets, indices, None, how)
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)) and np.array_equal(deg, want_deg), how
        assert arg is None or np.array_equal(arg, want_arg)
        gx = R.gather_backward(R.reduce_backward(g, ent, how, "target", arg, deg), ent, "source")
        want = A.backward_values(g, offsets, indices, None, how, want_arg, want_deg)
        assert np.array_equal(gx.view(np.uint32), want.view(np.uint32)), how


@pytest.mark.parametrize("seed,N,K,degree,C", CASES)
def test_weighted_messages_are_the_weighted_aggregate(seed, N, K, degree, C):
    rng, ent, offsets, indices = case(seed + 10, N, K, degree)
    x, g = (rng.standard_normal((N, C, K)).astype(F32) for _ in range(2))
    w = rng.standard_normal(ent.nnz).astype(F32)
    xj = R.gather(x, ent, "source")
    assert np.array_equal(R.reduce(w[None] * xj, ent)[0], A.forward(x, offsets, indices, w)[0])
    # the gradient for w through the product, folded over c from the left as the model of grad_weight folds
    gm = R.reduce_backward(g, ent, "sum", "target")
    acc = np.zeros(ent.nnz, F32)
    for c in range(C):
        acc = acc + gm[c] * xj[c]
    assert np.array_equal(acc, A.backward_weight(x, g, offsets, indices))
    # and the gradient for x: the gather's backward of w * grad_m
    assert np.array_equal(R.gather_backward(w[None] * gm, ent, "source"), A.backward_values(g, offsets, indices, w))


@pytest.mark.parametrize("seed,N,K,degree,C", CASES)
def test_sum_to_the_source_is_rule_a_transposed(seed, N, K, degree, C):
    rng, ent, offsets, indices = case(seed + 20, N, K, degree)
    m = rng.standard_normal((C, ent.nnz)).astype(F32)
    assert np.array_equal(R.reduce(m, ent, "sum", "source")[0], M.apply_transposed(np.ones((N, C, K), F32), m, ent))


# ---- against float64: torch's autograd of a dense restatement ----
def gather64(x, ent, end):
    N, C, K = x.shape
    node, valid = torch.from_numpy(R.node_of(ent, end)), torch.from_numpy(ent.valid)
    return x.transpose(0, 1).reshape(C, N * K).index_select(1, node) * valid


def reduce64(m, ent, how, to):
    Fc, RR = m.shape[0], ent.N * ent.K
    p = torch.from_numpy(np.nonzero(ent.valid)[0])
    node = torch.from_numpy(R.node_of(ent, to))[p]
    if how in ("sum", "mean"):
        y = torch.zeros((Fc, RR), dtype=m.dtype).index_add(1, node, m[:, p])
        if how == "mean":
            y = y / torch.bincount(node, minlength=RR).clamp(min=1)
    else:
        y = torch.zeros((Fc, RR), dtype=m.dtype).scatter_reduce(1, node.expand(Fc, -1), m[:, p], "amax" if how == "max" else "amin", include_self=False)
    return y.reshape(Fc, ent.N, ent.K).transpose(0, 1)


@pytest.mark.parametrize("seed,N,K,degree,C", CASES)
def test_model_against_float64_autograd(seed, N, K, degree, C):
    """A gather, an extremum and the masked gradient are copies and selections: equality (no ties in random messages, so torch does not
    split a gradient).  A sum of d terms is d - 1 roundings and the mean one more: gamma(d) * sum |terms| (messages_ref's docstring);
    the mean's backward is one division: u |exact| / (1 - u) = gamma(0) |exact|."""
    rng, ent, offsets, indices = case(seed + 30, N, K, degree)
    x = rng.standard_normal((N, C, K)).astype(F32)
    m, gm = (rng.standard_normal((C, ent.nnz)).astype(F32) for _ in range(2))
    gy = rng.standard_normal((N, C, K)).astype(F32)
    for end in ("target", "source"):
        d = np.bincount(R.node_of(ent, end)[ent.valid], minlength=N * K).reshape(N, 1, K)
        leaf = t64(x).requires_grad_()
        out = gather64(leaf, ent, end)
        out.backward(t64(gm))
        assert np.array_equal(R.gather(x, ent, end), out.detach().numpy())
        terms = reduce64(t64(np.abs(gm)), ent, "sum", end).numpy()
        assert (np.abs(R.gather_backward(gm, ent, end) - leaf.grad.numpy()) <= A.gamma(d) * terms).all() and np.abs(leaf.grad.numpy()).max() > 0
        for how in R.REDUCES:
            leaf = t64(m).requires_grad_()
            y64 = reduce64(leaf, ent, how, end)
            y64.backward(t64(gy))
            y, arg, deg = R.reduce(m, ent, how, end)
            got = R.reduce_backward(gy, ent, how, end, arg, deg)
            assert np.array_equal(deg.reshape(N, 1, K), d)
            if how in ("max", "min"):
                assert np.array_equal(y, y64.detach().numpy()) and np.array_equal(got, leaf.grad.numpy()), (how, end)
                assert ((arg >= 0) == (d > 0)).all()
            else:
                terms = reduce64(t64(np.abs(m)), ent, how, end).numpy()
                assert (np.abs(y - y64.detach().numpy()) <= A.gamma(d) * terms).all(), (how, end)
                if how == "sum":
                    assert np.array_equal(got, leaf.grad.numpy()), end
                else:
                    assert (np.abs(got - leaf.grad.numpy()) <= A.gamma(0) * np.abs(leaf.grad.numpy())).all(), end
            assert np.abs(leaf.grad.numpy()).max() > 0


# ---- argument errors: all before any device work (a CPU tensor is the last thing refused) ----
G = make_graph([path(5), star(5, 3)], 5)                                   # N = 2, K = 5, E = 7, nnz = 14
NL = neighbour_lists(G)
PAIR = (NL.offsets, NL.indices)
X = torch.zeros((2, 4, 5))
S = torch.zeros((2, 14))
NK = dict(num_frames=2, num_components=5)


def refused(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def test_bad_gather_arguments():
    for lists in (G, NL, PAIR):
        refused("x must be float32", entry_gather, X.double(), lists)
        refused(r"x must be \[C, K\] or \[N, C, K\]", entry_gather, torch.zeros(5), lists)
        refused("x must be a torch tensor", entry_gather, None, lists)
        refused("x must not be empty", entry_gather, torch.zeros((2, 0, 5)), lists)
        refused(r"the values have 3 of 5|graph offsets must be \[N \* K \+ 1\] = \[16\]", entry_gather, torch.zeros((3, 4, 5)), lists)
        refused(r"the values have 1 of 5|graph offsets must be \[N \* K \+ 1\] = \[6\]", entry_gather, X[0], lists)
        refused("K, the last dimension of x, must be in", entry_gather, torch.zeros((1, 1, 65535)), lists)
        for end in ("both", 0, None, b"target"):
            refused("end must be 'target' or 'source'", entry_gather, X, lists, end)
    refused("a pair", entry_gather, X, None)
    refused("graph indices must be int32", entry_gather, X, (NL.offsets, NL.indices.long()))


def test_bad_reduce_arguments():
    for lists, kw in ((G, {}), (NL, {}), (PAIR, NK)):
        refused(r"messages must be \[F, nnz\] or \[nnz\] with nnz = 14", entry_reduce, torch.zeros((2, 13)), lists, **kw)
        refused(r"messages must be \[F, nnz\]", entry_reduce, torch.zeros((0, 14)), lists, **kw)
        refused(r"messages must be \[F, nnz\]", entry_reduce, torch.zeros((1, 2, 14)), lists, **kw)
        refused("messages must be float32", entry_reduce, S.double(), lists, **kw)
        refused("messages must be a torch tensor", entry_reduce, None, lists, **kw)
        for how in ("std", "amax", 2, None):
            refused("reduce must be 'sum', 'mean', 'max' or 'min'", entry_reduce, S, lists, how, **kw)
        for to in ("both", 1, None):
            refused("to must be 'target' or 'source'", entry_reduce, S, lists, "sum", to, **kw)
        for how in ("sum", "mean"):
            refused("return_argmax goes with reduce='max' and 'min' only", entry_reduce, S, lists, how, return_argmax=True, **kw)
    refused("num_frames must be an integer", entry_reduce, S, PAIR)
    refused("num_components must be an integer", entry_reduce, S, PAIR, num_frames=2)
    refused(r"graph offsets must be \[N \* K \+ 1\] = \[13\]", entry_reduce, S, PAIR, num_frames=2, num_components=6)
    refused("the graph has 2 frames of 5 nodes, not 2 of 6", entry_reduce, S, NL, num_frames=2, num_components=6)
    refused("a pair", entry_reduce, S, None, **NK)


def test_2_to_the_31_limits():
    """Tensors of the sizes in question without their memory: one element expanded."""
    text = r"N \* C \* K, the number of neighbour entries and C \* entries must be below 2\^31"
    K = 1 << 15
    offsets = torch.zeros(1, dtype=torch.int64).expand(K + 1)
    big = torch.zeros((1, 1, 1)).expand(1, 1 << 16, K)
    few = torch.zeros(4, dtype=torch.int32)
    refused(text, entry_gather, big, (offsets, few))
    refused("no CPU fallback", entry_gather, big[:, :-1], (offsets, few))
    refused(text, entry_reduce, torch.zeros((1, 1)).expand(1 << 16, 4), (offsets, few), num_frames=1, num_components=K)
    small = torch.zeros(11, dtype=torch.int64)
    for nnz, Cc, ok in ((1 << 31, 1, False), (1 << 29, 4, False), ((1 << 29) - 1, 4, True), ((1 << 31) - 1, 1, True)):
        lists = (small, torch.zeros(1, dtype=torch.int32).expand(nnz))
        match = "no CPU fallback" if ok else text                          # just below: the next refusal is the device's
        refused(match, entry_gather, torch.zeros((2, Cc, 5)), lists)
        refused(match, entry_reduce, torch.zeros((1, 1)).expand(Cc, nnz), lists, **NK)


def test_cpu_tensors_are_refused_after_every_other_check():
    for lists, kw in ((G, {}), (NL, {}), (PAIR, NK)):
        refused("x must be on a ROCm GPU, got device cpu .there is no CPU fallback.", entry_gather, X, lists, "source")
        refused("messages must be on a ROCm GPU, got device cpu .there is no CPU fallback.", entry_reduce, S, lists, "min", "source", return_argmax=True, **kw)
        refused("messages must be on a ROCm GPU", entry_reduce, S[0], lists, **kw)                       # the 1-D form
    refused("x must be on a ROCm GPU", entry_gather, X[0], neighbour_lists(make_graph([path(5)], 5)))      # [C, K]


def test_the_tensors_are_handed_to_one_device_in_this_order(monkeypatch):
    """No GPU here, let alone two: _tensors.one_device refuses two GPUs first and a CPU tensor last (tests/test_aggregate_cpu.py)."""
    seen = []

    def one_device(tensors):
        seen.append([name for _, name in tensors])
        raise ValueError("stop")

    monkeypatch.setattr(messages.T, "one_device", one_device)
    refused("stop", entry_gather, X, NL)
    refused("stop", entry_reduce, S, G)
    refused("stop", entry_reduce, S, PAIR, **NK)
    assert seen == [["x", "nl.offsets", "nl.indices"], ["messages", "graph.edge_index", "graph.offsets"], ["messages", "graph offsets", "graph indices"]]


def test_the_package_itself_does_not_import_the_module():
    assert "messages" not in open(os.path.join(ROOT, "fast_slic_amd", "__init__.py")).read()
    assert messages.__all__ == ["entry_gather", "entry_reduce"] and "bit for bit" in messages.__doc__


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
NAMES = ["fslic_hip_message_gather", "fslic_hip_message_reduce"]


def lib():
    return B.load_library()


def test_exports():
    header = open(os.path.join(ROOT, "include", "fslic_hip.h")).read()
    assert [n for n in B.EXPORTS if "_message_" in n] == NAMES and all(hasattr(lib(), n) and "int %s(" % n in header for n in NAMES)
    assert B.EXPORTS.index("fslic_hip_knn_graph") < B.EXPORTS.index(NAMES[0])
    assert B.EXPORTS.index(NAMES[-1]) < B.EXPORTS.index("fslic_hip_pool_workspace_size")      # in front of the pinned tail of the table


# streamapi.h's checks of a [N][C][K] call (N = 0 leaves no way to N * C * K >= 2^31), then the cells of a [C][nnz] array
CELLS = [("stream", dict(device=-1), b"device must be >= 0"), ("stream", dict(N=0), b"N must be positive"), ("stream", dict(C=0), b"C must be positive"),
         ("stream", dict(K=65535), b"K must be in [1, 65534]"), ("stream", dict(N=1 << 16, K=1 << 15), b"N * C * K must be below 2^31"),
         ("stream", dict(nnz=-1), b"nnz must be in [0, 2^31)"), ("message:1", dict(nnz=1 << 30), b"C * nnz must be below 2^31")]
CALL = dict(device=DEVICE, stream=NUL, N=2, C=3, K=5, nnz=14)

# (entry, valid arguments, checks in source order, argument sets answered with FSLIC_OK before any HIP call, the pointers refused alone)
# the max and the mean are one argument: each of the two checks is violated with the value it is about
TABLE = [
    ("fslic_hip_message_gather", dict(CALL, end=1, rows=P, indices=P, values=P, scale_degree=P, argmax=P, out=P),
     CELLS + [("message:2", dict(end=2), b"end must be 0 (target) or 1 (source)"),
              ("message:3", dict(values=NUL, rows=NUL, indices=NUL, out=NUL), NULL_ARG)],
     [dict(nnz=0), dict(nnz=0, rows=NUL, indices=NUL, scale_degree=NUL, argmax=NUL, out=NUL)], ["rows", "indices", "values", "out"]),
    # (without entries the reduce is still a launch, of zeros: no row of FSLIC_OK)
    ("fslic_hip_message_reduce", dict(CALL, reduce=0, transposed=1, offsets=P, ia=P, ib=P, messages=P, out=P, argmax=P, degree=P),
     CELLS + [("message:4", dict(reduce=4), b"reduce must be 0 (sum), 1 (mean), 2 (max) or 3 (min)"),
              ("message:5", dict(transposed=2), b"transposed must be 0 or 1"),
              ("message:6", dict(reduce=2, argmax=NUL), b"reduce 2 (max) and 3 (min) need argmax"),
              ("message:7", dict(reduce=1, degree=NUL), b"reduce 1 (mean) needs degree"),
              ("message:8", dict(offsets=NUL, ia=NUL, ib=NUL, messages=NUL, out=NUL), NULL_ARG)],
     [], ["offsets", "ia", "ib", "messages", "out"]),
]
REFUSALS = [pytest.param(name, args, text, id="%s-%d-%s" % (name[len("fslic_hip_"):], i, site))
            for name, valid, checks, _, _ in TABLE for i, (site, args, text) in enumerate(rows_of(valid, checks))]
ALONE = [pytest.param(name, dict(valid, **{p: NUL}), id="%s-%s" % (name[len("fslic_hip_"):], p)) for name, valid, _, _, ps in TABLE for p in ps]
NOTHING_TO_DO = [pytest.param(name, dict(valid, **kw), id="%s-%d" % (name[len("fslic_hip_"):], i)) for name, valid, _, oks, _ in TABLE for i, kw in enumerate(oks)]


def test_the_table_holds_every_entry_and_reaches_every_site():
    assert [name for name, _, _, _, _ in TABLE] == NAMES
    for name, valid, _, _, _ in TABLE:
        assert len(valid) == len(dict((n, a) for n, _, a in B.SIGNATURES)[name]), name
    source = open(os.path.join(ROOT, "fast_slic_amd", "csrc", "messageapi.cpp")).read()
    sites = source.count("fail(FSLIC_E_INVALID")
    reached = {site for _, _, checks, _, _ in TABLE for site, _, _ in checks if site != "stream"}
    assert sites == 8 and reached == {"message:%d" % (i + 1) for i in range(sites)}


@pytest.mark.parametrize("name,args,text", REFUSALS)
def test_refused_with_these_words(name, args, text):
    assert (getattr(lib(), name)(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, text)


def test_the_min_needs_argmax_and_a_sum_needs_neither():
    valid = TABLE[1][1]
    args = dict(valid, reduce=3, argmax=NUL, degree=NUL, offsets=NUL)
    assert (lib().fslic_hip_message_reduce(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, b"reduce 2 (max) and 3 (min) need argmax")
    args = dict(valid, reduce=0, argmax=NUL, degree=NUL, offsets=NUL)          # the next refusal is the pointer's
    assert (lib().fslic_hip_message_reduce(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, NULL_ARG)
    args = dict(valid, transposed=0, ib=NUL, nnz=0, ia=NUL, messages=NUL, out=NUL)      # ib, ia and messages are not read; out is
    assert (lib().fslic_hip_message_reduce(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, NULL_ARG)


@pytest.mark.parametrize("name,args", ALONE)
def test_every_pointer_is_refused_alone(name, args):
    assert (getattr(lib(), name)(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, NULL_ARG)


@pytest.mark.parametrize("name,args", NOTHING_TO_DO)
def test_nothing_to_do_is_ok_before_any_hip_call(name, args):
    assert getattr(lib(), name)(*args.values()) == B.FSLIC_OK
