"""CPU tests of the nearest neighbours in feature space (fast_slic_amd/knn.py, fslic_hip_knn_graph): the numpy model (tests/knn_ref.py)
by hand, the model against a float64 brute force on integer-valued points (exact in both precisions: equality, ties included), the
arithmetic of the fixed-degree lists in plain torch, and every argument error refused before any device work -- ValueError in Python,
FSLIC_E_INVALID from the C ABI before its first HIP call, with the words and the order of csrc/knnapi.cpp.  No kernel is launched here."""
import os

import numpy as np
import pytest
import torch

import knn_ref as M
from fast_slic_amd import _binding as B
from fast_slic_amd import knn
from fast_slic_amd.knn import fixed_degree_lists, knn_graph
from fast_slic_amd.propagate import NeighbourLists
from test_stream_refusals_cpu import DEVICE, NUL, NULL_ARG, P, rows_of

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = np.inf, np.nan


def line(*xs):
    return np.array([[list(xs)]], F32)                                     # N = 1, D = 1


def lists(points, k, **kw):
    ind, d = M.knn(points, k, **kw)
    K = points.shape[2]
    return ind.reshape(-1, K, k).tolist(), d.reshape(-1, K, k).tolist()


# ---- the model, by hand ----
def test_model_on_a_line_with_an_exact_tie():
    # 0 1 2 4: node 1 is at distance 1 from nodes 0 and 2, and the smaller index wins
    ind, d = lists(line(0, 1, 2, 4), 2)
    assert ind == [[[1, 2], [0, 2], [1, 0], [2, 1]]] and d == [[[1, 4], [1, 1], [1, 4], [4, 9]]]
    ind, d = lists(line(0, 1, 2, 4), 1)
    assert ind == [[[1], [0], [1], [2]]] and d == [[[1], [1], [1], [4]]]


def test_model_on_equal_points_takes_the_smallest_indices_other_than_itself():
    ind, d = lists(np.full((1, 3, 5), 2.5, F32), 3)
    assert ind == [[[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2]]] and not np.any(d) and not np.signbit(d).any()


def test_model_with_special_values_masks_loop_and_other():
    # a NaN channel: node 2 is nobody's neighbour and has no neighbour
    ind, d = lists(np.array([[[0, 1, 5, 3], [0, 0, NAN, 0]]], F32), 2)
    assert ind == [[[1, 3], [0, 3], [-1, -1], [1, 0]]] and d == [[[1, 9], [1, 4], [INF, INF], [4, 9]]]
    # a +inf channel: an ordinary distance, the largest; inf - inf is NaN and drops out
    ind, d = lists(np.array([[[0, 1, INF, INF]]], F32), 3)
    assert ind == [[[1, 2, 3], [0, 2, 3], [0, 1, -1], [0, 1, -1]]] and d == [[[1, INF, INF], [1, INF, INF], [INF, INF, INF], [INF, INF, INF]]]
    # an invalid node is nobody's neighbour and its row is all padding
    ind, d = lists(line(0, 1, 2, 4), 2, valid=np.array([[True, False, True, True]]))
    assert ind == [[[2, 3], [-1, -1], [0, 3], [2, 0]]] and d == [[[4, 16], [INF, INF], [4, 4], [4, 16]]]
    # loop=True: the node itself first, at +0
    ind, d = lists(line(0, 1, 2, 4), 2, loop=True)
    assert ind == [[[0, 1], [1, 0], [2, 1], [3, 2]]] and d == [[[0, 1], [0, 1], [0, 1], [0, 4]]]
    # other=: candidates from the other tensor, the same index included
    ind, d = lists(line(0, 1, 2, 4), 2, other=line(4, 0, 0, 1))
    assert ind == [[[1, 2], [3, 1], [3, 0], [0, 3]]] and d == [[[0, 0], [0, 1], [1, 4], [0, 9]]]      # node 2: 0, 1 and 2 tie at 4
    # two frames do not see each other
    ind, d = lists(np.array([[[0, 1, 3]], [[7, 0, 6]]], F32), 1)
    assert ind == [[[1], [0], [1]], [[2], [2], [0]]] and d == [[[1], [1], [4]], [[1], [36], [1]]]


def test_model_pads_behind_the_last_candidate():
    ind, d = lists(line(0, 1, 3), 4)
    assert ind == [[[1, 2, -1, -1], [0, 2, -1, -1], [1, 0, -1, -1]]] and d == [[[1, 9, INF, INF], [1, 4, INF, INF], [4, 9, INF, INF]]]
    ind, d = lists(line(5), 2)
    assert ind == [[[-1, -1]]] and d == [[[INF, INF]]]
    ind, d = M.knn(line(0, 1, 3), 4)
    assert ind.dtype == np.int32 and d.dtype == F32 and ind.shape == d.shape == (12,)


def test_the_fold_is_three_rounded_operations_a_channel():
    # (1 + 2^-12)^2 rounds in float32, and the sum of two such terms rounds again: float64 differs, the written fold does not
    a = F32(1) + F32(2.0 ** -12)
    x = np.array([[[a, 0], [a, 0], [3, 0]]], F32)
    t = F32(a * a)
    want = F32(F32(F32(0) + t) + t) + F32(9)
    d = M.distances(x, x)
    assert d.dtype == F32 and d[0, 0, 1] == F32(want) == d[0, 1, 0] and d[0, 0, 0] == 0
    assert float(d[0, 0, 1]) != 2 * float(a) ** 2 + 9


@pytest.mark.parametrize("seed,N,D,K,k", [(0, 1, 1, 9, 3), (1, 2, 3, 40, 8), (2, 3, 33, 31, 32), (3, 1, 5, 130, 16), (4, 2, 2, 64, 1)])
def test_model_against_float64_brute_force_on_integer_points(seed, N, D, K, k):
    """Coordinates are integers in [-64, 64] and D <= 33: every partial sum is an integer at most 33 * 128^2 < 2^24, exact in float32
    and in float64, so indices and distances are equal exactly, ties included, in every row."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-64, 65, (N, D, K)).astype(F32)
    y = rng.integers(-64, 65, (N, D, K)).astype(F32)
    valid = rng.random((N, K)) < 0.8
    for kw in (dict(), dict(loop=True), dict(other=y), dict(valid=valid), dict(other=y, valid=valid)):
        ind, d = M.knn(x, k, **kw)
        ind64, d64 = M.brute64(x, k, **kw)
        assert np.array_equal(ind, ind64) and np.array_equal(d.astype(np.float64), d64), kw
    ind, d = M.knn(x, k)
    d = d.reshape(N * K, k)
    assert (d[:, 1:] >= d[:, :-1]).all()                                   # ascending, the padding last


# ---- the arithmetic of the lists, in plain torch ----
def test_fixed_degree_lists_and_their_transpose():
    N, K, k = 2, 4, 3
    indices = torch.tensor([1, 2, -1, 0, 2, 3, 3, -1, -1, -1, -1, -1,
                            3, 3, 0, 0, -1, -1, 1, 0, 3, 2, 1, 0], dtype=torch.int32)      # asymmetric, padded, one row all padding
    nl = fixed_degree_lists(indices, N, K, k)
    assert isinstance(nl, NeighbourLists) and nl.edge is None and (nl.num_frames, nl.num_components) == (N, K)
    assert nl.offsets.dtype == torch.int64 and nl.offsets.tolist() == [3 * r for r in range(N * K + 1)]
    assert nl.rows.dtype == torch.int32 and nl.rows.tolist() == [r for r in range(N * K) for _ in range(k)]
    assert nl.indices is indices and nl.degree().dtype == torch.int32 and nl.degree().tolist() == [[3] * K] * N
    t_offsets, t_entries, t_rows = nl.transposed()
    want = [[] for _ in range(N * K)]
    for p, j in enumerate(indices.tolist()):                               # target (f, j) <- entry p of row p // k, ascending p
        if 0 <= j < K:
            want[(p // k) // K * K + j].append(p)
    got = [t_entries[t_offsets[r]:t_offsets[r + 1]].tolist() for r in range(N * K)]
    assert got == want and int(t_offsets[-1]) == sum(len(w) for w in want) == 16
    assert all(t_rows[t_offsets[r]:t_offsets[r + 1]].tolist() == [p // k for p in want[r]] for r in range(N * K))


# ---- argument errors: all before any device work (a CPU tensor is the last thing refused) ----
X = torch.zeros((2, 3, 5))
V = torch.ones((2, 5), dtype=torch.bool)


def refused(match, *args, **kw):
    with pytest.raises(ValueError, match=match):
        knn_graph(*args, **kw)


def test_bad_points_k_other_and_valid():
    refused("points must be float32", X.double(), 2)
    refused("points must be float32", X.half(), 2)
    refused("points must be a torch tensor", X.numpy(), 2)
    refused(r"points must be \[D, K\] or \[N, D, K\]", torch.zeros(5), 2)
    refused(r"points must be \[D, K\] or \[N, D, K\]", torch.zeros((1, 2, 3, 5)), 2)
    refused("points must not be empty", torch.zeros((2, 0, 5)), 2)
    refused("K, the last dimension of points, must be in", torch.zeros((1, 1, 1)).expand(1, 1, 65535), 2)
    refused(r"D, the channels of points, must be in \[1, 4096\], got 4097", torch.zeros((1, 1, 1)).expand(1, 4097, 5), 2)
    for k in (0, 33, -1, 2.0, True, None, "2"):
        refused(r"k must be an integer in \[1, 32\]", X, k)
    refused(r"other must be the shape of points, \(2, 3, 5\)", X, 2, other=torch.zeros((2, 3, 4)))
    refused(r"other must be the shape of points, \(2, 3, 5\)", X, 2, other=X[0])
    refused("other must be float32", X, 2, other=X.double())
    refused("other must be a torch tensor", X, 2, other=X.numpy())
    refused("loop goes with points alone", X, 2, other=X.clone(), loop=True)
    refused(r"valid must be \[2, 5\], one per node", X, 2, valid=V[:, :4])
    refused(r"valid must be \[2, 5\], one per node", X, 2, valid=V[0])
    refused(r"valid must be \[5\], one per node", X[0], 2, valid=V)
    refused("valid must be bool", X, 2, valid=V.to(torch.uint8))
    refused("valid must be bool", X, 2, valid=V.float())


def test_2_to_the_31_limit():
    """Tensors of the sizes in question without their memory: one element expanded."""
    big = torch.zeros((1, 1, 1)).expand(1 << 11, 1, 1 << 15)               # N * K = 2^26
    refused(r"N \* K \* k must be below 2\^31", big, 32)
    refused("no CPU fallback", big, 31)                                     # just below: the next refusal is the device's


def test_cpu_tensors_are_refused_after_every_other_check():
    text = "points must be on a ROCm GPU, got device cpu .there is no CPU fallback."
    refused(text, X, 2)
    refused(text, X[0], 32, valid=V[0], loop=True)
    refused(text, X.transpose(1, 2), 2, other=X.transpose(1, 2).clone(), valid=torch.zeros((2, 3), dtype=torch.bool))


def test_the_tensors_are_handed_to_one_device_in_this_order(monkeypatch):
    """No GPU here, let alone two: _tensors.one_device refuses two GPUs first and a CPU tensor last (tests/test_aggregate_cpu.py)."""
    seen = []

    def one_device(tensors):
        seen.append([(name, t is not None) for t, name in tensors])
        raise ValueError("stop")

    monkeypatch.setattr(knn.T, "one_device", one_device)
    refused("stop", X, 2)
    refused("stop", X, 2, other=X, valid=V)
    assert seen == [[("points", True), ("other", False), ("valid", False)], [("points", True), ("other", True), ("valid", True)]]


def test_the_module_says_what_it_leaves_out():
    text = " ".join(knn.__doc__.split())
    for words in ("Out of scope", "other metrics", "radius cut", "approximate search", "k > 32", "float16 / bfloat16", "gradients of the selection",
                  "symmetrising the lists", "no CPU fallback", "not differentiable"):
        assert words in text, words
    assert knn.__all__ == ["knn_graph"]
    import fast_slic_amd
    assert "torch" not in getattr(fast_slic_amd, "__all__", [])


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
NAME = "fslic_hip_knn_graph"


def lib():
    return B.load_library()


def test_export_order():
    header = open(os.path.join(ROOT, "include", "fslic_hip.h")).read()
    assert NAME in B.EXPORTS and hasattr(lib(), NAME) and "int %s(" % NAME in header
    assert B.EXPORTS.index("fslic_hip_attend_apply") < B.EXPORTS.index(NAME) < B.EXPORTS.index("fslic_hip_pool_workspace_size")


# streamapi.h's checks of a [N][D][K] call (N = 0 leaves no way to N * D * K >= 2^31; its words name the channels C), then the entry's
# own, in source order; N * K * k needs a k that passes the range check
CHECKS = [("stream", dict(device=-1), b"device must be >= 0"), ("stream", dict(N=0), b"N must be positive"), ("stream", dict(D=0), b"C must be positive"),
          ("stream", dict(K=65535), b"K must be in [1, 65534]"), ("stream", dict(N=1 << 16, K=1 << 15), b"N * C * K must be below 2^31"),
          ("knn:1", dict(k=33), b"k must be in [1, 32]"), ("knn:2", dict(N=1 << 12, K=1 << 15, k=16), b"N * K * k must be below 2^31"),
          ("knn:3", dict(loop=1, other=P), b"loop goes with points alone, not with other"),
          ("knn:4", dict(points=NUL, indices=NUL, dist=NUL), NULL_ARG)]
VALID = dict(device=DEVICE, stream=NUL, N=2, D=3, K=5, k=2, loop=0, points=P, other=P, valid=P, indices=P, dist=P)
REFUSALS = [pytest.param(args, text, id="%d-%s" % (i, site)) for i, (site, args, text) in enumerate(rows_of(VALID, CHECKS))]


def test_the_table_reaches_every_site():
    assert len(VALID) == len(dict((n, a) for n, _, a in B.SIGNATURES)[NAME])
    source = open(os.path.join(ROOT, "fast_slic_amd", "csrc", "knnapi.cpp")).read()
    sites = source.count("fail(FSLIC_E_INVALID")
    assert sites == 4 and {site for site, _, _ in CHECKS if site != "stream"} == {"knn:%d" % (i + 1) for i in range(sites)}
    # all checks stand in front of the first HIP call
    assert source.index("NULL pointer argument") < source.index("on_stream(")


@pytest.mark.parametrize("args,text", REFUSALS)
def test_refused_with_these_words(args, text):
    assert (getattr(lib(), NAME)(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, text)


@pytest.mark.parametrize("k", [0, -1, 33])
def test_k_outside_its_range(k):
    assert (getattr(lib(), NAME)(*dict(VALID, k=k).values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, b"k must be in [1, 32]")


@pytest.mark.parametrize("pointer", ["points", "indices", "dist"])
def test_every_needed_pointer_is_refused_alone(pointer):
    for extra in (dict(), dict(other=NUL, valid=NUL, loop=1)):             # `other` and `valid` may be NULL: they are no refusal
        args = dict(VALID, **extra)
        args[pointer] = NUL
        assert (getattr(lib(), NAME)(*args.values()), lib().fslic_hip_last_error()) == (B.FSLIC_E_INVALID, NULL_ARG)
