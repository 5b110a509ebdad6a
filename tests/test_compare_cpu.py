"""CPU tests of the comparison of two label maps (fast_slic_amd/compare.py, the fslic_hip_overlap* and fslic_hip_boundary_match entries):
the numpy model (tests/compare_ref.py) against plain Python loops on maps small enough to check that way and against the host
yardsticks of tests/util.py, and every argument error refused before any device work -- ValueError in Python, FSLIC_E_INVALID from
the C ABI before its first HIP call.  No kernel is launched here."""
import ctypes as C
import math
import subprocess
import sys

import numpy as np
import pytest
import torch

import compare_ref as R
import util as U
from fast_slic_amd import _binding as B
from fast_slic_amd.compare import OverlapTable, boundary_match, capacity_limit, first_capacity, label_overlap

L = torch.zeros(5, 7, dtype=torch.int32)
O = torch.zeros(5, 7, dtype=torch.int16)


def test_package_import_stays_torch_free():
    code = "import sys, fast_slic_amd; assert 'torch' not in sys.modules; import fast_slic_amd.compare; assert 'torch' in sys.modules"
    subprocess.check_call([sys.executable, "-c", code])


# ---- the model against plain loops ----
def loops_overlap(la, ot, K, M):
    """frame -> {(a, b): pixels}"""
    out = []
    for n in range(la.shape[0]):
        d = {}
        for y in range(la.shape[1]):
            for x in range(la.shape[2]):
                a, b = int(la[n, y, x]), int(ot[n, y, x])
                if 0 <= a < K and 0 <= b < M:
                    d[(a, b)] = d.get((a, b), 0) + 1
        out.append(d)
    return out


def loops_match(la, ot, r):
    H, W = la.shape

    def is_boundary(m, y, x):
        return (x + 1 < W and m[y, x] != m[y, x + 1]) or (y + 1 < H and m[y, x] != m[y + 1, x])
    hits = nother = nlabels = 0
    for y in range(H):
        for x in range(W):
            nlabels += bool(is_boundary(la, y, x))
            if is_boundary(ot, y, x):
                nother += 1
                hits += any(is_boundary(la, v, u) for v in range(max(0, y - r), min(H, y + r + 1))
                            for u in range(max(0, x - r), min(W, x + r + 1)))
    return [hits, nother, nlabels]


SMALL = [(1, 1, 1), (1, 6, 7), (2, 5, 3), (3, 1, 7), (2, 6, 1), (3, 4, 6)]


@pytest.mark.parametrize("N,H,W", SMALL)
def test_model_overlap_against_loops(N, H, W):
    rng = np.random.default_rng(N * 100 + H * 10 + W)
    K, M = 4, 3
    la = rng.integers(-1, K + 1, (N, H, W)).astype(np.int16)                  # -1 and K: no label
    ot = rng.integers(-1, M + 1, (N, H, W)).astype(np.int64)
    if N > 1:
        la[1] = -1                                                            # a frame without a pixel that takes part
    t = R.overlap(la, ot, K, M)
    want = loops_overlap(la, ot, K, M)
    off = t["offsets"].tolist()
    assert off[0] == 0 and len(off) == N + 1
    for n in range(N):
        rows = list(zip(t["pairs"][0, off[n]:off[n + 1]].tolist(), t["pairs"][1, off[n]:off[n + 1]].tolist()))
        assert rows == sorted(want[n]) and t["count"][off[n]:off[n + 1]].tolist() == [want[n][p] for p in rows]
        assert t["frame"][off[n]:off[n + 1]].tolist() == [n] * len(rows)
    A, Bm = R.areas(t, K, M)
    maj, bo, ue = R.majority(t, K, M), R.best_overlap(t, K, M), R.undersegmentation_error(t, K, M)
    for n in range(N):
        d = want[n]
        total = sum(d.values())
        area = [sum(c for (a, _), c in d.items() if a == k) for k in range(K)]
        assert A[n].tolist() == area
        assert Bm[n].tolist() == [sum(c for (_, b), c in d.items() if b == m) for m in range(M)]
        best, leak = 0, 0
        for k in range(K):
            row = [d.get((k, m), 0) for m in range(M)]
            assert maj[n, k] == (row.index(max(row)) if area[k] else -1)
            best += max(row)
            leak += sum(min(c, area[k] - c) for c in row if c)
        if total:
            assert bo[n] == best / total and ue[n] == leak / total
        else:
            assert math.isnan(bo[n]) and math.isnan(ue[n]) and off[n] == off[n + 1]
    one = R.overlap(la[0], ot[0], K, M)                                        # an [H, W] pair is a batch of one
    assert one["offsets"].tolist() == off[:2] and np.array_equal(one["pairs"], t["pairs"][:, :off[1]])


def test_model_majority_tie_takes_the_smallest():
    la = np.zeros((2, 4), np.int32)
    ot = np.array([[2, 2, 1, 1], [3, 3, 0, 5]], np.int32)                       # label 0: b = 1, 2 and 3 with two pixels each
    t = R.overlap(la, ot, 1, 6)
    assert R.majority(t, 1, 6).tolist() == [[1]] and R.best_overlap(t, 1, 6).tolist() == [2 / 8]
    assert R.undersegmentation_error(t, 1, 6).tolist() == [(2 + 2 + 2 + 1 + 1) / 8]


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (6, 1), (3, 3), (6, 7), (5, 6)])
@pytest.mark.parametrize("r", [0, 1, 2, 5])
def test_model_boundary_match_against_loops(H, W, r):
    rng = np.random.default_rng(H * 100 + W * 10 + r)
    la = rng.integers(-1, 2, (H, W)).astype(np.int16) * (rng.random((H, W)) < 0.5)
    ot = rng.integers(0, 2, (H, W)).astype(np.int32) * (rng.random((H, W)) < 0.4)
    assert R.boundary_match(la, ot, r).tolist() == loops_match(la, ot, r)
    assert R.boundary_match(np.stack([la, la]), np.stack([ot, la]), r).tolist() == [loops_match(la, ot, r), loops_match(la, la, r)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_model_against_the_host_yardsticks(seed):
    rng = np.random.default_rng(seed)
    H, W, K, M = 37, 53, 9, 6
    y, x = np.mgrid[0:H, 0:W]
    la = ((y // 7) * 3 + x // 19 + rng.integers(0, 2, (H, W))) % K              # blocks with ragged edges, every pixel valid
    ot = ((y // 11) * 2 + x // 30 + rng.integers(0, 2, (H, W))) % M
    assert R.best_overlap(R.overlap(la, ot, K, M), K, M)[0] == U.best_overlap(la, ot)
    assert np.array_equal(R.boundary_mask(la), U.boundary_mask(la))
    hits, nother, nlabels = R.boundary_match(la, ot, 0).tolist()
    assert hits / max(1, nother + nlabels - hits) == U.boundary_iou(la, ot) and 0 < hits < min(nother, nlabels)


def test_table_methods_on_a_host_table():
    """(the methods are plain torch operations: a table built by hand on the host runs them without a GPU)"""
    la = np.array([[[0, 0, 1, 1], [2, 2, 2, 7]], [[7, 7, 7, 7], [7, 7, 7, 7]], [[1, 1, 1, 1], [0, 0, 0, 0]]], np.int64)
    ot = np.array([[[1, 0, 0, 1], [1, 1, 0, 0]], [[0, 0, 0, 0], [0, 0, 0, 0]], [[1, 1, 0, 0], [1, 0, 0, 0]]], np.int64)
    K, M = 3, 2
    ref = R.overlap(la, ot, K, M)
    t = OverlapTable(torch.from_numpy(ref["pairs"]), torch.from_numpy(ref["count"].astype(np.int32)), torch.from_numpy(ref["offsets"]),
                     K, M, 1024)
    assert ref["offsets"].tolist() == [0, 6, 6, 10]
    A, Bm = t.areas()
    assert np.array_equal(A.numpy(), R.areas(ref, K, M)[0]) and np.array_equal(Bm.numpy(), R.areas(ref, K, M)[1])
    assert A.dtype == torch.int64 and Bm.dtype == torch.int64
    assert t.majority().tolist() == R.majority(ref, K, M).tolist() == [[0, 0, 1], [-1, -1, -1], [0, 0, -1]]
    for got, want in ((t.best_overlap(), R.best_overlap(ref, K, M)), (t.undersegmentation_error(), R.undersegmentation_error(ref, K, M))):
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want, equal_nan=True) and math.isnan(got[1])
    one = R.overlap(la[0], ot[0], K, M)
    t1 = OverlapTable(torch.from_numpy(one["pairs"]), torch.from_numpy(one["count"].astype(np.int32)), torch.from_numpy(one["offsets"]),
                      K, M, 1024, batched=False)
    assert t1.majority().tolist() == [0, 0, 1] and t1.best_overlap().shape == () and t1.areas()[1].tolist() == [3, 4]


def test_capacities():
    assert first_capacity(1, 1) == 1024 and first_capacity(64, 3) == 1024 and first_capacity(3, 65) == 2048
    assert first_capacity(1600, 1600) == 32768
    assert capacity_limit(1600, 1600, 720, 1280) == 1 << 21                      # 2 * 921 600 pixels
    assert capacity_limit(300, 300, 48, 130) == 1 << 14                          # 2 * 6 240 pixels
    assert capacity_limit(2, 3, 4000, 4000) == 1024
    assert capacity_limit(65534, 65534, 40000, 40000) == 1 << 31


# ---- argument errors: all before any device work (a CPU tensor is the last thing refused) ----
def both(labels, other, **kw):
    """The two calls that must refuse alike."""
    return [lambda: label_overlap(labels, other, 4, 4, **kw), lambda: boundary_match(labels, other, **kw)]


@pytest.mark.parametrize("labels,other,match", [
    (torch.zeros(5, 7, dtype=torch.float32), O, "labels must be int16"),
    (L, torch.zeros(5, 7, dtype=torch.uint8), "other must be int16"),
    (np.zeros((5, 7), np.float64), O, "labels must be int16"),
    (L, np.zeros((5, 7), bool), "other must be int16"),
    ([[0] * 7] * 5, O, "labels must be a numpy array or a torch tensor"),
    (L, None, "other must be a numpy array or a torch tensor"),
    (torch.zeros(7, dtype=torch.int32), torch.zeros(7, dtype=torch.int32), r"labels must be \[H, W\]"),
    (torch.zeros(1, 2, 5, 7, dtype=torch.int32), O, r"labels must be \[H, W\]"),
    (L, torch.zeros(35, dtype=torch.int16), r"other must be \[H, W\]"),
    (torch.zeros(0, 7, dtype=torch.int32), torch.zeros(0, 7, dtype=torch.int32), "labels must not be empty"),
    (np.zeros((2, 5, 0), np.int16), np.zeros((2, 5, 0), np.int16), "labels must not be empty"),
    (L, np.zeros((0, 7), np.int16), "other must not be empty"),
    (L, torch.zeros(7, 5, dtype=torch.int16), "other must have shape"),
    (L, torch.zeros(1, 5, 7, dtype=torch.int16), "other must have shape"),
    (np.zeros((2, 5, 7), np.int64), np.zeros((3, 5, 7), np.int64), "other must have shape"),
])
def test_bad_maps(labels, other, match):
    for call in both(labels, other):
        with pytest.raises(ValueError, match=match):
            call()


@pytest.mark.parametrize("K", [0, -1, 65535, 1 << 20, 2.0, True, "4", None])
def test_bad_label_counts(K):
    with pytest.raises(ValueError, match="num_components"):
        label_overlap(L, O, K, 4)
    with pytest.raises(ValueError, match="num_other"):
        label_overlap(L, O, 4, K)
    with pytest.raises(ValueError, match="num_components"):                     # the first of the two is the first refused
        label_overlap(L, O, K, K)


@pytest.mark.parametrize("tolerance", [-1, 16, 100, 1.0, 0.5, True, False, "1", None])
def test_bad_tolerance(tolerance):
    with pytest.raises(ValueError, match="tolerance"):
        boundary_match(L, O, tolerance)


@pytest.mark.parametrize("cap", [0, 32, 1000, 1 << 32, 2048.0, True])
def test_bad_start_capacity(cap):
    with pytest.raises(ValueError, match="_start_capacity"):
        label_overlap(L, O, 4, 4, _start_capacity=cap)


class OnGpu(torch.Tensor):
    """A host tensor that says it lives on a GPU: what the device rules see of a device tensor (they run before any device work)."""
    index = 0
    device = property(lambda self: torch.device("cuda", self.index))


class OnGpu1(OnGpu):
    index = 1


def test_tensors_on_two_devices():
    a, b = L.as_subclass(OnGpu), O.as_subclass(OnGpu1)
    assert a.device == torch.device("cuda", 0) and b.device == torch.device("cuda", 1)
    for call in both(a, b) + both(a, O.numpy(), device="cuda:1") + both(L.numpy(), b, device=torch.device("cuda", 0)) \
            + both(a, O, device="cuda:1"):                                       # (two GPUs named: refused before the CPU tensor is)
        with pytest.raises(ValueError, match="must name one GPU"):
            call()


def test_cpu_tensors_are_refused_after_every_other_check():
    for call in both(L, O) + both(L, O.numpy()) + both(L, O.as_subclass(OnGpu), device="cuda:0"):
        with pytest.raises(ValueError, match="labels must be on a ROCm GPU"):
            call()
    for call in both(L.numpy(), O) + both(L.as_subclass(OnGpu), O):
        with pytest.raises(ValueError, match="other must be on a ROCm GPU"):
            call()
    for call in both(L.numpy(), O.numpy(), device="cpu"):
        with pytest.raises(ValueError, match="device must be a ROCm GPU"):
            call()
    with pytest.raises(ValueError, match="labels must be on a ROCm GPU"):
        label_overlap(torch.zeros(2, 5, 7, dtype=torch.int16), np.zeros((2, 5, 7), np.int64), 65534, 1, _start_capacity=64)
    with pytest.raises(ValueError, match="labels must be on a ROCm GPU"):
        boundary_match(L, O, 15)
    with pytest.raises(ValueError, match="num_other"):                          # any other error comes first
        label_overlap(L, O, 4, 0)
    with pytest.raises(ValueError, match="_start_capacity"):
        label_overlap(L, O, 4, 4, _start_capacity=100)
    with pytest.raises(ValueError, match="tolerance"):
        boundary_match(L, O, 16)


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
P = C.c_void_p(0x1000)
NUL = None


def lib():
    return B.load_library()


def accumulate_call(device=0, N=1, H=5, W=7, K=4, M=4, lab=P, ltype=0, oth=P, otype=2, cap=1024, ws=P, nbytes=1 << 30):
    return lib().fslic_hip_overlap_accumulate(device, NUL, N, H, W, K, M, lab, ltype, oth, otype, cap, ws, nbytes)


@pytest.mark.parametrize("kw", [
    dict(device=-1), dict(N=0), dict(N=-2), dict(H=0), dict(W=-3), dict(H=1 << 16, W=1 << 15), dict(K=0), dict(K=65535), dict(M=0),
    dict(M=65535), dict(M=-1), dict(ltype=3), dict(ltype=-1), dict(otype=3), dict(otype=-1), dict(lab=NUL), dict(oth=NUL), dict(ws=NUL),
    dict(cap=0), dict(cap=32), dict(cap=1000), dict(cap=1 << 32), dict(N=1 << 20, cap=1 << 20), dict(nbytes=32 + 1024 * 8 - 1),
    dict(N=5, nbytes=48 + 5 * 1024 * 8 - 1), dict(nbytes=0),
])
def test_capi_accumulate_refuses(kw):
    assert accumulate_call(**kw) == B.FSLIC_E_INVALID


def test_capi_workspace_size():
    n = C.c_size_t()
    assert lib().fslic_hip_overlap_workspace_size(1, 1024, C.byref(n)) == 0
    assert n.value == 32 + 1024 * 8                                        # header 16 + 4 N, rounded up to 16; keys and counts
    assert lib().fslic_hip_overlap_workspace_size(8, 32768, C.byref(n)) == 0
    assert n.value == 48 + 8 * 32768 * 8
    assert lib().fslic_hip_overlap_workspace_size(5, 64, C.byref(n)) == 0
    assert n.value == 48 + 5 * 64 * 8
    for args in [(0, 1024), (-1, 1024), (1, 1000), (1, 32), (1, 0), (1, 1 << 32), (1 << 20, 1 << 20)]:
        assert lib().fslic_hip_overlap_workspace_size(*args, C.byref(n)) == B.FSLIC_E_INVALID
    assert lib().fslic_hip_overlap_workspace_size(1, 1024, None) == B.FSLIC_E_INVALID
    assert accumulate_call(nbytes=32 + 1024 * 8 - 1) == B.FSLIC_E_INVALID
    assert b"workspace" in lib().fslic_hip_last_error()


@pytest.mark.parametrize("kw", [
    dict(device=-1), dict(N=0), dict(cap=1000), dict(cap=0), dict(cap=1 << 32), dict(ws=NUL), dict(keys=NUL), dict(count=NUL),
    dict(max_pairs=-1), dict(nbytes=32 + 1024 * 8 - 1),
])
def test_capi_compact_refuses(kw):
    a = dict(device=0, N=1, cap=1024, ws=P, nbytes=1 << 30, keys=P, count=P, max_pairs=10)
    a.update(kw)
    assert lib().fslic_hip_overlap_compact(a["device"], NUL, a["N"], a["cap"], a["ws"], a["nbytes"], a["keys"], a["count"],
                                           a["max_pairs"]) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", [
    dict(device=-1), dict(N=0), dict(H=0), dict(W=0), dict(H=-1), dict(H=1 << 16, W=1 << 15), dict(ltype=3), dict(ltype=-1), dict(otype=3),
    dict(otype=-1), dict(lab=NUL), dict(oth=NUL), dict(counts=NUL), dict(tolerance=-1), dict(tolerance=16),
])
def test_capi_boundary_match_refuses(kw):
    a = dict(device=0, N=1, H=5, W=7, lab=P, ltype=0, oth=P, otype=1, tolerance=0, counts=P)
    a.update(kw)
    assert lib().fslic_hip_boundary_match(a["device"], NUL, a["N"], a["H"], a["W"], a["lab"], a["ltype"], a["oth"], a["otype"],
                                          a["tolerance"], a["counts"]) == B.FSLIC_E_INVALID
