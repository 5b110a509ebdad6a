"""CPU tests of the connectivity pass on label tensors: the model (tests/connect_ref.py) against the reference's
ConnectivityEnforcer with the cut at K never binding, hand-written cases for each of the five rules, and the argument refusals of
fast_slic_amd/connect.py and of the C entries.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest
import torch

import connect_ref as R
from fast_slic_amd import _binding as B
from fast_slic_amd.connect import connected_components, enforce_connectivity
from oracle import oracle as orc


# ---- the model is the reference with K above the number of candidates ----
MAPS = [("blocky", 37, 53, 40), ("blocky", 64, 130, 300), ("noise", 33, 65, 3), ("noise", 50, 41, 2), ("blocky", 1, 77, 9), ("noise", 61, 1, 3)]


@pytest.mark.parametrize("kind,H,W,K", MAPS)
def test_model_equals_the_reference(kind, H, W, K):
    lab = (R.blocky if kind == "blocky" else R.noise)(H, W, K, seed=H * 1000 + W)
    comp, leaders, areas = R.components(lab)
    assert len(leaders) < 65535
    for thr in (0, 1, 2, 7, H * W + 1):
        out, n = R.enforce(lab, thr)
        ref = orc.enforce_connectivity(lab.astype(np.uint16), 65535, thr)
        assert np.array_equal(out, ref.astype(np.int32)), (kind, H, W, thr)
        assert n == max(int((areas >= thr).sum()), 1) and out.max() == n - 1
        assert np.array_equal(np.unique(out), np.arange(n))


def test_model_components_are_numbered_by_leader():
    lab = R.noise(23, 31, 3, seed=5)
    comp, leaders, areas = R.components(lab)
    flat = comp.reshape(-1)
    assert np.array_equal(flat[leaders], np.arange(len(leaders))) and np.all(np.diff(leaders) > 0)
    first = np.array([np.flatnonzero(flat == c)[0] for c in range(len(leaders))])
    assert np.array_equal(first, leaders)
    assert np.array_equal(np.bincount(flat), areas) and areas.sum() == lab.size
    assert len(np.unique(lab.reshape(-1)[leaders[comp]] - lab)) == 1          # a component holds one label


# ---- the rules by hand ----
def test_component_0_small_while_another_is_kept():
    lab = np.array([[5, 7, 7, 7],
                    [7, 7, 7, 7]])
    out, n = R.enforce(lab, 3)
    assert n == 1 and np.array_equal(out, np.zeros((2, 4), np.int32))            # rule 3: label 0, which is also the kept one's
    lab = np.array([[5, 7, 7, 9],
                    [7, 7, 9, 9]])
    out, n = R.enforce(lab, 3)
    assert n == 2 and np.array_equal(out, [[0, 0, 0, 1], [0, 0, 1, 1]])


def test_leader_in_column_0_adopts_from_above():
    lab = np.array([[1, 1, 2, 2],
                    [1, 1, 2, 2],
                    [3, 2, 2, 2]])
    out, n = R.enforce(lab, 2)
    assert n == 2 and np.array_equal(out, [[0, 0, 1, 1], [0, 0, 1, 1], [0, 1, 1, 1]])
    out, n = R.enforce(lab.T.copy(), 2)                                          # the leader (0, 2) adopts from its left
    assert np.array_equal(out, [[0, 0, 0], [0, 0, 1], [1, 1, 1], [1, 1, 1]])


def test_chain_of_three_unkept_components():
    lab = np.array([[1, 1, 1, 4, 5, 6, 2, 2, 2]])
    out, n = R.enforce(lab, 3)
    assert n == 2 and np.array_equal(out, [[0, 0, 0, 0, 0, 0, 1, 1, 1]])
    lab = np.array([[9, 1, 1, 1, 4, 5, 6]])                                      # ... that ends at the first kept component, label 0
    out, n = R.enforce(lab, 3)
    assert n == 1 and np.array_equal(out, np.zeros((1, 7), np.int32))


def test_no_component_kept():
    lab = R.noise(9, 11, 3, seed=1)
    out, n = R.enforce(lab, 9 * 11 + 1)
    assert n == 1 and not out.any()
    comp, leaders, _ = R.components(lab)
    assert comp.max() + 1 == len(leaders)


def test_minus_one_is_a_label_like_any_other():
    lab = np.array([[-1, -1, 3], [3, -1, 3]], np.int16)
    comp, leaders, areas = R.components(lab)
    assert np.array_equal(comp, [[0, 0, 1], [2, 0, 1]]) and list(areas) == [3, 2, 1]
    assert np.array_equal(R.enforce(lab, 2)[0], [[0, 0, 1], [0, 0, 1]])


# ---- connect.py refuses before any device work ----
@pytest.mark.parametrize("f", [connected_components, lambda l, **k: enforce_connectivity(l, 4, **k)])
def test_python_refuses_bad_maps(f):
    good = np.zeros((4, 5), np.int32)
    for bad in (None, [[1, 2]], good.astype(np.float32), good.astype(np.uint8), np.zeros((5,), np.int32), np.zeros((1, 1, 4, 5), np.int32),
                np.zeros((0, 5), np.int32), torch.zeros((4, 5), dtype=torch.float32), torch.zeros((4, 5), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            f(bad)
    with pytest.raises(ValueError, match="no CPU fallback"):
        f(torch.zeros((4, 5), dtype=torch.int32))
    with pytest.raises(ValueError, match="ROCm GPU"):
        f(good, device="cpu")
    with pytest.raises(ValueError, match="2\\^31"):                              # (never touched: a broadcast view of one element)
        f(np.broadcast_to(np.zeros((), np.int16), (1 << 11, 1 << 10, 1 << 10)))


def test_python_refuses_bad_min_size():
    good = np.zeros((4, 5), np.int32)
    for bad in (True, False, 2.0, -1, "3", None, np.float32(2)):
        with pytest.raises(ValueError, match="min_size"):
            enforce_connectivity(good, bad)
    with pytest.raises(TypeError):
        enforce_connectivity(good)


# ---- the C entries refuse before the first HIP call ----
def _entries():
    lib = B.load_library()
    assert hasattr(lib, "fslic_hip_connect_enforce")
    return lib


def test_header_exports_and_library_agree_on_the_names():
    names = ["fslic_hip_connect_workspace_size", "fslic_hip_connected_components", "fslic_hip_connect_enforce"]
    lib = _entries()
    assert sorted(n for n in B.EXPORTS if "_connect" in n and "connectivity" not in n) == sorted(names)
    for n in names:
        assert hasattr(lib, n)


def test_workspace_size():
    lib = _entries()
    nbytes = C.c_size_t()
    assert lib.fslic_hip_connect_workspace_size(8, 720, 1280, C.byref(nbytes)) == 0
    assert nbytes.value == 8 * 720 * 1280 * 8 + 8 * 900 * 4                      # 8 bytes per pixel, 4 per 1024 pixels of a frame
    assert lib.fslic_hip_connect_workspace_size(3, 1, 1, C.byref(nbytes)) == 0 and nbytes.value == 16 + 16 + 16
    for N, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 1 << 16, 1 << 15), (2, 1 << 15, 1 << 15), (1 << 11, 1 << 10, 1 << 10)):
        assert lib.fslic_hip_connect_workspace_size(N, H, W, C.byref(nbytes)) == B.FSLIC_E_INVALID, (N, H, W)
    assert lib.fslic_hip_connect_workspace_size(1, 4, 4, None) == B.FSLIC_E_INVALID


def test_c_entries_refuse_bad_arguments():
    lib = _entries()
    p = C.c_void_p(4096)                                                         # never dereferenced: every call is refused first
    big = 1 << 40

    def comp(device=0, N=1, H=4, W=4, labels=p, ltype=1, out=p, counts=p, ws=p, wsb=big):
        return lib.fslic_hip_connected_components(device, None, N, H, W, labels, ltype, out, counts, ws, wsb)

    def enf(device=0, N=1, H=4, W=4, labels=p, ltype=1, min_size=2, out=p, counts=p, ws=p, wsb=big):
        return lib.fslic_hip_connect_enforce(device, None, N, H, W, labels, ltype, min_size, out, counts, ws, wsb)

    for f in (comp, enf):
        for kw in (dict(device=-1), dict(N=0), dict(H=0), dict(W=-3), dict(labels=None), dict(out=None), dict(counts=None), dict(ws=None),
                   dict(ltype=3), dict(ltype=-1), dict(H=1 << 16, W=1 << 15), dict(N=2, H=1 << 15, W=1 << 15), dict(N=1 << 21, H=32, W=32),
                   dict(wsb=4 * 4 * 8 + 16 - 1), dict(wsb=0)):
            assert f(**kw) == B.FSLIC_E_INVALID, (f.__name__, kw)
    assert enf(min_size=-1) == B.FSLIC_E_INVALID
    assert enf(wsb=4 * 4 * 8 + 16 - 1) == B.FSLIC_E_INVALID and b"workspace too small: 144 bytes" in lib.fslic_hip_last_error()
    with pytest.raises(ValueError, match="label type"):
        B._check(comp(ltype=7))
