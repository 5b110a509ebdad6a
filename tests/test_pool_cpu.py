"""CPU tests of superpixel pooling (fast_slic_amd/pool.py, the fslic_hip_pool* entries): every argument error is refused before any
device work -- ValueError in Python, FSLIC_E_INVALID from the C ABI before its first HIP call.  No kernel is launched here."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import torch

from fast_slic_amd import _binding as B
from fast_slic_amd.pool import superpixel_pool, superpixel_unpool

F = torch.zeros(3, 5, 7)
L = torch.zeros(5, 7, dtype=torch.int32)


def test_package_import_stays_torch_free():
    code = "import sys, fast_slic_amd; assert 'torch' not in sys.modules; import fast_slic_amd.pool; assert 'torch' in sys.modules"
    subprocess.check_call([sys.executable, "-c", code])


@pytest.mark.parametrize("features,labels,match", [
    (F.double(), L, "float32"),
    (F.half(), L, "float32"),
    (F.numpy(), L, "torch tensor"),
    (torch.zeros(5, 7), L, r"\[C, H, W\]"),
    (torch.zeros(1, 1, 3, 5, 7), L, r"\[C, H, W\]"),
    (torch.zeros(0, 5, 7), L, "empty"),
    (F, torch.zeros(5, 7, dtype=torch.float32), "int16"),
    (F, torch.zeros(5, 7, dtype=torch.uint8), "int16"),
    (F, np.zeros((5, 7), np.float64), "int16"),
    (F, [[0] * 7] * 5, "numpy array or a torch tensor"),
    (F, torch.zeros(5, 6, dtype=torch.int32), "shape"),
    (F, torch.zeros(1, 5, 7, dtype=torch.int32), "shape"),
    (torch.zeros(2, 3, 5, 7), torch.zeros(3, 5, 7, dtype=torch.int32), "shape"),
    (torch.zeros(2, 3, 5, 7), torch.zeros(5, 7, dtype=torch.int32), "shape"),
])
def test_bad_features_or_labels(features, labels, match):
    with pytest.raises(ValueError, match=match):
        superpixel_pool(features, labels, 4)


@pytest.mark.parametrize("K", [0, -1, 65535, 1 << 20, 2.0, True, "4"])
def test_bad_num_components(K):
    with pytest.raises(ValueError, match="num_components"):
        superpixel_pool(F, L, K)


@pytest.mark.parametrize("reduce", ["min", "avg", None, "MEAN"])
def test_bad_reduce(reduce):
    with pytest.raises(ValueError, match="reduce"):
        superpixel_pool(F, L, 4, reduce=reduce)


def test_cpu_features_are_refused_after_every_other_check():
    with pytest.raises(ValueError, match="ROCm GPU"):
        superpixel_pool(F, L, 4)
    with pytest.raises(ValueError, match="ROCm GPU"):
        superpixel_pool(F, L.numpy().astype(np.int16), 65534, reduce="max", return_counts=True)
    with pytest.raises(ValueError, match="ROCm GPU"):
        superpixel_unpool(torch.zeros(3, 4), L, fill=-1.0)


@pytest.mark.parametrize("values,labels,fill,match", [
    (torch.zeros(3, 4, dtype=torch.float64), L, 0.0, "float32"),
    (torch.zeros(4), L, 0.0, r"\[C, K\]"),
    (torch.zeros(3, 4), torch.zeros(2, 5, 7, dtype=torch.int32), 0.0, r"\[H, W\]"),
    (torch.zeros(2, 3, 4), torch.zeros(3, 5, 7, dtype=torch.int32), 0.0, "shape"),
    (torch.zeros(3, 4), torch.zeros(5, 7, dtype=torch.float32), 0.0, "int16"),
    (torch.zeros(3, 65535), L, 0.0, "num_components"),
    (torch.zeros(3, 4), L, "x", "fill"),
    (torch.zeros(3, 4), L, None, "fill"),
])
def test_bad_unpool_arguments(values, labels, fill, match):
    with pytest.raises(ValueError, match=match):
        superpixel_unpool(values, labels, fill=fill)


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
P = C.c_void_p(0x1000)
NUL = None


def lib():
    return B.load_library()


def pool_call(device=0, N=1, Cc=3, H=5, W=7, K=4, reduce=0, feat=P, lab=P, ltype=0, ws=P, nbytes=1 << 20):
    return lib().fslic_hip_pool(device, NUL, N, Cc, H, W, K, reduce, feat, lab, ltype, ws, nbytes)


@pytest.mark.parametrize("kw", [
    dict(device=-1), dict(N=0), dict(Cc=0), dict(H=0), dict(W=-3), dict(H=1 << 16, W=1 << 15), dict(K=0), dict(K=65535),
    dict(reduce=3), dict(reduce=-1), dict(ltype=3), dict(feat=NUL), dict(lab=NUL), dict(ws=NUL), dict(nbytes=3 * 4 * 56),
])
def test_capi_pool_refuses(kw):
    assert pool_call(**kw) == B.FSLIC_E_INVALID


def test_capi_workspace_size():
    n = C.c_size_t()
    assert lib().fslic_hip_pool_workspace_size(8, 21, 1600, 1, C.byref(n)) == 0
    assert n.value == 8 * 21 * 1600 * 56 + 8 * 1600 * 4
    assert lib().fslic_hip_pool_workspace_size(2, 3, 5, 2, C.byref(n)) == 0
    assert n.value == 2 * 3 * 5 * 8 + 40
    assert lib().fslic_hip_pool_workspace_size(1, 1, 3, 0, C.byref(n)) == 0
    assert n.value == 56 * 3 + 16                                     # counts padded to 8 bytes
    for args in [(0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, 65535, 0), (1, 1, 1, 5)]:
        assert lib().fslic_hip_pool_workspace_size(*args, C.byref(n)) == B.FSLIC_E_INVALID
    assert lib().fslic_hip_pool_workspace_size(1, 1, 1, 0, None) == B.FSLIC_E_INVALID
    # one byte short is refused by pool and finalize
    need = 3 * 4 * 56 + 16
    assert pool_call(nbytes=need - 1) == B.FSLIC_E_INVALID
    assert b"workspace" in lib().fslic_hip_last_error()


@pytest.mark.parametrize("args", [
    (-1, NUL, 1, 3, 4, 0, P, 1 << 20, P, P, NUL), (0, NUL, 0, 3, 4, 0, P, 1 << 20, P, P, NUL), (0, NUL, 1, 3, 0, 0, P, 1 << 20, P, P, NUL),
    (0, NUL, 1, 3, 4, 7, P, 1 << 20, P, P, NUL), (0, NUL, 1, 3, 4, 0, NUL, 1 << 20, P, P, NUL), (0, NUL, 1, 3, 4, 0, P, 1 << 20, NUL, P, NUL),
    (0, NUL, 1, 3, 4, 0, P, 8, P, P, NUL), (0, NUL, 1, 3, 4, 1, P, 1 << 20, P, P, P),     # argmax without max
])
def test_capi_finalize_refuses(args):
    assert lib().fslic_hip_pool_finalize(*args) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", [
    dict(device=-1), dict(N=0), dict(Cc=0), dict(H=0), dict(W=0), dict(K=0), dict(K=70000), dict(ltype=-1), dict(values=NUL),
    dict(lab=NUL), dict(out=NUL),
])
def test_capi_unpool_refuses(kw):
    a = dict(device=0, N=1, Cc=3, H=5, W=7, K=4, values=P, lab=P, ltype=1, argmax=NUL, fill=0.0, out=P)
    a.update(kw)
    assert lib().fslic_hip_unpool(a["device"], NUL, a["N"], a["Cc"], a["H"], a["W"], a["K"], a["values"], a["lab"], a["ltype"],
                                  a["argmax"], a["fill"], a["out"]) == B.FSLIC_E_INVALID
