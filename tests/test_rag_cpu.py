"""CPU tests of the region adjacency graph (fast_slic_amd/rag.py, the fslic_hip_rag* entries): the numpy reference (tests/rag_ref.py)
on maps small enough to check by hand, and every argument error refused before any device work -- ValueError in Python,
FSLIC_E_INVALID from the C ABI before its first HIP call.  No kernel is launched here."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import torch

import rag_ref as R
from fast_slic_amd import _binding as B
from fast_slic_amd.rag import capacity_limit, first_capacity, superpixel_graph

L = torch.zeros(5, 7, dtype=torch.int32)
IMG = torch.zeros(5, 7, 3, dtype=torch.uint8)


def test_package_import_stays_torch_free():
    code = "import sys, fast_slic_amd; assert 'torch' not in sys.modules; import fast_slic_amd.rag; assert 'torch' in sys.modules"
    subprocess.check_call([sys.executable, "-c", code])


# ---- the reference, by hand ----
def edges_of(labels, K, connectivity, image=None):
    e, b, c = R.graph_frame(np.asarray(labels), K, connectivity, image)
    return [tuple(r) for r in e.tolist()], b.tolist(), c


def test_reference_four_pixels():
    lab = [[0, 1], [2, 3]]
    e, b, _ = edges_of(lab, 4, 4)
    assert e == [(0, 1), (0, 2), (1, 3), (2, 3)] and b == [1, 1, 1, 1]
    e, b, _ = edges_of(lab, 4, 8)
    assert e == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] and b == [1] * 6


@pytest.mark.parametrize("H,W", [(1, 2), (4, 6), (7, 10)])
def test_reference_two_halves(H, W):
    lab = np.zeros((H, W), np.int16)
    lab[:, W // 2:] = 1
    assert edges_of(lab, 2, 4)[:2] == ([(0, 1)], [H])
    assert edges_of(lab, 2, 8)[:2] == ([(0, 1)], [3 * H - 2])            # H across, H - 1 on either diagonal
    assert edges_of(lab.T.copy(), 2, 8)[:2] == ([(0, 1)], [3 * H - 2])


def test_reference_labels_outside_the_range():
    lab = np.array([[0, -1, 1],
                    [0, 7, 1],
                    [2, 2, 1]], np.int16)
    # K = 3: -1 and 7 are no labels.  4-connectivity: 0|2 (down, once), 2|1 (right, once); 0 and 1 never touch
    e, b, _ = edges_of(lab, 3, 4)
    assert e == [(0, 2), (1, 2)] and b == [1, 1]
    # 8-connectivity adds 0(1,0)-2(2,1) and 1(1,2)-2(2,1); no pair through the two holes
    e, b, _ = edges_of(lab, 3, 8)
    assert e == [(0, 2), (1, 2)] and b == [2, 2]
    assert edges_of(lab.view(np.uint16), 3, 8)[:2] == (e, b)             # the uint16 view of the int16 map: 0xFFFF is no label
    e, b, _ = edges_of(lab, 8, 4)                                         # K = 8: label 7 takes part
    assert e == [(0, 2), (0, 7), (1, 2), (1, 7), (2, 7)] and b == [1] * 5


def test_reference_contrast_and_batch():
    lab = np.array([[0, 0, 1], [0, 1, 1]], np.int32)
    img = np.array([[[10, 0], [20, 5], [50, 5]], [[0, 0], [100, 255], [7, 9]]], np.uint8)
    e, b, c = edges_of(lab, 2, 4, img)
    # pixel pairs across the boundary: (0,1)|(0,2): |20-50|, |5-5|; (1,0)|(1,1): |0-100|, |0-255|; (0,1)|(1,1): |20-100|, |5-255|
    assert e == [(0, 1)] and b == [3] and c.tolist() == [[30 + 100 + 80, 0 + 255 + 250]]
    e, b, c = edges_of(lab, 2, 8, img)
    # and the diagonals (0,0)|(1,1): 90, 255; (0,2)|(1,1) is 1|1; (0,1)|(1,2): |20-7|, |5-9|; (0,1)|(1,0) is 0|0
    assert b == [5] and c.tolist() == [[210 + 90 + 13, 505 + 255 + 4]]
    g = R.graph(np.stack([lab, 1 - lab, np.zeros_like(lab)]), 2, 4, np.stack([img, img, img]))
    assert g["offsets"].tolist() == [0, 1, 2, 2] and g["edge_index"].tolist() == [[0, 0], [1, 1]]
    assert g["boundary"].tolist() == [3, 3] and g["contrast"].tolist() == [[210, 505], [210, 505]]


def test_capacities():
    assert first_capacity(1) == 1024 and first_capacity(128) == 1024 and first_capacity(129) == 2048 and first_capacity(1600) == 16384
    assert capacity_limit(1600, 720, 1280, 4) == 1 << 22                 # 2 * 1600 * 1599 / 2 = 2 558 400 label pairs
    assert capacity_limit(1024, 96, 96, 8) == 1 << 17                    # 2 * 4 * 96 * 96 = 73 728 pixel pairs
    assert capacity_limit(2, 4000, 4000, 8) == 1024
    assert capacity_limit(65534, 20000, 20000, 8) == 1 << 31


# ---- argument errors of superpixel_graph: all before any device work (a CPU tensor is the last thing refused) ----
@pytest.mark.parametrize("labels,match", [
    (torch.zeros(5, 7, dtype=torch.float32), "int16"),
    (torch.zeros(5, 7, dtype=torch.uint8), "int16"),
    (np.zeros((5, 7), np.float64), "int16"),
    ([[0] * 7] * 5, "numpy array or a torch tensor"),
    (torch.zeros(7, dtype=torch.int32), r"\[H, W\]"),
    (torch.zeros(1, 2, 5, 7, dtype=torch.int32), r"\[H, W\]"),
    (torch.zeros(0, 7, dtype=torch.int32), "empty"),
    (np.zeros((2, 5, 0), np.int16), "empty"),
])
def test_bad_labels(labels, match):
    with pytest.raises(ValueError, match=match):
        superpixel_graph(labels, 4)


@pytest.mark.parametrize("K", [0, -1, 65535, 1 << 20, 2.0, True, "4"])
def test_bad_num_components(K):
    with pytest.raises(ValueError, match="num_components"):
        superpixel_graph(L, K)


@pytest.mark.parametrize("connectivity", [0, 6, 2, "8", None, 4.5, True])
def test_bad_connectivity(connectivity):
    with pytest.raises(ValueError, match="connectivity"):
        superpixel_graph(L, 4, connectivity=connectivity)


@pytest.mark.parametrize("image,match", [
    (torch.zeros(5, 7, 3), "uint8"),
    (np.zeros((5, 7, 3), np.int8), "uint8"),
    ([[[0] * 3] * 7] * 5, "numpy array or a torch tensor"),
    (torch.zeros(5, 7, dtype=torch.uint8), "shape"),
    (torch.zeros(3, 5, 7, dtype=torch.uint8), "shape"),
    (torch.zeros(5, 6, 3, dtype=torch.uint8), "shape"),
    (torch.zeros(1, 5, 7, 3, dtype=torch.uint8), "shape"),
    (torch.zeros(5, 7, 5, dtype=torch.uint8), "channels"),
    (np.zeros((5, 7, 0), np.uint8), "channels"),
])
def test_bad_image(image, match):
    with pytest.raises(ValueError, match=match):
        superpixel_graph(L, 4, image=image)


@pytest.mark.parametrize("cap", [0, 32, 1000, 1 << 32, 2048.0, True])
def test_bad_start_capacity(cap):
    with pytest.raises(ValueError, match="_start_capacity"):
        superpixel_graph(L, 4, _start_capacity=cap)


def test_cpu_tensors_are_refused_after_every_other_check():
    with pytest.raises(ValueError, match="labels must be on a ROCm GPU"):
        superpixel_graph(L, 4)
    with pytest.raises(ValueError, match="labels must be on a ROCm GPU"):
        superpixel_graph(torch.zeros(2, 5, 7, dtype=torch.int16), 65534, connectivity=8, image=np.zeros((2, 5, 7, 4), np.uint8))
    with pytest.raises(ValueError, match="image must be on a ROCm GPU"):
        superpixel_graph(L.numpy(), 4, image=IMG)
    with pytest.raises(ValueError, match="device must be a ROCm GPU"):
        superpixel_graph(L.numpy(), 4, device="cpu")


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
P = C.c_void_p(0x1000)
NUL = None


def lib():
    return B.load_library()


def accumulate_call(device=0, N=1, H=5, W=7, K=4, conn=4, lab=P, ltype=0, img=NUL, Cc=0, cap=1024, ws=P, nbytes=1 << 30):
    return lib().fslic_hip_rag_accumulate(device, NUL, N, H, W, K, conn, lab, ltype, img, Cc, cap, ws, nbytes)


@pytest.mark.parametrize("kw", [
    dict(device=-1), dict(N=0), dict(H=0), dict(W=-3), dict(H=1 << 15, W=1 << 14), dict(K=0), dict(K=65535), dict(conn=6), dict(conn=0),
    dict(ltype=3), dict(ltype=-1), dict(lab=NUL), dict(ws=NUL), dict(img=P, Cc=0), dict(img=NUL, Cc=3), dict(img=P, Cc=5), dict(Cc=-1),
    dict(cap=0), dict(cap=32), dict(cap=1000), dict(cap=1 << 32), dict(nbytes=32 + 1024 * 8 - 1), dict(img=P, Cc=2, nbytes=32 + 1024 * 24 - 1),
])
def test_capi_accumulate_refuses(kw):
    assert accumulate_call(**kw) == B.FSLIC_E_INVALID


def test_capi_workspace_size():
    n = C.c_size_t()
    assert lib().fslic_hip_rag_workspace_size(1, 4, 0, 1024, C.byref(n)) == 0
    assert n.value == 32 + 1024 * 8                                        # header 16 + 4 N, rounded up to 16
    assert lib().fslic_hip_rag_workspace_size(8, 1600, 3, 16384, C.byref(n)) == 0
    assert n.value == 48 + 8 * 16384 * (8 + 8 * 3)
    assert lib().fslic_hip_rag_workspace_size(5, 1600, 4, 64, C.byref(n)) == 0
    assert n.value == 48 + 5 * 64 * 40
    for args in [(0, 4, 0, 1024), (1, 0, 0, 1024), (1, 65535, 0, 1024), (1, 4, 5, 1024), (1, 4, -1, 1024), (1, 4, 0, 1000), (1, 4, 0, 32),
                 (1, 4, 0, 1 << 32), (1 << 20, 4, 0, 1 << 20)]:
        assert lib().fslic_hip_rag_workspace_size(*args, C.byref(n)) == B.FSLIC_E_INVALID
    assert lib().fslic_hip_rag_workspace_size(1, 4, 0, 1024, None) == B.FSLIC_E_INVALID
    assert accumulate_call(nbytes=32 + 1024 * 8 - 1) == B.FSLIC_E_INVALID
    assert b"workspace" in lib().fslic_hip_last_error()


@pytest.mark.parametrize("kw", [
    dict(device=-1), dict(N=0), dict(Cc=5), dict(Cc=-1), dict(cap=1000), dict(cap=0), dict(ws=NUL), dict(keys=NUL), dict(boundary=NUL),
    dict(contrast=P, Cc=0), dict(max_edges=-1), dict(nbytes=32 + 1024 * 8 - 1),
])
def test_capi_compact_refuses(kw):
    a = dict(device=0, N=1, Cc=0, cap=1024, ws=P, nbytes=1 << 30, keys=P, boundary=P, contrast=NUL, max_edges=10)
    a.update(kw)
    assert lib().fslic_hip_rag_compact(a["device"], NUL, a["N"], a["Cc"], a["cap"], a["ws"], a["nbytes"], a["keys"], a["boundary"],
                                       a["contrast"], a["max_edges"]) == B.FSLIC_E_INVALID
