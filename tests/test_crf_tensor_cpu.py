"""CPU tests of SimpleCRF inference on torch tensors (fast_slic_amd/crf_torch.py, the fslic_hip_crf_tensor_* entries): every argument
error refused before any device work -- ValueError in Python, FSLIC_E_INVALID from the C ABI before its first HIP call -- the
workspace size, and SuperpixelGraph.to_batch_csr on hand-built graphs (plain torch, so it runs on CPU tensors).  No kernel is launched
here."""
import ctypes as C
import subprocess
import sys

import pytest
import torch

from fast_slic_amd import _binding as B
from fast_slic_amd.crf_torch import DEFAULT_PARAMS, superpixel_crf
from fast_slic_amd.rag import SuperpixelGraph

CN, K = 3, 4
U = torch.zeros(CN, K)
YX = torch.zeros(5, K)
MEM = torch.ones(K, dtype=torch.int32)
OFF = torch.zeros(K + 1, dtype=torch.int64)
IDX = torch.zeros(0, dtype=torch.int32)


def call(unaries=U, graph=(OFF, IDX), yxrgb=YX, members=MEM, **kw):
    return superpixel_crf(unaries, graph, yxrgb, members, **kw)


def test_package_import_stays_torch_free():
    code = "import sys, fast_slic_amd; assert 'torch' not in sys.modules; import fast_slic_amd.crf_torch; assert 'torch' in sys.modules"
    subprocess.check_call([sys.executable, "-c", code])


def test_defaults_are_a_fresh_simple_crf():
    from fast_slic_amd.crf import SimpleCRF
    crf = SimpleCRF(CN, K)
    assert {n: getattr(crf, n) for n in DEFAULT_PARAMS} == DEFAULT_PARAMS
    assert [crf.get_compat(c) for c in range(CN)] == [1.0] * CN


# ---- argument errors of superpixel_crf: all before any device work (a CPU tensor is the last thing refused) ----
@pytest.mark.parametrize("kw,match", [
    (dict(unaries=U.double()), "unaries must be float32"),
    (dict(unaries=U.numpy()), "unaries must be a torch tensor"),
    (dict(unaries=torch.zeros(K)), r"\[C, K\] or \[N, C, K\]"),
    (dict(unaries=torch.zeros(1, 2, CN, K)), r"\[C, K\] or \[N, C, K\]"),
    (dict(unaries=torch.zeros(CN, 0)), "empty"),
    (dict(yxrgb=YX.double()), "yxrgb must be float32"),
    (dict(yxrgb=YX.numpy()), "yxrgb must be a torch tensor"),
    (dict(yxrgb=torch.zeros(6, K)), "yxrgb must have shape"),
    (dict(yxrgb=torch.zeros(K, 5)), "yxrgb must have shape"),
    (dict(yxrgb=torch.zeros(1, 5, K)), "yxrgb must have shape"),
    (dict(yxrgb=torch.zeros(5, K + 1)), "yxrgb must have shape"),
    (dict(members=MEM.long()), "members must be int32"),
    (dict(members=MEM.float()), "members must be int32"),
    (dict(members=torch.ones(K + 1, dtype=torch.int32)), "members must have shape"),
    (dict(members=torch.ones(1, K, dtype=torch.int32)), "members must have shape"),
    (dict(q0=U.double()), "q0 must be float32"),
    (dict(q0=torch.zeros(CN, K + 1)), "q0 must have shape"),
    (dict(q0=torch.zeros(1, CN, K)), "q0 must have shape"),
    (dict(q0=[[0.0] * K] * CN), "q0 must be a torch tensor"),
    (dict(unaries=torch.zeros(2, CN, K)), "yxrgb must have shape"),                       # a batch needs batched clusters
    (dict(unaries=torch.zeros(2, CN, K), yxrgb=torch.zeros(2, 5, K)), "members must have shape"),
    (dict(graph=None), "SuperpixelGraph or a pair"),
    (dict(graph=(OFF,)), "SuperpixelGraph or a pair"),
    (dict(graph=(OFF.numpy(), IDX)), "must be torch tensors"),
    (dict(graph=(OFF.int(), IDX)), "offsets must be int64"),
    (dict(graph=(OFF, IDX.long())), "indices must be int32"),
    (dict(graph=(OFF[:-1], IDX)), "offsets must have shape"),
    (dict(graph=(torch.zeros(K + 2, dtype=torch.int64), IDX)), "offsets must have shape"),
    (dict(graph=(OFF.reshape(1, -1), IDX)), "offsets must have shape"),
    (dict(graph=(OFF, IDX.reshape(0, 1))), "indices must be one-dimensional"),
    (dict(max_iter=-1), "max_iter"),
    (dict(max_iter=2.0), "max_iter"),
    (dict(max_iter=True), "max_iter"),
    (dict(max_iter="3"), "max_iter"),
    (dict(max_iter=None), "max_iter"),
    (dict(max_iter=1 << 31), "max_iter"),
    (dict(params=dict(spatial_v=1.0)), "unknown params name 'spatial_v'"),
    (dict(params=dict(spatial_w="1")), "real number"),
    (dict(params=[10.0] * 7), "params must be None or a dict"),
    (dict(compat=[1.0] * (CN + 1)), "one value per class"),
    (dict(compat=[]), "one value per class"),
    (dict(compat=torch.ones(CN + 1)), "compat must have shape"),
    (dict(compat=torch.ones(CN, dtype=torch.float64)), "compat must be float32"),
    (dict(compat=["a"] * CN), "real numbers"),
    (dict(compat=1.0), "compat must be None, a sequence"),
    (dict(temporal=1), "temporal"),
    (dict(temporal=None), "temporal"),
])
def test_bad_arguments(kw, match):
    with pytest.raises(ValueError, match=match):
        call(**kw)


def test_graph_object_must_match_the_unaries():
    def graph(N, k):
        return SuperpixelGraph(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None,
                               torch.zeros(N + 1, dtype=torch.int64), k, 1024)
    with pytest.raises(ValueError, match="graph has 1 frames of 5 nodes"):
        call(graph=graph(1, K + 1))
    with pytest.raises(ValueError, match="graph has 2 frames of 4 nodes"):
        call(graph=graph(2, K))
    with pytest.raises(ValueError, match="unaries must be on a ROCm GPU"):
        call(graph=graph(1, K))


def test_sizes_of_2_to_the_31_are_refused():
    big = torch.zeros(1).expand(1 << 11, 1 << 10, 1 << 10)                  # N * C * K = 2^31, one float of storage
    with pytest.raises(ValueError, match="below 2\\^31"):
        superpixel_crf(big, (torch.zeros(1, dtype=torch.int64).expand((1 << 21) + 1), IDX), torch.zeros(1).expand(1 << 11, 5, 1 << 10),
                       torch.zeros(1, dtype=torch.int32).expand(1 << 11, 1 << 10))
    with pytest.raises(ValueError, match="below 2\\^31"):
        call(graph=(OFF, torch.zeros(1, dtype=torch.int32).expand(1 << 31)))


def test_cpu_tensors_are_refused_after_every_other_check():
    with pytest.raises(ValueError, match="unaries must be on a ROCm GPU"):
        call()
    with pytest.raises(ValueError, match="unaries must be on a ROCm GPU"):
        call(unaries=torch.zeros(2, CN, K), yxrgb=torch.zeros(2, 5, K), members=torch.ones(2, K, dtype=torch.int32),
             graph=(torch.zeros(2 * K + 1, dtype=torch.int64), torch.zeros(7, dtype=torch.int32)), max_iter=0, temporal=True,
             params=dict(DEFAULT_PARAMS), compat=[1.0, 2, 0.5], q0=torch.zeros(2, CN, K))


# ---- SuperpixelGraph.to_batch_csr on CPU tensors ----
def hand_graph():
    # frame 0: 0-1, 0-2, 1-2; frame 1: nothing; frame 2: 1-3
    edge_index = torch.tensor([[0, 0, 1, 1], [1, 2, 2, 3]], dtype=torch.int64)
    return SuperpixelGraph(edge_index, torch.ones(4, dtype=torch.int32), None, torch.tensor([0, 3, 3, 4]), K, 1024)


def test_to_batch_csr_by_hand():
    off, idx = hand_graph().to_batch_csr()
    assert off.dtype == torch.int64 and idx.dtype == torch.int32
    assert off.tolist() == [0, 2, 4, 6, 6, 6, 6, 6, 6, 6, 7, 7, 8]
    assert idx.tolist() == [1, 2, 0, 2, 0, 1, 3, 1]


def test_to_batch_csr_is_the_concatenation_of_to_csr():
    g = hand_graph()
    off, idx = g.to_batch_csr()
    offs, idxs, shift = [torch.zeros(1, dtype=torch.int64)], [], 0
    for n in range(g.num_frames):
        o, i = g.to_csr(n)
        offs.append(o[1:] + shift)
        idxs.append(i)
        shift += int(o[-1])
    assert torch.equal(off, torch.cat(offs)) and torch.equal(idx, torch.cat(idxs))
    empty = SuperpixelGraph(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), None,
                            torch.zeros(3, dtype=torch.int64), K, 1024)
    off, idx = empty.to_batch_csr()
    assert off.tolist() == [0] * (2 * K + 1) and idx.shape == (0,) and idx.dtype == torch.int32


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
P = C.c_void_p(0x1000)
NUL = None
PARAMS = (C.c_float * 7)(10, 10, 13, 13, 80, 0, 3)


def lib():
    return B.load_library()


def workspace_size(N, Cn, k, nnz):
    n = C.c_size_t()
    assert lib().fslic_hip_crf_tensor_workspace_size(N, Cn, k, nnz, C.byref(n)) == 0
    return n.value


def inference_call(**kw):
    a = dict(device=0, N=2, Cn=3, k=70, temporal=1, max_iter=3, params=C.cast(PARAMS, C.c_void_p), compat=P, yxrgb=P, members=P,
             offsets=P, indices=P, nnz=100, unaries=P, q0=NUL, q_out=P, ws=P, nbytes=1 << 40)
    a.update(kw)
    return lib().fslic_hip_crf_tensor_inference(a["device"], NUL, a["N"], a["Cn"], a["k"], a["temporal"], a["max_iter"], a["params"],
                                                a["compat"], a["yxrgb"], a["members"], a["offsets"], a["indices"], a["nnz"],
                                                a["unaries"], a["q0"], a["q_out"], a["ws"], a["nbytes"])


@pytest.mark.parametrize("kw", [
    dict(device=-1), dict(N=0), dict(N=-2), dict(Cn=0), dict(k=0), dict(k=-1), dict(temporal=2), dict(temporal=-1), dict(max_iter=-1),
    dict(nnz=-1), dict(nnz=1 << 31), dict(N=1 << 11, Cn=1 << 10, k=1 << 10), dict(N=1 << 16, Cn=1, k=1 << 15), dict(N=(1 << 31) - 1, Cn=1, k=1),
    dict(params=NUL), dict(compat=NUL), dict(yxrgb=NUL), dict(members=NUL), dict(offsets=NUL), dict(indices=NUL), dict(unaries=NUL),
    dict(q_out=NUL), dict(ws=NUL), dict(ws=C.c_void_p(0x1008)), dict(nbytes=0), dict(nbytes=2 * 70 * 24 + 800 + 2 * 3 * 70 * 4 - 1),
])
def test_capi_inference_refuses(kw):
    assert inference_call(**kw) == B.FSLIC_E_INVALID


def test_capi_workspace_size():
    n = C.c_size_t()
    # rows 8 B + temporal 16 B a node, 8 B an entry, one q buffer; every part rounded up to 16
    assert workspace_size(2, 3, 70, 100) == 2 * 70 * 24 + 800 + 2 * 3 * 70 * 4
    assert workspace_size(1, 1, 1, 0) == 16 + 16 + 0 + 16
    assert workspace_size(1, 128, 70, 3) == 70 * 24 + 32 + 128 * 70 * 4
    assert workspace_size(1, 129, 70, 3) == 70 * 24 + 32 + 2 * (129 * 70 * 4 + 8)          # the message plane above 128 classes
    assert workspace_size(8, 21, 1600, 8 * 9200) == 8 * 1600 * 24 + 8 * 9200 * 8 + 8 * 21 * 1600 * 4
    for args in [(0, 3, 70, 0), (1, 0, 70, 0), (1, 3, 0, 0), (1, 3, 70, -1), (1, 3, 70, 1 << 31), (1 << 11, 1 << 10, 1 << 10, 0),
                 (1 << 16, 1, 1 << 15, 0)]:
        assert lib().fslic_hip_crf_tensor_workspace_size(*args, C.byref(n)) == B.FSLIC_E_INVALID
    assert lib().fslic_hip_crf_tensor_workspace_size(1, 3, 70, 0, None) == B.FSLIC_E_INVALID
    assert inference_call(nbytes=workspace_size(2, 3, 70, 100) - 1) == B.FSLIC_E_INVALID
    assert b"workspace" in lib().fslic_hip_last_error()
    assert inference_call(indices=NUL, nnz=1) == B.FSLIC_E_INVALID
    assert b"NULL" in lib().fslic_hip_last_error()


def test_capi_workspace_size_is_monotone():
    base = (2, 100, 65, 1000)
    for pos in range(4):
        sizes = []
        for v in (1, 2, 63, 64, 65, 127, 128, 129, 130, 1000, 4097):
            args = list(base)
            args[pos] = v
            sizes.append(workspace_size(*args))
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], (pos, sizes)
