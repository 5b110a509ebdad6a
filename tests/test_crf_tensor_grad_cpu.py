"""CPU tests of the differentiable path of superpixel_crf (fast_slic_amd/crf_torch.py, the fslic_hip_crf_tensor_inference_saved /
_backward / _grad_workspace_size entries): the float64 model the GPU tests compare against (tests/crf_grad_ref.py) against central
finite differences, the transposition helper on CPU tensors against a loop, every argument error of the new C entries refused before
any device work, and the workspace size by hand.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest
import torch

import crf_grad_ref as R
from fast_slic_amd import _binding as B
from fast_slic_amd.crf_torch import transpose_batch_csr


# ---- the model: autograd against central differences ----
def small_case(seed, N, Cn, K):
    rng = np.random.default_rng(seed)
    rows = [[int(v) for v in rng.integers(0, K, int(rng.integers(0, 5)))] for _ in range(N * K)]
    rows[1] = [1, 0, 0]                                                          # a self-loop and a duplicate
    off = np.zeros(N * K + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    idx = np.array([v for r in rows for v in r], np.int64)
    yx = np.concatenate([rng.uniform(0, 200, (N, 2, K)), rng.uniform(0, 40, (N, 3, K))], axis=1).astype(np.float32)
    mem = rng.integers(0, 50, (N, K)).astype(np.int32)
    un = rng.uniform(0.0, 4.0, (N, Cn, K))
    q0 = rng.uniform(0.1, 1.0, (N, Cn, K))
    compat = rng.uniform(0.5, 1.5, Cn)
    weight = rng.normal(0, 1, (N, Cn, K))
    return off, idx, yx, mem, un, q0, compat, weight


@pytest.mark.parametrize("with_q0", [False, True])
def test_model_autograd_equals_finite_differences(with_q0):
    N, Cn, K, iters = 3, 4, 6, 3
    off, idx, yx, mem, un, q0, compat, weight = small_case(1, N, Cn, K)
    params = dict(spatial_w=0.7, temporal_w=0.4, spatial_sxy=150.0, spatial_srgb=30.0, temporal_srgb=30.0, spatial_smooth_w=0.3,
                  spatial_smooth_sxy=60.0)
    kw = dict(params=params, temporal=True)
    start = q0 if with_q0 else None
    grads = R.gradients(weight, un, off, idx, yx, mem, iters, compat=compat, q0=start, **kw)
    assert float(grads["unaries"].abs().max()) > 1e-3 and float(grads["compat"].abs().max()) > 1e-3

    def loss(**changed):
        a = dict(unaries=un, compat=compat, q0=start)
        a.update(changed)
        q = R.mean_field(a["unaries"], off, idx, yx, mem, iters, compat=a["compat"], q0=a["q0"], **kw)
        return float((q * torch.from_numpy(weight)).sum())

    h = 1e-6
    rng = np.random.default_rng(2)
    for name, arr in (("unaries", un), ("compat", compat)) + ((("q0", q0),) if with_q0 else ()):
        for _ in range(5):
            at = tuple(int(rng.integers(0, d)) for d in arr.shape)
            hi, lo = arr.copy(), arr.copy()
            hi[at] += h
            lo[at] -= h
            fd = (loss(**{name: hi}) - loss(**{name: lo})) / (2 * h)
            got = float(grads[name][at])
            assert abs(got - fd) <= 1e-6 * max(1.0, abs(fd)), (name, at, got, fd)


def test_model_drops_out_of_range_entries_and_clamps():
    N, Cn, K = 2, 3, 6
    off, idx, yx, mem, un, q0, compat, weight = small_case(3, N, Cn, K)
    dirty_rows, clean = [], []
    for r in range(N * K):
        row = [int(v) for v in idx[off[r]:off[r + 1]]]
        clean.append(row)
        dirty_rows.append([-1] + row + [K, (1 << 31) - 1])
    d_off = np.zeros(N * K + 1, np.int64)
    d_off[1:] = np.cumsum([len(r) for r in dirty_rows])
    d_idx = np.array([v for r in dirty_rows for v in r], np.int64)
    a = R.mean_field(un, off, idx, yx, mem, 2, temporal=True)
    b = R.mean_field(un, d_off, d_idx, yx, mem, 2, temporal=True)
    assert torch.equal(a, b)
    big = np.full_like(un, 30.0)
    q = R.mean_field(big, off, idx, yx, mem, 1)
    assert float(q.sum(1).max()) < 1e-6                                          # the sum was clamped at 1e-5


# ---- the transposition helper on CPU tensors ----
def check_transpose(rows, N, K):
    off = torch.zeros(N * K + 1, dtype=torch.int64)
    off[1:] = torch.tensor([len(r) for r in rows]).cumsum(0)
    idx = torch.tensor([v for r in rows for v in r], dtype=torch.int64).to(torch.int32)
    t_off, t_ent, t_row = transpose_batch_csr(off, idx, N, K)
    assert t_off.dtype == torch.int64 and t_ent.dtype == torch.int32 and t_row.dtype == torch.int32
    assert t_off.shape == (N * K + 1,) and t_ent.shape == idx.shape and t_row.shape == idx.shape
    exp = R.transpose_loop(off.tolist(), idx.tolist(), N, K)
    for g in range(N * K):
        got = list(zip(t_ent[t_off[g]:t_off[g + 1]].tolist(), t_row[t_off[g]:t_off[g + 1]].tolist()))
        assert got == exp[g], (g, got, exp[g])
        assert [k for k, _ in got] == sorted(k for k, _ in got)                   # ascending entry order inside a target
    assert sorted(t_ent.tolist()) == list(range(idx.shape[0]))                    # a permutation: the dropped entries sit behind
    assert int(t_off[-1]) == sum(len(e) for e in exp)
    return t_off, t_ent, t_row


def test_transpose_by_hand():
    K = 3
    #        row 0      row 1 (self-loop, duplicates)   row 2 (empty)   frame 1: row 3   row 4 (only dead entries)   row 5
    rows = [[1, 2], [1, 0, 0, -1], [], [K, 2, 0], [(1 << 31) - 1, -1], [2, 2]]
    t_off, t_ent, t_row = check_transpose(rows, 2, K)
    assert t_off.tolist() == [0, 2, 4, 5, 6, 6, 9]
    assert t_ent.tolist()[:9] == [3, 4, 0, 2, 1, 8, 7, 11, 12]
    assert t_row.tolist()[:9] == [1, 1, 0, 1, 0, 3, 3, 5, 5]
    assert sorted(t_ent.tolist()[9:]) == [5, 6, 9, 10]                            # -1, K and 2^31 - 1 behind everything


def test_transpose_random_and_empty():
    rng = np.random.default_rng(4)
    N, K = 2, 9
    rows = []
    for r in range(N * K):
        row = [int(v) for v in rng.integers(0, K, int(rng.integers(0, 7)))] if rng.random() > 0.2 else []
        for bad in (-1, K, (1 << 31) - 1):
            if rng.random() < 0.3:
                row.insert(int(rng.integers(0, len(row) + 1)), bad)
        rows.append(row)
    rows[4] = [3] * 5 + [4]
    check_transpose(rows, N, K)
    check_transpose([[] for _ in range(N * K)], N, K)                             # nnz = 0
    # offsets that end before the last entry: the entries behind the last row belong to no target
    off = torch.tensor([0, 1, 2, 2], dtype=torch.int64)
    t_off, t_ent, t_row = transpose_batch_csr(off, torch.tensor([1, 0, 2, 1], dtype=torch.int32), 1, 3)
    assert t_off.tolist() == [0, 1, 2, 2] and t_ent.tolist()[:2] == [1, 0] and t_row.tolist()[:2] == [1, 0]


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
P = C.c_void_p(0x1000)
NUL = None
PARAMS = (C.c_float * 7)(10, 10, 13, 13, 80, 0, 3)
# N = 2, C = 3, K = 70, nnz = 100: rows + temporal, edge, then the backward's two dm planes and the slots of 2 * 2 blocks
FORWARD_BYTES = 2 * 70 * 24 + 800
BACKWARD_BYTES = FORWARD_BYTES + 2 * 2 * 3 * 70 * 4
SLOT_BYTES = 4 * 3 * 4


def lib():
    return B.load_library()


def workspace_size(N, Cn, k, nnz, backward, with_compat):
    n = C.c_size_t()
    assert lib().fslic_hip_crf_tensor_grad_workspace_size(N, Cn, k, nnz, backward, with_compat, C.byref(n)) == 0
    return n.value


def saved_call(**kw):
    a = dict(device=0, N=2, Cn=3, k=70, temporal=1, max_iter=3, params=C.cast(PARAMS, C.c_void_p), compat=P, yxrgb=P, members=P,
             offsets=P, indices=P, nnz=100, unaries=P, q0=NUL, q_all=P, ws=P, nbytes=1 << 40)
    a.update(kw)
    return lib().fslic_hip_crf_tensor_inference_saved(a["device"], NUL, a["N"], a["Cn"], a["k"], a["temporal"], a["max_iter"],
                                                      a["params"], a["compat"], a["yxrgb"], a["members"], a["offsets"], a["indices"],
                                                      a["nnz"], a["unaries"], a["q0"], a["q_all"], a["ws"], a["nbytes"])


def backward_call(**kw):
    a = dict(device=0, N=2, Cn=3, k=70, temporal=1, max_iter=3, params=C.cast(PARAMS, C.c_void_p), compat=P, yxrgb=P, members=P,
             offsets=P, indices=P, nnz=100, t_offsets=P, t_entries=P, t_rows=P, unaries=P, q_all=P, grad_q=P, grad_unaries=P,
             grad_q0=P, grad_compat=P, ws=P, nbytes=1 << 40)
    a.update(kw)
    return lib().fslic_hip_crf_tensor_backward(a["device"], NUL, a["N"], a["Cn"], a["k"], a["temporal"], a["max_iter"], a["params"],
                                               a["compat"], a["yxrgb"], a["members"], a["offsets"], a["indices"], a["nnz"],
                                               a["t_offsets"], a["t_entries"], a["t_rows"], a["unaries"], a["q_all"], a["grad_q"],
                                               a["grad_unaries"], a["grad_q0"], a["grad_compat"], a["ws"], a["nbytes"])


COMMON = [
    dict(device=-1), dict(N=0), dict(N=-2), dict(Cn=0), dict(k=0), dict(k=-1), dict(temporal=2), dict(temporal=-1), dict(max_iter=-1),
    dict(nnz=-1), dict(nnz=1 << 31), dict(N=1 << 11, Cn=1 << 10, k=1 << 10), dict(N=1 << 16, Cn=1, k=1 << 15), dict(N=(1 << 31) - 1, Cn=1, k=1),
    dict(params=NUL), dict(compat=NUL), dict(yxrgb=NUL), dict(members=NUL), dict(offsets=NUL), dict(indices=NUL), dict(unaries=NUL),
    dict(ws=NUL), dict(ws=C.c_void_p(0x1008)), dict(nbytes=0),
]


@pytest.mark.parametrize("kw", COMMON + [dict(q_all=NUL), dict(nbytes=FORWARD_BYTES - 1)])
def test_capi_inference_saved_refuses(kw):
    assert saved_call(**kw) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", COMMON + [
    dict(q_all=NUL), dict(grad_q=NUL), dict(grad_unaries=NUL), dict(t_offsets=NUL), dict(t_entries=NUL), dict(t_rows=NUL),
    dict(nbytes=BACKWARD_BYTES + SLOT_BYTES - 1), dict(grad_compat=NUL, nbytes=BACKWARD_BYTES - 1),
])
def test_capi_backward_refuses(kw):
    assert backward_call(**kw) == B.FSLIC_E_INVALID


def test_capi_messages_are_the_forward_entrys():
    assert saved_call(nbytes=FORWARD_BYTES - 1) == B.FSLIC_E_INVALID
    assert b"workspace too small: %d bytes needed" % FORWARD_BYTES in lib().fslic_hip_last_error()
    assert backward_call(nbytes=BACKWARD_BYTES) == B.FSLIC_E_INVALID
    assert b"workspace too small: %d bytes needed" % (BACKWARD_BYTES + SLOT_BYTES) in lib().fslic_hip_last_error()
    assert backward_call(ws=C.c_void_p(0x1008)) == B.FSLIC_E_INVALID
    assert b"workspace must be 16-byte aligned" in lib().fslic_hip_last_error()
    assert backward_call(t_rows=NUL, nnz=1) == B.FSLIC_E_INVALID
    assert b"NULL" in lib().fslic_hip_last_error()
    assert saved_call(temporal=2) == B.FSLIC_E_INVALID
    assert b"temporal must be 0 or 1" in lib().fslic_hip_last_error()


def test_capi_grad_workspace_size():
    n = C.c_size_t()
    assert workspace_size(2, 3, 70, 100, 0, 0) == FORWARD_BYTES
    assert workspace_size(2, 3, 70, 100, 0, 1) == FORWARD_BYTES                   # the slots belong to the backward
    assert workspace_size(2, 3, 70, 100, 1, 0) == BACKWARD_BYTES
    assert workspace_size(2, 3, 70, 100, 1, 1) == BACKWARD_BYTES + SLOT_BYTES
    assert workspace_size(1, 1, 1, 0, 0, 0) == 16 + 16
    assert workspace_size(1, 1, 1, 0, 1, 1) == 16 + 16 + 16 + 16                  # 8 B of dm and 4 B of slots, each rounded up
    assert workspace_size(1, 128, 70, 3, 1, 0) == 70 * 24 + 32 + 2 * 128 * 70 * 4
    # above 128 classes: the message plane, and for the backward the second plane
    plane = 129 * 70 * 4 + 8
    assert workspace_size(1, 129, 70, 3, 0, 0) == 70 * 24 + 32 + plane
    assert workspace_size(1, 129, 70, 3, 1, 1) == 70 * 24 + 32 + plane + 2 * 129 * 70 * 4 + plane + 2 * 129 * 4 + 8
    assert workspace_size(8, 21, 1600, 8 * 9200, 1, 1) == 8 * 1600 * 24 + 8 * 9200 * 8 + 2 * 8 * 21 * 1600 * 4 + 8 * 25 * 21 * 4
    for args in [(0, 3, 70, 0, 1, 1), (1, 0, 70, 0, 1, 1), (1, 3, 0, 0, 1, 1), (1, 3, 70, -1, 1, 1), (1, 3, 70, 1 << 31, 1, 1),
                 (1 << 11, 1 << 10, 1 << 10, 0, 1, 1), (1 << 16, 1, 1 << 15, 0, 1, 1), (1, 3, 70, 0, 2, 0), (1, 3, 70, 0, 0, -1)]:
        assert lib().fslic_hip_crf_tensor_grad_workspace_size(*args, C.byref(n)) == B.FSLIC_E_INVALID
    assert lib().fslic_hip_crf_tensor_grad_workspace_size(1, 3, 70, 0, 1, 1, None) == B.FSLIC_E_INVALID
