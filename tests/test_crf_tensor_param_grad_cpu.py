"""CPU tests of the learnable energies of superpixel_crf (fast_slic_amd/crf_torch.py: a params tensor, crf_edge_energies, the energies
argument; the fslic_hip_crf_tensor_energies* and *_energies entries): the float64 model the GPU tests compare against
(tests/crf_param_grad_ref.py) against central finite differences for all seven names and for given energies, its agreement with the
model of tests/crf_grad_ref.py, every new ValueError of the Python surface raised before any device work (the tensors are on the CPU, so
a call that passed its argument checks would end at the device check, whose message none of these match; a params tensor or energies
on another device than the unaries need a GPU and are in tests/test_gpu_crf_tensor_param_grad.py), every argument error of the new C
entries, and the workspace sizes by hand.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest
import torch

import crf_grad_ref as R
import crf_param_grad_ref as PR
from fast_slic_amd import _binding as B
from fast_slic_amd.crf import _PARAMS
from fast_slic_amd.crf_torch import DEFAULT_PARAMS, PARAM_NAMES, crf_edge_energies, superpixel_crf
from test_crf_tensor_grad_cpu import small_case

PARAMS = dict(spatial_w=0.7, temporal_w=0.4, spatial_sxy=150.0, spatial_srgb=30.0, temporal_srgb=30.0, spatial_smooth_w=0.3,
              spatial_smooth_sxy=60.0)


def test_param_names():
    assert PARAM_NAMES == _PARAMS == PR.PARAM_NAMES and set(PARAM_NAMES) == set(DEFAULT_PARAMS) and PR.DEFAULTS == DEFAULT_PARAMS


# ---- the model: autograd against central differences, and against the model of the existing backward ----
def test_model_equals_the_model_of_the_fixed_params():
    N, Cn, K, iters = 3, 4, 6, 3
    off, idx, yx, mem, un, q0, compat, weight = small_case(1, N, Cn, K)
    values = {n: float(v) for n, v in zip(PR.PARAM_NAMES, PR.theta_of(PARAMS))}
    old = R.gradients(weight, un, off, idx, yx, mem, iters, params=values, compat=compat, temporal=True, q0=q0)
    new = PR.gradients(weight, un, off, idx, yx, mem, iters, theta=PR.theta_of(PARAMS), compat=compat, temporal=True, q0=q0)
    for name in ("q", "unaries", "compat", "q0"):
        assert float((old[name] - new[name]).abs().max()) <= 1e-12 * max(1.0, float(old[name].abs().max())), name
    # the given energies reproduce it, except that a self-loop would keep its weight: entry 1 of row 1 is one, with energy 0
    given = PR.gradients(weight, un, off, idx, yx, mem, iters, energies_given=(new["edge_value"], new["links_value"]), compat=compat,
                         temporal=True, q0=q0)
    for name in ("q", "unaries", "edge", "links"):
        assert torch.equal(given[name], new[name]), name
    assert int(idx[off[1]]) == 1 and float(new["edge_value"][off[1]]) == 0.0


@pytest.mark.parametrize("temporal", [False, True])
def test_model_autograd_equals_finite_differences(temporal):
    N, Cn, K, iters = 3, 4, 6, 3
    off, idx, yx, mem, un, q0, compat, weight = small_case(1, N, Cn, K)
    theta = PR.theta_of(PARAMS).numpy().copy()
    kw = dict(compat=compat, temporal=temporal, q0=q0)
    grads = PR.gradients(weight, un, off, idx, yx, mem, iters, theta=theta, **kw)
    spatial = [p for p in range(7) if p in PR.SPATIAL]
    assert all(abs(float(grads["theta"][p])) > 1e-6 for p in (spatial if not temporal else range(7)))
    if not temporal:
        assert float(grads["theta"][1]) == 0.0 and float(grads["theta"][3]) == 0.0 and float(grads["links"].abs().max()) == 0.0
    assert torch.all(grads["A"] >= grads["theta"].abs() * (1 - 1e-12)) and torch.all(grads["B"] >= grads["A"] * (1 - 1e-12))
    W = torch.from_numpy(weight)

    def loss_theta(t):
        edge, links = PR.energies(torch.from_numpy(t), off, idx, yx, temporal)
        return float((PR.mean_field(un, off, idx, mem, edge, links, iters, **kw) * W).sum())

    for p in range(7):
        h = 1e-5 * max(1.0, abs(theta[p]))
        hi, lo = theta.copy(), theta.copy()
        hi[p] += h
        lo[p] -= h
        fd = (loss_theta(hi) - loss_theta(lo)) / (2 * h)
        got = float(grads["theta"][p])
        assert abs(got - fd) <= 1e-6 * max(abs(fd), float(grads["A"][p]) * 1e-3, 1e-9), (PR.PARAM_NAMES[p], got, fd)

    # the given energies: any values, a self-loop's included
    rng = np.random.default_rng(5)
    edge = rng.uniform(0.0, 0.5, idx.shape[0])
    links = rng.uniform(0.0, 0.5, (N, 2, K))
    given = PR.gradients(weight, un, off, idx, yx, mem, iters, energies_given=(edge, links), **kw)
    assert float(given["edge"][off[1]]) != 0.0                                     # the self-loop of row 1 carries a gradient here

    def loss_given(e, l):
        return float((PR.mean_field(un, off, idx, mem, torch.from_numpy(e), torch.from_numpy(l), iters, **kw) * W).sum())

    h = 1e-6
    for name, arr in (("edge", edge), ("links", links)):
        for _ in range(6):
            at = tuple(int(rng.integers(0, d)) for d in arr.shape)
            hi, lo = arr.copy(), arr.copy()
            hi[at] += h
            lo[at] -= h
            fd = (loss_given(hi, links) - loss_given(lo, links)) / (2 * h) if name == "edge" else (loss_given(edge, hi) - loss_given(edge, lo)) / (2 * h)
            got = float(given[name][at])
            assert abs(got - fd) <= 1e-6 * max(1.0, abs(fd)), (name, at, got, fd)
    if temporal:
        assert torch.all(given["links"][0, 0] == 0) and torch.all(given["links"][N - 1, 1] == 0)
        assert float(given["links"][1:, 0].abs().max()) > 0 and float(given["links"][:-1, 1].abs().max()) > 0
    else:
        assert torch.all(given["links"] == 0)


def test_model_energies_are_zero_where_nothing_is():
    N, K = 2, 6
    off, idx, yx, mem, un, q0, compat, weight = small_case(3, N, 3, K)
    dirty = np.concatenate([idx, [K, -1, 2]])                                      # off ends before them: behind the last row
    dirty[0] = (1 << 31) - 1
    edge, links, de = PR.energies(PR.theta_of(PARAMS), off, dirty, yx, True, derivatives=True)
    assert edge.shape == dirty.shape and links.shape == (N, 2, K)
    assert float(edge[0]) == 0.0 and torch.all(edge[-3:] == 0) and float(edge[off[1]]) == 0.0 and float(edge.max()) > 0
    assert torch.all(links[0, 0] == 0) and torch.all(links[N - 1, 1] == 0) and torch.equal(links[1, 0], links[0, 1])
    assert all(float(d[0]) == 0.0 and float(d[off[1]]) == 0.0 for p, d in enumerate(de) if p in PR.SPATIAL)
    assert torch.all(PR.energies(PR.theta_of(PARAMS), off, dirty, yx, False)[1] == 0)


# ---- the Python surface: every new ValueError before any device work ----
def cpu_call(**kw):
    N, Cn, K = 2, 3, 6
    off, idx, yx, mem, un, q0, compat, weight = small_case(3, N, Cn, K)
    a = dict(unaries=torch.from_numpy(un).float(), graph=(torch.from_numpy(off), torch.from_numpy(idx).to(torch.int32)),
             yxrgb=torch.from_numpy(yx), members=torch.from_numpy(mem))
    a.update(kw)
    return a, int(idx.shape[0]), N, K


def test_a_list_of_params_is_refused_with_the_old_words():
    a, nnz, N, K = cpu_call()
    with pytest.raises(ValueError, match="params must be None or a dict"):
        superpixel_crf(params=[1.0] * 7, **a)
    with pytest.raises(ValueError, match="params must be None or a dict"):
        crf_edge_energies(a["graph"], a["yxrgb"], a["members"], [1.0] * 7)


@pytest.mark.parametrize("params,words", [
    (torch.zeros(7, dtype=torch.float64), "params tensor must be float32"), (torch.zeros(7, dtype=torch.int32), "params tensor must be float32"),
    (torch.zeros(6), "params tensor must have shape"), (torch.zeros(1, 7), "params tensor must have shape"), (torch.zeros(()), "params tensor must have shape"),
])
def test_params_tensor_errors(params, words):
    a, nnz, N, K = cpu_call()
    with pytest.raises(ValueError, match=words):
        superpixel_crf(params=params, **a)
    with pytest.raises(ValueError, match=words):
        crf_edge_energies(a["graph"], a["yxrgb"], a["members"], params)
    # a good one passes every argument check and ends at the device check, like every CPU tensor
    with pytest.raises(ValueError, match="must be on a ROCm GPU"):
        superpixel_crf(params=torch.ones(7), **a)
    with pytest.raises(ValueError, match="must be on a ROCm GPU"):
        crf_edge_energies(a["graph"], a["yxrgb"], a["members"], torch.ones(7))


def test_energies_errors():
    a, nnz, N, K = cpu_call()
    edge, links = torch.zeros(nnz), torch.zeros(N, 2, K)
    for bad, words in [
        (dict(energies=(edge, links), params={}), "params must be None when energies are given"),
        (dict(energies=(edge, links), params=torch.ones(7)), "params must be None when energies are given"),
        (dict(energies=edge), "energies must be a pair"), (dict(energies=(edge,)), "energies must be a pair"),
        (dict(energies=(edge, links, links)), "energies must be a pair"), (dict(energies={"edge": edge}), "energies must be a pair"),
        (dict(energies=(edge.numpy(), links)), "edge must be a torch tensor"), (dict(energies=(edge, links.numpy())), "links must be a torch tensor"),
        (dict(energies=(edge.double(), links)), "edge must be float32"), (dict(energies=(edge, links.double())), "links must be float32"),
        (dict(energies=(torch.zeros(nnz + 1), links)), "edge must have shape"), (dict(energies=(torch.zeros(nnz, 1), links)), "edge must have shape"),
        (dict(energies=(edge, torch.zeros(N, K, 2))), "links must have shape"), (dict(energies=(edge, torch.zeros(2, K))), "links must have shape"),
        (dict(energies=(edge, None), temporal=True), "links must be given with temporal=True"),
        (dict(yxrgb=None), "yxrgb must be given unless energies are"), (dict(yxrgb=None, params=torch.ones(7)), "yxrgb must be given unless energies are"),
    ]:
        kw = dict(a)
        kw.update(bad)
        with pytest.raises(ValueError, match=words):
            superpixel_crf(**kw)
    # the good ones end at the device check: without yxrgb, without links, unbatched
    for good in (dict(energies=(edge, links)), dict(energies=(edge, links), yxrgb=None, temporal=True), dict(energies=(edge, None), yxrgb=None)):
        kw = dict(a)
        kw.update(good)
        with pytest.raises(ValueError, match="must be on a ROCm GPU"):
            superpixel_crf(**kw)
    one = dict(unaries=a["unaries"][0], graph=(a["graph"][0][:K + 1], a["graph"][1][:int(a["graph"][0][K])]), members=a["members"][0], yxrgb=None)
    n1 = int(a["graph"][0][K])
    with pytest.raises(ValueError, match="must be on a ROCm GPU"):
        superpixel_crf(energies=(torch.zeros(n1), torch.zeros(2, K)), temporal=True, **one)
    with pytest.raises(ValueError, match="links must have shape"):
        superpixel_crf(energies=(torch.zeros(n1), torch.zeros(1, 2, K)), **one)


def test_edge_energies_errors():
    a, nnz, N, K = cpu_call()
    g, yx, mem = a["graph"], a["yxrgb"], a["members"]
    for args, words in [((g, yx.double(), mem), "yxrgb must be float32"), ((g, yx[:, :4], mem), "yxrgb must be"), ((g, yx, mem[0]), "members must have shape"),
                        ((g, yx, mem.long()), "members must be int32"), ((g[0], yx, mem), "graph must be"), ((g, yx, mem, {"nope": 1.0}), "unknown params name")]:
        with pytest.raises(ValueError, match=words):
            crf_edge_energies(*args)
    with pytest.raises(ValueError, match="temporal must be True or False"):
        crf_edge_energies(g, yx, mem, None, 1)
    with pytest.raises(ValueError, match="must be on a ROCm GPU"):
        crf_edge_energies(g, yx, mem, PARAMS, True)


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
P = C.c_void_p(0x1000)
NUL = None
# N = 2, C = 3, K = 70, nnz = 100 as in tests/test_crf_tensor_grad_cpu.py: the given energies change no workspace
FORWARD_BYTES = 2 * 70 * 24 + 800
BACKWARD_BYTES = FORWARD_BYTES + 2 * 2 * 3 * 70 * 4
SLOT_BYTES = 4 * 3 * 4
PLAIN_BYTES = FORWARD_BYTES + 2 * 3 * 70 * 4                                       # fslic_hip_crf_tensor_workspace_size: the second q buffer
PARAM_SLOT_BYTES = 64                                                              # one block of 256 rows: 7 doubles, rounded up to 16


def lib():
    return B.load_library()


def last_error():
    return lib().fslic_hip_last_error()


def energies_call(**kw):
    a = dict(device=0, N=2, k=70, temporal=1, params=P, yxrgb=P, members=P, offsets=P, indices=P, nnz=100, edge=P, links=P)
    a.update(kw)
    return lib().fslic_hip_crf_tensor_energies(a["device"], NUL, a["N"], a["k"], a["temporal"], a["params"], a["yxrgb"], a["members"],
                                               a["offsets"], a["indices"], a["nnz"], a["edge"], a["links"])


def energies_backward_call(**kw):
    a = dict(device=0, N=2, k=70, temporal=1, params=P, yxrgb=P, offsets=P, indices=P, nnz=100, grad_edge=P, grad_links=P, grad_params=P,
             ws=P, nbytes=1 << 40)
    a.update(kw)
    return lib().fslic_hip_crf_tensor_energies_backward(a["device"], NUL, a["N"], a["k"], a["temporal"], a["params"], a["yxrgb"],
                                                        a["offsets"], a["indices"], a["nnz"], a["grad_edge"], a["grad_links"],
                                                        a["grad_params"], a["ws"], a["nbytes"])


def given_call(entry, **kw):
    a = dict(device=0, N=2, Cn=3, k=70, temporal=1, max_iter=3, compat=P, members=P, offsets=P, indices=P, nnz=100, edge=P, links=P,
             t_offsets=P, t_entries=P, t_rows=P, unaries=P, q0=NUL, q=P, grad_q=P, grad_unaries=P, grad_q0=P, grad_compat=P, grad_edge=P,
             grad_links=P, ws=P, nbytes=1 << 40)
    a.update(kw)
    head = (a["device"], NUL, a["N"], a["Cn"], a["k"], a["temporal"], a["max_iter"], a["compat"], a["members"], a["offsets"], a["indices"],
            a["nnz"], a["edge"], a["links"])
    if entry == "backward":
        return lib().fslic_hip_crf_tensor_backward_energies(*head, a["t_offsets"], a["t_entries"], a["t_rows"], a["unaries"], a["q"],
                                                            a["grad_q"], a["grad_unaries"], a["grad_q0"], a["grad_compat"], a["grad_edge"],
                                                            a["grad_links"], a["ws"], a["nbytes"])
    f = lib().fslic_hip_crf_tensor_inference_energies if entry == "inference" else lib().fslic_hip_crf_tensor_inference_saved_energies
    return f(*head, a["unaries"], a["q0"], a["q"], a["ws"], a["nbytes"])


SIZES = [dict(device=-1), dict(N=0), dict(N=-2), dict(k=0), dict(k=-1), dict(temporal=2), dict(temporal=-1), dict(nnz=-1), dict(nnz=1 << 31),
         dict(N=1 << 16, k=1 << 15), dict(N=(1 << 31) - 1, k=1)]
GIVEN = SIZES + [dict(Cn=0), dict(max_iter=-1), dict(N=1 << 11, Cn=1 << 10, k=1 << 10), dict(compat=NUL), dict(members=NUL), dict(offsets=NUL),
                 dict(indices=NUL), dict(edge=NUL), dict(unaries=NUL), dict(q=NUL), dict(ws=NUL), dict(ws=C.c_void_p(0x1008)), dict(nbytes=0)]


@pytest.mark.parametrize("kw", SIZES + [dict(params=NUL), dict(yxrgb=NUL), dict(members=NUL), dict(offsets=NUL), dict(indices=NUL),
                                        dict(edge=NUL), dict(links=NUL)])
def test_capi_energies_refuses(kw):
    assert energies_call(**kw) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", SIZES + [dict(params=NUL), dict(yxrgb=NUL), dict(offsets=NUL), dict(indices=NUL), dict(grad_params=NUL),
                                        dict(ws=NUL), dict(ws=C.c_void_p(0x1008)), dict(nbytes=0), dict(nbytes=PARAM_SLOT_BYTES - 1)])
def test_capi_energies_backward_refuses(kw):
    assert energies_backward_call(**kw) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", GIVEN + [dict(nbytes=PLAIN_BYTES - 1)])
def test_capi_inference_energies_refuses(kw):
    assert given_call("inference", **kw) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", GIVEN + [dict(nbytes=FORWARD_BYTES - 1)])
def test_capi_inference_saved_energies_refuses(kw):
    assert given_call("saved", **kw) == B.FSLIC_E_INVALID


@pytest.mark.parametrize("kw", GIVEN + [dict(grad_q=NUL), dict(grad_unaries=NUL), dict(t_offsets=NUL), dict(t_entries=NUL), dict(t_rows=NUL),
                                        dict(nbytes=BACKWARD_BYTES + SLOT_BYTES - 1), dict(grad_compat=NUL, nbytes=BACKWARD_BYTES - 1)])
def test_capi_backward_energies_refuses(kw):
    assert given_call("backward", **kw) == B.FSLIC_E_INVALID


def test_capi_messages_are_the_existing_entries():
    assert given_call("inference", nbytes=PLAIN_BYTES - 1) == B.FSLIC_E_INVALID
    assert b"workspace too small: %d bytes needed" % PLAIN_BYTES in last_error()
    assert given_call("saved", nbytes=FORWARD_BYTES - 1) == B.FSLIC_E_INVALID
    assert b"workspace too small: %d bytes needed" % FORWARD_BYTES in last_error()
    assert given_call("backward", nbytes=BACKWARD_BYTES) == B.FSLIC_E_INVALID
    assert b"workspace too small: %d bytes needed" % (BACKWARD_BYTES + SLOT_BYTES) in last_error()
    assert energies_backward_call(nbytes=PARAM_SLOT_BYTES - 1) == B.FSLIC_E_INVALID
    assert b"workspace too small: %d bytes needed" % PARAM_SLOT_BYTES in last_error()
    for call in (lambda **kw: given_call("backward", **kw), energies_backward_call):
        assert call(ws=C.c_void_p(0x1008)) == B.FSLIC_E_INVALID
        assert b"workspace must be 16-byte aligned" in last_error()
        assert call(temporal=2) == B.FSLIC_E_INVALID
        assert b"temporal must be 0 or 1" in last_error()
        assert call(nnz=1 << 31) == B.FSLIC_E_INVALID
        assert b"nnz must be in [0, 2^31)" in last_error()
    assert given_call("backward", edge=NUL, nnz=1) == B.FSLIC_E_INVALID
    assert b"NULL" in last_error()
    assert energies_call(links=NUL) == B.FSLIC_E_INVALID
    assert b"NULL" in last_error()
    assert energies_call(N=1 << 16, k=1 << 15) == B.FSLIC_E_INVALID
    assert b"must be below 2^31" in last_error()


def test_capi_energies_backward_workspace_size():
    n = C.c_size_t()
    f = lib().fslic_hip_crf_tensor_energies_backward_workspace_size
    for N, K, blocks in [(2, 70, 1), (1, 1, 1), (1, 256, 1), (1, 257, 2), (8, 1600, 50), (3, 171, 3)]:
        assert f(N, K, C.byref(n)) == 0
        assert n.value == (blocks * 7 * 8 + 15) // 16 * 16, (N, K)
    for args in [(0, 70), (1, 0), (-1, 70), (1 << 16, 1 << 15)]:
        assert f(*args, C.byref(n)) == B.FSLIC_E_INVALID
    assert f(2, 70, None) == B.FSLIC_E_INVALID
    # the given energies take the workspaces of the entries they mirror
    assert lib().fslic_hip_crf_tensor_workspace_size(2, 3, 70, 100, C.byref(n)) == 0 and n.value == PLAIN_BYTES
    assert lib().fslic_hip_crf_tensor_grad_workspace_size(2, 3, 70, 100, 1, 1, C.byref(n)) == 0 and n.value == BACKWARD_BYTES + SLOT_BYTES
