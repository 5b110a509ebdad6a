"""The learnable energies of superpixel_crf on the MI355X (fast_slic_amd/crf_torch.py; csrc/crf_tensor.hip, csrc/crf_tensor_grad.hip): a
params tensor, crf_edge_energies and the energies argument.

Inputs are the generators, PARAMS and COUPLED of tests/test_gpu_crf_tensor_grad.py at its SHAPES, 1 and 4 sweeps, temporal off and on
(the two shapes with C >= 128 at 4 sweeps with temporal on only).  The references are the models of tests/crf_param_grad_ref.py.  The
rule is that file's: with err = max |x - ref| / max |ref| and b the err of the same model evaluated in float32 on the CPU, a gradient
tensor must satisfy err <= max(8 b, 2^-20).  The gradient of the seven params has its own scales (crf_param_grad_ref.scales):
  the reduction alone      |x_p - ref_p| / A_p <= max(8 b_p, 2^-20), b_p the float32 model's figure in the same metric (terms and sums
                           are double in the kernel, so its own error is the final rounding);
  end to end               |x_p - ref_p| <= max(8 b_e, 2^-20) B_p + 2^-20 A_p, b_e the larger of the float32 model's err on the two
                           energy gradients: what the two bounds above imply by the triangle inequality.
The reduction is checked with COUPLED and with MIXED below, not with PARAMS: with PARAMS' deviations (13 for colours all over 0 .. 255,
3 for positions hundreds of pixels apart) whole columns of d energy / d param lie below the smallest float32, so A_p is a number the
float32 result cannot hold and the relative metric says nothing.  Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import crf_param_grad_ref as PR
import test_gpu_crf_tensor_grad as G
from fast_slic_amd.crf import SimpleCRF
from fast_slic_amd.crf_torch import DEFAULT_PARAMS, PARAM_NAMES, crf_edge_energies, superpixel_crf
from fast_slic_amd.pool import superpixel_pool, superpixel_unpool
from fast_slic_amd.rag import superpixel_graph

pytestmark = pytest.mark.gpu
DEV, FLOOR, PARAMS, COUPLED, SHAPES, on_gpu = G.DEV, G.FLOOR, G.PARAMS, G.COUPLED, G.SHAPES, G.on_gpu
MIXED = dict(spatial_w=3.5, temporal_w=7.25, spatial_srgb=120.0, temporal_srgb=90.0, spatial_sxy=700.0, spatial_smooth_w=2.5,
             spatial_smooth_sxy=400.0)


def combos(Cn):
    return [(4, True)] if Cn >= G.LDS_CUT else [(1, False), (1, True), (4, False), (4, True)]


@functools.lru_cache(maxsize=None)
def case_of(shape):
    N, Cn, K, hub, fan_in = shape
    return G.Case(N * 1000 + Cn * 10 + K, N, Cn, K, hub=hub, fan_in=fan_in)


def theta_gpu(params, grad=False):
    return PR.theta_of(params, torch.float32).to(DEV).requires_grad_(grad)


def values_of(params):
    """The dict of the float32 values of theta_gpu(params)."""
    return {n: float(v) for n, v in zip(PARAM_NAMES, PR.theta_of(params, torch.float32))}


def leaves(case, grad, with_q0):
    un = on_gpu(case.unaries).requires_grad_(grad)
    comp = on_gpu(case.compat).requires_grad_(grad)
    q0 = on_gpu(case.q0).requires_grad_(grad) if with_q0 else None
    return un, comp, q0


def crf(case, iters, temporal, un, comp, q0, yxrgb=True, **kw):
    return superpixel_crf(un, case.graph, case.yx if yxrgb else None, case.mem, max_iter=iters, compat=comp, temporal=temporal, q0=q0, **kw)


def backward(case, q):
    (q * on_gpu(case.weight)).sum().backward()


@functools.lru_cache(maxsize=None)
def given_run(shape, iters, temporal, params_key="coupled", energy_grads=True):
    """The sweeps on the energies of `params` given as leaves -> the energies, q and every gradient (q0 only with 1 sweep)."""
    case = case_of(shape)
    with torch.no_grad():
        edge, links = crf_edge_energies(case.graph, case.yx, case.mem, theta_gpu(KEYS[params_key]), temporal)
    e, l = edge.clone().requires_grad_(energy_grads), links.clone().requires_grad_(energy_grads)
    un, comp, q0 = leaves(case, True, iters == 1)
    q = crf(case, iters, temporal, un, comp, q0, yxrgb=False, energies=(e, l))
    backward(case, q)
    return dict(edge_value=edge, links_value=links, q=q.detach(), unaries=un.grad, compat=comp.grad, q0=None if q0 is None else q0.grad,
                edge=e.grad, links=l.grad)


@functools.lru_cache(maxsize=None)
def composed_run(shape, iters, temporal):
    """superpixel_crf(params=theta) with COUPLED -> q and theta.grad."""
    case = case_of(shape)
    theta = theta_gpu(COUPLED, True)
    un, comp, q0 = leaves(case, True, iters == 1)
    q = crf(case, iters, temporal, un, comp, q0, params=theta)
    backward(case, q)
    return dict(q=q.detach(), theta=theta.grad, unaries=un.grad, compat=comp.grad)


KEYS = dict(coupled=COUPLED, params=PARAMS, mixed=MIXED)


def model_args(case, iters, temporal):
    off, idx = (t.cpu() for t in case.graph)
    return (case.weight, case.unaries, off, idx, case.yx.cpu(), case.mem.cpu(), iters), dict(
        compat=case.compat, temporal=temporal, q0=case.q0 if iters == 1 else None)


def what_of(shape, iters, temporal):
    return "N=%d C=%d K=%d hub=%d fan_in=%d sweeps=%d temporal=%d" % (shape + (iters, temporal))


# ---- 1. bits ----
@pytest.mark.parametrize("key", ["params", "coupled"])
@pytest.mark.parametrize("shape", SHAPES)
def test_q_has_the_bits_of_the_dict_call(shape, key):
    case, params = case_of(shape), KEYS[key]
    for iters, temporal in combos(shape[1]):
        with_q0 = iters == 1
        plain = crf(case, iters, temporal, *leaves(case, False, with_q0), params=values_of(params))
        assert plain.grad_fn is None
        theta = theta_gpu(params)
        by_tensor = crf(case, iters, temporal, *leaves(case, False, with_q0), params=theta)
        edge, links = crf_edge_energies(case.graph, case.yx, case.mem, theta, temporal)
        assert edge.shape == case.graph[1].shape and links.shape == (case.N, 2, case.K) and edge.dtype == links.dtype == torch.float32
        by_energies = crf(case, iters, temporal, *leaves(case, False, with_q0), yxrgb=False, energies=(edge, links))
        assert by_tensor.grad_fn is None and by_energies.grad_fn is None and edge.grad_fn is None
        assert torch.equal(by_tensor, plain) and torch.equal(by_energies, plain), what_of(shape, iters, temporal)
        # the same with gradients asked for: through the params, through the energies, through the unaries alone
        theta_g = theta_gpu(params, True)
        a = crf(case, iters, temporal, *leaves(case, False, with_q0), params=theta_g)
        e_g, l_g = crf_edge_energies(case.graph, case.yx, case.mem, theta_g, temporal)
        b = crf(case, iters, temporal, *leaves(case, False, with_q0), energies=(e_g, l_g))
        c = crf(case, iters, temporal, *leaves(case, True, with_q0), params=theta)
        d = crf(case, iters, temporal, *leaves(case, False, with_q0), yxrgb=False,
                energies=(edge.clone().requires_grad_(True), links if temporal else None))
        assert torch.equal(e_g, edge) and torch.equal(l_g, links) and e_g.grad_fn is not None
        for q in (a, b, c, d):
            assert q.grad_fn is not None and torch.equal(q, plain), what_of(shape, iters, temporal)
        if not temporal:
            assert torch.all(links == 0)
        assert torch.all(links[0, 0] == 0) and torch.all(links[-1, 1] == 0)


@pytest.mark.parametrize("N,Cn,K", [(2, 21, 129), (2, G.LDS_CUT + 1, 70)])
def test_forward_bits_and_repeated_calls_with_energies(N, Cn, K):
    """test_forward_bits_and_repeated_calls of tests/test_gpu_crf_tensor_grad.py through energies=."""
    case = G.Case(26, N, Cn, K)
    with torch.no_grad():
        edge, links = crf_edge_energies(case.graph, case.yx, case.mem, theta_gpu(COUPLED), True)

    def grads(iters, with_q0):
        e, l = edge.clone().requires_grad_(True), links.clone().requires_grad_(True)
        un, comp, q0 = leaves(case, True, with_q0)
        q = crf(case, iters, True, un, comp, q0, yxrgb=False, energies=(e, l))
        backward(case, q)
        return dict(q=q.detach(), unaries=un.grad, compat=comp.grad, q0=None if q0 is None else q0.grad, edge=e.grad, links=l.grad)

    for iters in (0, 1, 2, 3):                                                      # no sweep, both parities of the ping-pong
        for with_q0 in (False, True):
            a, b = grads(iters, with_q0), grads(iters, with_q0)
            with torch.no_grad():
                plain = crf(case, iters, True, *leaves(case, True, with_q0), yxrgb=False, energies=(edge, links))
            assert torch.equal(a["q"], plain), (iters, with_q0)
            for name in ("unaries", "compat", "q0", "edge", "links"):
                assert (a[name] is None and b[name] is None) or torch.equal(a[name], b[name]), (name, iters, with_q0)
            if iters >= 1:
                assert float(a["unaries"].abs().max()) > 0 and float(a["compat"].abs().max()) > 0


def test_energies_are_simple_crfs_and_zero_where_nothing_is():
    N, Cn, K = 3, 3, 70
    case = G.Case(41, N, Cn, K)
    rows = [[list(r) for r in frame] for frame in case.rows]
    rows[0][3] = [-1, K, (1 << 31) - 1, 3, 5] + rows[0][3]
    rows[2][K - 1] = [K - 1, 0, K] + rows[2][K - 1]
    graph = G.csr_tensors(rows)
    for params in (None, PARAMS, COUPLED):
        crf_ = SimpleCRF(Cn, K)
        for n, v in values_of(params).items():
            setattr(crf_, n, v)
        frames = []
        for cl in case.clusters:
            f = crf_.push_frame()
            f.set_clusters(cl)
            frames.append(f)
        edge, links = crf_edge_energies(graph, case.yx, case.mem, theta_gpu(params), True)
        by_dict = crf_edge_energies(graph, case.yx, case.mem, None if params is None else values_of(params), True)
        assert torch.equal(by_dict[0], edge) and torch.equal(by_dict[1], links)
        edge, links = edge.cpu().numpy(), links.cpu().numpy()
        k, checked, live = 0, 0, 0
        for n in range(N):
            for i in range(K):
                for j in rows[n][i]:
                    if not 0 <= j < K or j == i:
                        assert edge[k] == 0.0, (n, i, j)
                        checked += 1
                    elif k % 7 == 0 or i in (3, K - 1):
                        assert edge[k] == np.float32(frames[n].spatial_pairwise_energy(j, i)), (n, i, j)
                        live += edge[k] != 0
                    k += 1
        assert k == edge.shape[0] and checked >= 8 and (params is not COUPLED or live > 50)
        for n in range(N):
            for i in (0, 1, 17, K - 1):
                assert links[n, 0, i] == (np.float32(frames[n].temporal_pairwise_energy(i, frames[n - 1])) if n > 0 else 0.0)
                assert links[n, 1, i] == (np.float32(frames[n].temporal_pairwise_energy(i, frames[n + 1])) if n < N - 1 else 0.0)
        assert params is not COUPLED or float(np.abs(links).max()) > 0
    off_links = crf_edge_energies(graph, case.yx, case.mem, theta_gpu(COUPLED))[1]
    assert torch.all(off_links == 0)
    # unbatched clusters: [2, K], all zero (no other frame); offsets that end early leave the entries behind them at 0.0
    first = [list(r) for r in rows[0]]
    first[K - 1] = [0, 1, 2]
    off, idx = G.csr_tensors([first])
    one = crf_edge_energies((off, idx), case.yx[0], case.mem[0], COUPLED, True)
    assert one[1].shape == (2, K) and torch.all(one[1] == 0)
    n_same = int(off[K - 1])
    assert torch.equal(one[0][:n_same], crf_edge_energies(graph, case.yx, case.mem, COUPLED, True)[0][:n_same])
    short = off.clone()
    short[-1] -= 2
    cut = crf_edge_energies((short, idx), case.yx[0], case.mem[0], COUPLED)[0]
    assert torch.all(cut[-2:] == 0) and torch.equal(cut[:-2], one[0][:-2]) and float(one[0][-2:].abs().min()) > 0


# ---- 2. the gradients of the energies ----
def assert_tensor_rule(got, ref64, ref32, what):
    err, b = PR_rel(got, ref64), PR_rel(ref32, ref64)
    print("%s: err %.3g  b %.3g  bound %.3g  max|ref| %.3g" % (what, err, b, max(8 * b, FLOOR), float(ref64.abs().max()) if ref64.numel() else 0.0))
    assert np.isfinite(err) and err <= max(8 * b, FLOOR), "%s: err %.3g above max(8 * %.3g, 2^-20)" % (what, err, b)
    return b


def PR_rel(x, ref):
    return G.R.rel_err(x, ref) if torch.as_tensor(ref).numel() else 0.0


@pytest.mark.parametrize("shape", SHAPES)
def test_energy_gradients_match_the_float64_model(shape):
    case = case_of(shape)
    for iters, temporal in combos(shape[1]):
        got = given_run(shape, iters, temporal)
        args, kw = model_args(case, iters, temporal)
        given = (got["edge_value"].cpu(), got["links_value"].cpu())
        ref64 = PR.gradients(*args, energies_given=given, dtype=torch.float64, **kw)
        ref32 = PR.gradients(*args, energies_given=given, dtype=torch.float32, **kw)
        what = what_of(shape, iters, temporal)
        assert got["edge"].shape == case.graph[1].shape and got["links"].shape == (case.N, 2, case.K)
        for name in ("edge", "links", "unaries", "compat"):
            assert_tensor_rule(got[name], ref64[name], ref32[name], "%s d%s" % (what, name))
        assert float(got["edge"].abs().max()) > 0
        assert torch.all(got["links"][0, 0] == 0) and torch.all(got["links"][-1, 1] == 0)
        if temporal and case.N > 1:
            assert float(got["links"].abs().max()) > 0
        else:
            assert torch.all(got["links"] == 0)
        # the other gradients do not depend on who else asks for one
        base = given_run(shape, iters, temporal, energy_grads=False)
        assert base["edge"] is None and base["links"] is None
        for name in ("q", "unaries", "compat", "q0"):
            assert (got[name] is None and base[name] is None) or torch.equal(got[name], base[name]), (what, name)


def test_dead_entries_get_no_gradient_and_change_nothing():
    K = 70
    case = G.Case(28, 2, 3, K)
    rng = np.random.default_rng(29)
    dirty, keep = [], []
    for frame in case.rows:
        out = []
        for r in frame:
            r = list(r)
            for bad in (-1, K, (1 << 31) - 1):
                if rng.random() < 0.4:
                    r.insert(int(rng.integers(0, len(r) + 1)), bad)
            out.append(r)
            keep += [0 <= v < K for v in r]
        dirty.append(out)
    keep = torch.tensor(keep, device=DEV)
    assert int((~keep).sum()) > 50
    graph = G.csr_tensors(dirty)
    for temporal in (False, True):
        res = []
        for g in (case.graph, graph):
            edge, links = crf_edge_energies(g, case.yx, case.mem, theta_gpu(COUPLED), temporal)
            e, l = edge.clone().requires_grad_(True), links.clone().requires_grad_(True)
            un, comp, q0 = leaves(case, True, True)
            q = superpixel_crf(un, g, None, case.mem, max_iter=3, compat=comp, temporal=temporal, q0=q0, energies=(e, l))
            backward(case, q)
            theta = theta_gpu(COUPLED, True)
            backward(case, superpixel_crf(on_gpu(case.unaries), g, case.yx, case.mem, max_iter=3, params=theta, compat=on_gpu(case.compat),
                                          temporal=temporal, q0=on_gpu(case.q0)))
            res.append((q.detach(), edge, e.grad, l.grad, un.grad, comp.grad, q0.grad, theta.grad))
        clean, got = res
        assert torch.all(got[1][~keep] == 0) and torch.all(got[2][~keep] == 0)
        assert torch.equal(got[1][keep], clean[1]) and torch.equal(got[2][keep], clean[2]) and float(clean[2].abs().max()) > 0
        for a, b in zip(got[3:], clean[3:]):
            assert torch.equal(a, b)
        assert torch.equal(got[0], clean[0])
        # garbage at the dead entries of a given edge is never read into anything
        e = got[1].clone()
        e[~keep] = float("nan")
        e.requires_grad_(True)
        given_links = crf_edge_energies(graph, case.yx, case.mem, COUPLED, True)[1] if temporal else None
        un, comp, q0 = leaves(case, True, True)
        q = superpixel_crf(un, graph, None, case.mem, max_iter=3, compat=comp, temporal=temporal, q0=q0, energies=(e, given_links))
        backward(case, q)
        assert torch.equal(q.detach(), clean[0]) and torch.equal(e.grad, got[2]) and torch.equal(un.grad, clean[4])


# ---- 3. the reduction ----
@pytest.mark.parametrize("key", ["coupled", "mixed"])
@pytest.mark.parametrize("shape", SHAPES)
def test_params_gradient_of_the_energies_alone(shape, key):
    case = case_of(shape)
    off, idx = (t.cpu() for t in case.graph)
    rng = np.random.default_rng(50 + shape[2])
    g_edge = rng.normal(0, 1, idx.shape[0]).astype(np.float32)
    g_links = rng.normal(0, 1, (case.N, 2, case.K)).astype(np.float32)
    for temporal in (False, True):
        theta = theta_gpu(KEYS[key], True)
        edge, links = crf_edge_energies(case.graph, case.yx, case.mem, theta, temporal)
        torch.autograd.backward([edge, links], [on_gpu(g_edge), on_gpu(g_links)])
        x = theta.grad.cpu().double()
        assert theta.grad.dtype == torch.float32 and theta.grad.shape == (7,)
        ref64, A = PR.energies_backward(theta.detach().cpu(), off, idx, case.yx.cpu(), temporal, g_edge, g_links, torch.float64)
        ref32, _ = PR.energies_backward(theta.detach().cpu(), off, idx, case.yx.cpu(), temporal, g_edge, g_links, torch.float32)
        figures = []
        for p, name in enumerate(PARAM_NAMES):
            a = float(A[p])
            err = abs(float(x[p] - ref64[p])) / a if a > 0 else abs(float(x[p]))
            b = abs(float(ref32[p].double() - ref64[p])) / a if a > 0 else 0.0
            figures.append((name, err, b, a))
            print("N=%d C=%d K=%d hub=%d fan_in=%d temporal=%d %s d%s: err %.3g  b %.3g  bound %.3g  A %.3g  ref %.6g" % (
                shape + (temporal, key, name, err, b, max(8 * b, FLOOR) if a > 0 else 0.0, a, float(ref64[p]))))
        for name, err, b, a in figures:
            assert np.isfinite(err) and err <= (max(8 * b, FLOOR) if a > 0 else 0.0), (name, err, b, a)
        live = [0, 2, 4, 5, 6] + ([1, 3] if temporal and case.N > 1 else [])
        assert all(float(A[p]) > 0 and float(x[p]) != 0 for p in live)


# ---- 4. composition ----
@pytest.mark.parametrize("shape", SHAPES)
def test_params_gradient_is_the_energies_backward_of_the_energy_gradients(shape):
    case = case_of(shape)
    for iters, temporal in combos(shape[1]):
        whole, parts = composed_run(shape, iters, temporal), given_run(shape, iters, temporal)
        theta = theta_gpu(COUPLED, True)
        edge, links = crf_edge_energies(case.graph, case.yx, case.mem, theta, temporal)
        torch.autograd.backward([edge, links], [parts["edge"], parts["links"]])
        print("%s: dtheta %s" % (what_of(shape, iters, temporal), whole["theta"].tolist()))
        assert torch.equal(whole["theta"], theta.grad), what_of(shape, iters, temporal)
        for name in ("q", "unaries", "compat"):
            assert torch.equal(whole[name], parts[name]), name


# ---- 5. end to end against the model ----
@pytest.mark.parametrize("shape", SHAPES)
def test_params_gradient_matches_the_float64_model(shape):
    case = case_of(shape)
    for iters, temporal in combos(shape[1]):
        x = composed_run(shape, iters, temporal)["theta"].cpu().double()
        args, kw = model_args(case, iters, temporal)
        theta = PR.theta_of(COUPLED, torch.float32)
        ref64 = PR.gradients(*args, theta=theta, dtype=torch.float64, **kw)
        ref32 = PR.gradients(*args, theta=theta, dtype=torch.float32, **kw)
        b_e = max(PR_rel(ref32["edge"], ref64["edge"]), PR_rel(ref32["links"], ref64["links"]))
        what = what_of(shape, iters, temporal)
        figures = []
        for p, name in enumerate(PARAM_NAMES):
            bound = max(8 * b_e, FLOOR) * float(ref64["B"][p]) + FLOOR * float(ref64["A"][p])
            diff = abs(float(x[p] - ref64["theta"][p]))
            figures.append((name, diff, bound))
            print("%s d%s: |x - ref| %.3g  bound %.3g  b_e %.3g  ref %.6g  A %.3g  B %.3g  float32 model off by %.3g" % (
                what, name, diff, bound, b_e, float(ref64["theta"][p]), float(ref64["A"][p]), float(ref64["B"][p]),
                abs(float(ref32["theta"][p].double() - ref64["theta"][p]))))
        for name, diff, bound in figures:
            assert np.isfinite(diff) and diff <= bound, "%s d%s: %.3g above %.3g" % (what, name, diff, bound)


# ---- 6. exact zeros ----
def theta_grad(case, iters, temporal, params, **kw):
    theta = theta_gpu(params, True)
    un, comp, q0 = leaves(case, True, True)
    q = crf(case, iters, temporal, un, comp, q0, params=theta, **kw)
    backward(case, q)
    return theta.grad


def test_exact_zeros():
    case = G.Case(61, 3, 3, 70)
    names = list(PARAM_NAMES)
    no_smooth = dict(COUPLED, spatial_smooth_w=0.0)
    for temporal in (False, True):
        g = theta_grad(case, 3, temporal, no_smooth)
        assert float(g[names.index("spatial_smooth_sxy")]) == 0.0 and float(g[names.index("spatial_smooth_w")]) != 0.0
        assert float(g[names.index("spatial_w")]) != 0.0
    g = theta_grad(case, 3, False, COUPLED)
    assert float(g[1]) == 0.0 and float(g[3]) == 0.0 and all(float(g[p]) != 0.0 for p in (0, 2, 4, 5, 6))
    g = theta_grad(case, 3, True, COUPLED)
    assert all(float(v) != 0.0 for v in g)
    single = G.Case(62, 1, 3, 70)
    g = theta_grad(single, 3, True, COUPLED)                                       # one frame: no link
    assert float(g[1]) == 0.0 and float(g[3]) == 0.0 and float(g[0]) != 0.0
    for temporal in (False, True):
        assert torch.all(theta_grad(case, 0, temporal, COUPLED) == 0)               # no sweep
        assert torch.all(theta_grad(G.Case(63, 2, 1, 70), 3, temporal, COUPLED) == 0)      # one class
    K = 70
    empty = G.Case(64, 2, 3, K, rows=[[[] for _ in range(K)] for _ in range(2)])
    assert empty.graph[1].shape == (0,)
    assert torch.all(theta_grad(empty, 3, False, COUPLED) == 0)
    g = theta_grad(empty, 3, True, COUPLED)                                         # the links alone
    assert all(float(g[p]) == 0.0 for p in (0, 2, 4, 5, 6)) and float(g[1]) != 0.0 and float(g[3]) != 0.0
    # the energies of an empty graph, and their gradients
    e = torch.zeros(0, device=DEV, requires_grad=True)
    l = crf_edge_energies(empty.graph, empty.yx, empty.mem, COUPLED, True)[1].requires_grad_(True)
    un, comp, q0 = leaves(empty, False, True)
    backward(empty, crf(empty, 2, True, un, comp, q0, yxrgb=False, energies=(e, l)))
    assert e.grad.shape == (0,) and float(l.grad.abs().max()) > 0


# ---- 7. side conditions ----
def test_no_grad_fn_without_a_gradient():
    case = G.Case(30, 2, 3, 70)
    theta = theta_gpu(COUPLED, True)
    with torch.no_grad():
        q = crf(case, 2, True, *leaves(case, False, True), params=theta)
        edge, links = crf_edge_energies(case.graph, case.yx, case.mem, theta, True)
    assert q.grad_fn is None and not q.requires_grad and edge.grad_fn is None and links.grad_fn is None
    plain = crf(case, 2, True, *leaves(case, False, True), params=theta.detach())
    given = crf(case, 2, True, *leaves(case, False, True), yxrgb=False, energies=(edge, links))
    assert plain.grad_fn is None and given.grad_fn is None and torch.equal(plain, q) and torch.equal(given, q)
    assert plain._base is None and given._base is None                              # not a view of kept iterates
    # a yxrgb that requires a gradient gets none, from neither function
    yx = case.yx.clone().requires_grad_(True)
    edge, links = crf_edge_energies(case.graph, yx, case.mem, theta, True)
    assert edge.grad_fn is not None
    torch.autograd.backward([edge, links], [torch.ones_like(edge), torch.ones_like(links)])
    assert yx.grad is None and theta.grad is not None
    # the refusals that need a GPU: a params tensor or energies that live elsewhere
    un, comp, q0 = leaves(case, False, False)
    with pytest.raises(ValueError, match="params must be on a ROCm GPU"):
        crf(case, 2, True, un, comp, q0, params=torch.ones(7))
    with pytest.raises(ValueError, match="params must be on a ROCm GPU"):
        crf_edge_energies(case.graph, case.yx, case.mem, torch.ones(7))
    with pytest.raises(ValueError, match="edge must be on a ROCm GPU"):
        crf(case, 2, True, un, comp, q0, energies=(edge.detach().cpu(), links.detach()))
    with pytest.raises(ValueError, match="links must be on a ROCm GPU"):
        crf(case, 2, True, un, comp, q0, energies=(edge.detach(), links.detach().cpu()))
    # an unbatched frame is the batch of one
    one = superpixel_crf(on_gpu(case.unaries[0]), G.csr_tensors(case.rows[:1]), case.yx[0], case.mem[0], max_iter=2, params=theta_gpu(COUPLED, True))
    assert one.shape == (3, 70) and one.grad_fn is not None
    batch = superpixel_crf(on_gpu(case.unaries[:1]), G.csr_tensors(case.rows[:1]), case.yx[:1], case.mem[:1], max_iter=2, params=COUPLED)
    assert torch.equal(one.detach(), batch[0])


def test_non_default_stream_inputs_unchanged_and_repeated_calls():
    shape = (2, 5, 129, 0, 0)
    case = G.Case(31, 2, 5, 129)

    def run():
        theta = theta_gpu(COUPLED, True)
        un, comp, q0 = leaves(case, True, True)
        q = crf(case, 3, True, un, comp, q0, params=theta)
        edge, links = crf_edge_energies(case.graph, case.yx, case.mem, theta.detach(), True)
        e, l = edge.clone().requires_grad_(True), links.clone().requires_grad_(True)
        q2 = crf(case, 3, True, on_gpu(case.unaries), on_gpu(case.compat), on_gpu(case.q0), yxrgb=False, energies=(e, l))
        inputs = (theta, un, comp, q0, edge, links, case.yx, case.mem) + case.graph
        before = [t.detach().clone() for t in inputs]
        kept = q.detach().clone()
        backward(case, q)
        backward(case, q2)
        return (q, q2, theta.grad, un.grad, comp.grad, q0.grad, e.grad, l.grad), inputs, before, kept

    exp = run()[0]
    again = run()[0]
    for a, b in zip(exp, again):
        assert torch.equal(a, b)
    assert float(exp[2].abs().min()) > 0 and float(exp[6].abs().max()) > 0 and float(exp[7].abs().max()) > 0
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got, inputs, before, kept = run()
    side.synchronize()
    assert torch.equal(got[0], kept)
    for a, b in zip(got, exp):
        assert torch.equal(a, b)
    for t, b in zip(inputs, before):
        assert torch.equal(t.detach(), b)
    assert shape[2] == case.K


def test_batch_position():
    K = 150
    case = G.Case(27, 3, 5, K)
    off = case.graph[0].cpu()
    theta = theta_gpu(COUPLED)
    edge, links = crf_edge_energies(case.graph, case.yx, case.mem, theta)
    for pos in (1, 2):
        alone = G.Case(27, 1, 5, K, rows=[case.rows[pos]])
        alone.unaries, alone.weight, alone.q0 = case.unaries[pos:pos + 1], case.weight[pos:pos + 1], case.q0[pos:pos + 1]
        alone.yx, alone.mem = case.yx[pos:pos + 1].contiguous(), case.mem[pos:pos + 1].contiguous()
        k0, k1 = int(off[pos * K]), int(off[(pos + 1) * K])
        e1, l1 = crf_edge_energies(alone.graph, alone.yx, alone.mem, theta)
        assert torch.equal(e1, edge[k0:k1]) and torch.all(l1 == 0)
        e, a = edge.clone().requires_grad_(True), e1.clone().requires_grad_(True)
        whole = crf(case, 3, False, *leaves(case, False, True), yxrgb=False, energies=(e, None))
        single = crf(alone, 3, False, *leaves(alone, False, True), yxrgb=False, energies=(a, None))
        backward(case, whole)
        backward(alone, single)
        assert torch.equal(whole[pos], single[0]) and torch.equal(e.grad[k0:k1], a.grad), "position %d" % pos
        assert float(a.grad.abs().max()) > 0


def test_no_host_synchronisation():
    K = 64
    lab = on_gpu(np.stack([G.block_labels(), G.block_labels()[:, ::-1]]))
    graph = superpixel_graph(lab, K)                                                # (synchronises: the number of edges shapes its result)
    pair = tuple(t.clone() for t in graph.to_batch_csr())
    yxrgb, counts = G.pooled_clusters(lab, K, 32)
    rng = np.random.default_rng(33)
    un_dev, w = on_gpu(rng.uniform(0.0, 4.0, (2, 3, K)).astype(np.float32)), on_gpu(rng.normal(0, 1, (2, 3, K)).astype(np.float32))
    start = theta_gpu(dict(spatial_w=0.5, spatial_srgb=100.0, temporal_w=0.5, temporal_srgb=100.0, spatial_smooth_w=0.1, spatial_smooth_sxy=30.0))

    def run(g):
        theta = start.clone().requires_grad_(True)
        un = un_dev.clone().requires_grad_(True)
        q = superpixel_crf(un, g, yxrgb, counts, max_iter=3, params=theta, temporal=True)
        (q * w).sum().backward()
        with torch.no_grad():
            edge, links = crf_edge_energies(g, yxrgb, counts, start, True)
            plain = superpixel_crf(un_dev, g, None, counts, max_iter=3, energies=(edge, links), temporal=True)
        e, l = edge.clone().requires_grad_(True), links.clone().requires_grad_(True)
        q2 = superpixel_crf(un_dev, g, None, counts, max_iter=3, energies=(e, l), temporal=True)
        (q2 * w).sum().backward()
        return q.detach(), theta.grad, un.grad, plain, q2.detach(), e.grad, l.grad

    exp = run(graph)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            got_graph, got_pair = run(graph), run(pair)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error')")
    for got in (got_graph, got_pair):
        assert all(torch.equal(a, b) for a, b in zip(got, exp))
    assert torch.equal(exp[0], exp[3]) and torch.equal(exp[0], exp[4])
    assert float(exp[1].abs().min()) > 0 and float(exp[5].abs().max()) > 0 and float(exp[6].abs().max()) > 0


# ---- the chain, with the params as an nn.Parameter ----
def test_chain_trains_the_params():
    Cn, H, W, K, iters = 5, 48, 64, 64, 3
    lab = on_gpu(G.block_labels(H, W))
    rng = np.random.default_rng(34)
    logits = on_gpu(rng.normal(0, 2, (Cn, H, W)).astype(np.float32)).requires_grad_(True)
    target = on_gpu(rng.integers(0, Cn, (H, W)))
    yxrgb, counts = G.pooled_clusters(lab[None], K, 35)
    yxrgb, counts = yxrgb[0], counts[0]
    graph = superpixel_graph(lab, K)
    values = dict(DEFAULT_PARAMS, spatial_w=0.5, spatial_srgb=100.0, spatial_smooth_w=0.1, spatial_smooth_sxy=30.0)
    theta = torch.nn.Parameter(torch.tensor([values[n] for n in PARAM_NAMES], device=DEV))
    opt = torch.optim.SGD([theta], lr=0.1)
    before = theta.detach().clone()
    un = -torch.log(superpixel_pool(torch.softmax(logits, dim=0), lab, K).clamp_min(1e-6))
    q = superpixel_crf(un, graph, yxrgb, counts, max_iter=iters, params=theta)
    assert torch.equal(q, superpixel_crf(un.detach(), graph, yxrgb, counts, max_iter=iters, params=values))
    loss = torch.nn.functional.cross_entropy(superpixel_unpool(q, lab)[None], target[None])
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(theta.grad).all()) and bool(torch.isfinite(logits.grad).all())
    print("chain: loss %.6f  dtheta %s" % (float(loss.detach()), theta.grad.tolist()))
    assert float(theta.grad[1]) == 0.0 and float(theta.grad[3]) == 0.0             # one frame: no temporal link
    assert all(float(theta.grad[p]) != 0.0 for p in (0, 2, 4, 5, 6)) and float(logits.grad.abs().max()) > 0
    opt.step()
    assert not torch.equal(theta.detach(), before) and bool(torch.isfinite(theta).all())
