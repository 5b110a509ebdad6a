"""The backward of superpixel_crf on the MI355X (fast_slic_amd/crf_torch.py, csrc/crf_tensor_grad.hip).

Gradients of (q * W).sum() with respect to unaries, a tensor compat and q0 against the float64 model of tests/crf_grad_ref.py.  The
kernel has no bit-equal reference, so its bound is measured against the model inside the test: with
err = max |x - ref| / max |ref| and b the err of the SAME model evaluated in float32 on the CPU, the kernel must satisfy
err <= max(8 b, 2^-20): three bits for two float32 evaluations that differ in summation order and in crf_expf against torch's exp, and
a floor of a few ulps of the largest element.  Every figure is printed before it is asserted (pytest -s shows them).  Beside that:
exact checks by ==, the clamped sum, bit-exact properties (the forward with gradients against the forward without, repeated calls,
batch position, neighbour entries out of range), the side conditions (no grad_fn without a gradient, inputs untouched, streams, no host
synchronisation) and the chain pool -> CRF -> unpool -> cross_entropy."""
import os

import numpy as np
import pytest
import torch

import crf_cases as CC
import crf_grad_ref as R
from fast_slic_amd import _binding as B
from fast_slic_amd.crf_torch import superpixel_crf
from fast_slic_amd.pool import superpixel_pool, superpixel_unpool
from fast_slic_amd.rag import superpixel_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crf_cases.npz"))
LDS_CUT = 128                     # kCrfTensorLdsClasses (csrc/crf_tensor.h)
FLOOR = 2.0 ** -20
# the params and compat of tests/test_gpu_crf_tensor.py; with its clusters (colours all over 0 .. 255 against a deviation of 13)
# nearly every energy is tiny, so a second set gives every edge a weight that matters
PARAMS = dict(spatial_w=3.5, temporal_w=7.25, spatial_smooth_w=2.5, spatial_sxy=200.0)
COUPLED = dict(spatial_w=0.05, temporal_w=0.05, spatial_srgb=300.0, temporal_srgb=300.0, spatial_sxy=2000.0, spatial_smooth_w=0.02,
               spatial_smooth_sxy=1000.0)


def compat_of(Cn):
    return [0.5 + 0.25 * (c % 5) for c in range(Cn)]


def cluster_tensors(clusters):
    """CLUSTER_DTYPE[N][K] -> yxrgb float32 [N, 5, K], members int32 [N, K] on the GPU."""
    yx = np.stack([np.stack([cl[n] for n in ("y", "x", "r", "g", "b")]) for cl in clusters]).astype(np.float32)
    mem = np.stack([cl["num_members"].view(np.int32) for cl in clusters])
    return torch.from_numpy(yx).to(DEV), torch.from_numpy(np.ascontiguousarray(mem)).to(DEV)


def csr_tensors(rows):
    """rows[N][K] lists -> one CSR over (frame, node) on the GPU."""
    flat = [r for frame in rows for r in frame]
    off = np.zeros(len(flat) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in flat])
    idx = np.array([v for r in flat for v in r], np.int64).astype(np.int32)
    return torch.from_numpy(off).to(DEV), torch.from_numpy(idx).to(DEV)


def on_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def random_case(seed, N, Cn, K, max_degree=12, hub=0):
    """Clusters, neighbour lists (duplicates, self-loops, empty rows; node 0 of every frame with `hub` entries) and unaries: the
    generator of tests/test_gpu_crf_tensor.py."""
    rng = np.random.default_rng(seed)
    clusters, rows = [], []
    for _ in range(N):
        cl = np.zeros(K, B.CLUSTER_DTYPE)
        cl["y"] = rng.integers(0, 720, K).astype(np.float32) + rng.integers(0, 4, K) * np.float32(0.25)
        cl["x"] = rng.integers(0, 1280, K).astype(np.float32) + rng.integers(0, 8, K) * np.float32(0.125)
        for ch in ("r", "g", "b"):
            cl[ch] = rng.integers(0, 256, K).astype(np.float32)
        cl["number"] = np.arange(K)
        cl["num_members"] = rng.integers(1, 900, K)
        cl["num_members"][rng.random(K) < 0.1] = 0
        clusters.append(cl)
        frame = []
        for i in range(K):
            r = [int(v) for v in rng.integers(0, K, int(rng.integers(0, max_degree + 1)))] if rng.random() > 0.1 else []
            if len(r) > 2:
                r[1] = r[0]
                r[-1] = i
            frame.append(r)
        if hub:
            frame[0] = [int(v) for v in rng.integers(0, K, hub)]
        rows.append(frame)
    unaries = rng.uniform(0.0, 4.0, (N, Cn, K)).astype(np.float32)
    return clusters, rows, unaries


class Case(object):
    """One random case on the GPU and on the host, with W and a q0."""

    def __init__(self, seed, N, Cn, K, hub=0, fan_in=0, rows=None):
        self.clusters, self.rows, self.unaries = random_case(seed, N, Cn, K, hub=hub)
        if rows is not None:
            self.rows = rows
        for t in range(fan_in):                                   # node 1 of every frame as the target of `fan_in` entries
            for frame in self.rows:
                frame[(7 * t) % K].append(1)
        rng = np.random.default_rng(seed + 99)
        self.weight = rng.normal(0.0, 1.0, (N, Cn, K)).astype(np.float32)
        q0 = rng.uniform(0.05, 1.0, (N, Cn, K))
        self.q0 = (q0 / q0.sum(1, keepdims=True)).astype(np.float32)
        self.N, self.Cn, self.K = N, Cn, K
        self.compat = np.array(compat_of(Cn), np.float32)
        self.yx, self.mem = cluster_tensors(self.clusters)
        self.graph = csr_tensors(self.rows)

    def gpu(self, iters, params, temporal, with_q0, frames=None, graph=None, unaries=None, compat_grad=True):
        """-> q and the tensors whose .grad the backward fills: (q, unaries, compat, q0 or None)."""
        sel = slice(None) if frames is None else frames
        un = on_gpu(self.unaries[sel] if unaries is None else unaries).requires_grad_(True)
        comp = on_gpu(self.compat).requires_grad_(compat_grad)
        q0 = on_gpu(self.q0[sel]).requires_grad_(True) if with_q0 else None
        q = superpixel_crf(un, self.graph if graph is None else graph, self.yx[sel], self.mem[sel], max_iter=iters, params=params,
                           compat=comp, temporal=temporal, q0=q0)
        return q, un, comp, q0

    def grads(self, iters, params, temporal, with_q0, **kw):
        q, un, comp, q0 = self.gpu(iters, params, temporal, with_q0, **kw)
        sel = kw.get("frames")
        (q * on_gpu(self.weight[slice(None) if sel is None else sel])).sum().backward()
        return dict(q=q.detach(), unaries=un.grad, compat=comp.grad, q0=None if q0 is None else q0.grad)

    def model(self, iters, params, temporal, with_q0, dtype, unaries=None):
        off, idx = (t.cpu() for t in self.graph)
        return R.gradients(self.weight, self.unaries if unaries is None else unaries, off, idx, self.yx.cpu(), self.mem.cpu(), iters,
                           params=params, compat=self.compat, temporal=temporal, q0=self.q0 if with_q0 else None, dtype=dtype)


def assert_within_bound(got, ref64, ref32, what):
    """err <= max(8 b, 2^-20) for every gradient, every figure printed first."""
    figures = []
    for name in ("unaries", "compat", "q0"):
        if ref64[name] is None:
            assert got[name] is None
            continue
        err, b = R.rel_err(got[name], ref64[name]), R.rel_err(ref32[name], ref64[name])
        figures.append((name, err, b))
        print("%s d%s: err %.3g  b %.3g  bound %.3g  max|ref| %.3g" % (what, name, err, b, max(8 * b, FLOOR), float(ref64[name].abs().max())))
    for name, err, b in figures:
        assert np.isfinite(err) and err <= max(8 * b, FLOOR), "%s d%s: err %.3g above max(8 * %.3g, 2^-20)" % (what, name, err, b)


# ---- gradients against the float64 model ----
SHAPES = [
    (2, 3, 63, 0, 0), (2, 3, 64, 0, 0), (2, 3, 65, 0, 0), (2, 21, 129, 0, 0),      # the wavefront and block seams
    (3, 17, 70, 0, 0),                                                              # a middle frame with both temporal neighbours
    (1, LDS_CUT, 70, 0, 0), (2, LDS_CUT + 1, 70, 0, 0),                             # the LDS cut from both sides
    (2, 3, 70, 300, 0), (2, 3, 70, 0, 300),                                         # a hub row of 300 entries; one target of 300 entries
]


@pytest.mark.parametrize("params", [PARAMS, COUPLED], ids=["params", "coupled"])
@pytest.mark.parametrize("N,Cn,K,hub,fan_in", SHAPES)
def test_gradients_match_the_float64_model(N, Cn, K, hub, fan_in, params):
    case = Case(N * 1000 + Cn * 10 + K, N, Cn, K, hub=hub, fan_in=fan_in)
    for iters in (1, 4):                                                            # both parities of the ping-pong
        for temporal in (False, True):
            for with_q0 in (False, True):
                got = case.grads(iters, params, temporal, with_q0)
                ref64 = case.model(iters, params, temporal, with_q0, torch.float64)
                ref32 = case.model(iters, params, temporal, with_q0, torch.float32)
                what = "N=%d C=%d K=%d hub=%d fan_in=%d sweeps=%d temporal=%d q0=%d" % (N, Cn, K, hub, fan_in, iters, temporal, with_q0)
                assert got["q"].shape == (N, Cn, K) and got["unaries"].shape == (N, Cn, K) and got["compat"].shape == (Cn,)
                assert_within_bound(got, ref64, ref32, what)


# ---- exact checks ----
def test_one_class_has_zero_gradients():
    case = Case(21, 2, 1, 70)
    for temporal in (False, True):
        got = case.grads(3, COUPLED, temporal, False)
        assert torch.equal(got["q"], torch.ones_like(got["q"]))
        assert torch.all(got["unaries"] == 0) and torch.all(got["compat"] == 0)


def test_no_entries_means_no_spatial_term():
    K = 70
    case = Case(22, 2, 3, K, rows=[[[] for _ in range(K)] for _ in range(2)])
    assert case.graph[1].shape == (0,)
    one = case.grads(1, COUPLED, False, True)
    four = case.grads(4, COUPLED, False, True)
    # without neighbours a sweep does not look at its input: every sweep gives the same q, only the last one has a gradient
    assert torch.equal(one["q"], four["q"])
    assert torch.equal(one["unaries"], four["unaries"]) and float(one["unaries"].abs().max()) > 0
    assert torch.all(four["q0"] == 0) and torch.all(one["q0"] == 0) and torch.all(four["compat"] == 0)
    assert_within_bound(four, case.model(4, COUPLED, False, True, torch.float64), case.model(4, COUPLED, False, True, torch.float32), "nnz=0")
    # the temporal links alone do carry a gradient back
    window = case.grads(2, COUPLED, True, True)
    assert float(window["q0"].abs().max()) > 0
    assert_within_bound(window, case.model(2, COUPLED, True, True, torch.float64), case.model(2, COUPLED, True, True, torch.float32),
                        "nnz=0 temporal")


def test_no_sweeps():
    case = Case(23, 2, 3, 70)
    w = on_gpu(case.weight)
    given = case.grads(0, PARAMS, True, True)
    assert torch.equal(given["q"], on_gpu(case.q0))
    assert torch.equal(given["q0"], w) and torch.all(given["unaries"] == 0) and torch.all(given["compat"] == 0)
    start = case.grads(0, PARAMS, True, False)
    assert torch.equal(start["unaries"], -start["q"] * w) and torch.all(start["compat"] == 0)


# ---- the clamped sum ----
def test_clamped_nodes():
    N, Cn, K = 2, 3, 70
    case = Case(24, N, Cn, K)
    un = case.unaries.copy()
    clamped = np.random.default_rng(25).random((N, K)) < 0.1
    assert 5 <= clamped.sum() <= 30
    un[np.broadcast_to(clamped[:, None, :], un.shape)] = 30.0                       # a sum near C * 1e-13, far below 1e-5
    for with_q0 in (False, True):
        got = case.grads(2, COUPLED, True, with_q0, unaries=un)
        sums = got["q"].sum(1).cpu().numpy()
        assert np.all(sums[clamped] < 1.0) and np.all(np.abs(sums[~clamped] - 1.0) < 1e-5)
        assert_within_bound(got, case.model(2, COUPLED, True, with_q0, torch.float64, unaries=un),
                            case.model(2, COUPLED, True, with_q0, torch.float32, unaries=un), "clamped q0=%d" % with_q0)


# ---- bit-exact properties ----
def fixture(name):
    case, frames = CC.unpack_frames(GOLD, name)
    T = case["T"]
    frames = frames[:T]
    unaries = [GOLD["%s/f%d/unaries" % (name, j)] if frames[j]["umode"] != "unary" else frames[j]["udata"] for j in range(T)]
    rows = [[list(map(int, f["idx"][f["off"][i]:f["off"][i + 1]])) for i in range(case["K"])] for f in frames]
    yx, mem = cluster_tensors([f["clusters"] for f in frames])
    params = dict(zip(CC.PARAM_NAMES, case["params"])) if case.get("params") else None
    q0 = np.stack([GOLD["%s/q0/%d" % (name, j)] for j in range(T)])
    return case, on_gpu(np.stack(unaries).astype(np.float32)), csr_tensors(rows), yx, mem, params, case.get("compat"), q0


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_forward_with_gradients_has_the_forwards_bits(name):
    case, un, graph, yx, mem, params, compat, q0 = fixture(name)
    kw = dict(max_iter=case["iters"][0], params=params, compat=compat, temporal=True)
    plain = superpixel_crf(un, graph, yx, mem, q0=on_gpu(q0), **kw)
    assert plain.grad_fn is None
    q = superpixel_crf(un.clone().requires_grad_(True), graph, yx, mem, q0=on_gpu(q0), **kw)
    assert q.grad_fn is not None and q.shape == plain.shape and torch.equal(q, plain)
    start = superpixel_crf(un, graph, yx, mem, q0=on_gpu(q0).requires_grad_(True), **kw)       # q0 alone asks for the gradient
    assert start.grad_fn is not None and torch.equal(start, plain)
    none = superpixel_crf(un.clone().requires_grad_(True), graph, yx, mem, **kw)
    assert torch.equal(none, superpixel_crf(un, graph, yx, mem, **kw))


@pytest.mark.parametrize("N,Cn,K", [(2, 21, 129), (2, LDS_CUT + 1, 70)])
def test_forward_bits_and_repeated_calls(N, Cn, K):
    case = Case(26, N, Cn, K)
    for iters in (0, 1, 2, 3):                                                      # no sweep, both parities of the ping-pong
        for with_q0 in (False, True):
            a = case.grads(iters, COUPLED, True, with_q0)
            b = case.grads(iters, COUPLED, True, with_q0)
            with torch.no_grad():
                plain = case.gpu(iters, COUPLED, True, with_q0)[0]
            assert torch.equal(a["q"], plain), (iters, with_q0)
            for name in ("unaries", "compat", "q0"):
                assert (a[name] is None and b[name] is None) or torch.equal(a[name], b[name]), (name, iters, with_q0)
            if iters >= 1:                                                          # (test_no_sweeps states the values at 0)
                assert float(a["unaries"].abs().max()) > 0 and float(a["compat"].abs().max()) > 0


def test_batch_position():
    case = Case(27, 3, 5, 150)
    K = 150
    for pos in (1, 2):
        rows = [case.rows[pos]]
        alone = Case(27, 1, 5, K, rows=rows)
        alone.unaries, alone.weight, alone.q0 = case.unaries[pos:pos + 1], case.weight[pos:pos + 1], case.q0[pos:pos + 1]
        alone.yx, alone.mem = case.yx[pos:pos + 1].contiguous(), case.mem[pos:pos + 1].contiguous()
        for with_q0 in (False, True):
            whole = case.grads(3, COUPLED, False, with_q0, compat_grad=False)
            single = alone.grads(3, COUPLED, False, with_q0, compat_grad=False)
            assert torch.equal(whole["q"][pos], single["q"][0])
            assert torch.equal(whole["unaries"][pos], single["unaries"][0]), "position %d" % pos
            assert whole["compat"] is None
            if with_q0:
                assert torch.equal(whole["q0"][pos], single["q0"][0]), "position %d" % pos


def test_out_of_range_entries_change_nothing():
    K = 70
    case = Case(28, 2, 3, K)
    rng = np.random.default_rng(29)
    dirty = []
    for frame in case.rows:
        out = []
        for r in frame:
            r = list(r)
            for bad in (-1, K, (1 << 31) - 1):
                if rng.random() < 0.4:
                    r.insert(int(rng.integers(0, len(r) + 1)), bad)
            out.append(r)
        dirty.append(out)
    dirty[0][3] = [-1, K, (1 << 31) - 1] + case.rows[0][3]
    dirty[1][0] = [(1 << 31) - 1] + case.rows[1][0] + [-1]
    assert sum(len(r) for f in dirty for r in f) > sum(len(r) for f in case.rows for r in f) + 50
    for temporal in (False, True):
        clean = case.grads(3, COUPLED, temporal, True)
        got = case.grads(3, COUPLED, temporal, True, graph=csr_tensors(dirty))
        for name in ("q", "unaries", "compat", "q0"):
            assert torch.equal(got[name], clean[name]), (name, temporal)


# ---- side conditions ----
def test_no_grad_fn_without_a_gradient():
    case = Case(30, 2, 3, 70)
    with torch.no_grad():
        q = case.gpu(2, PARAMS, True, True)[0]
    assert q.grad_fn is None and not q.requires_grad
    plain = superpixel_crf(on_gpu(case.unaries), case.graph, case.yx, case.mem, max_iter=2, params=PARAMS, compat=on_gpu(case.compat),
                           temporal=True, q0=on_gpu(case.q0))
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, q)
    # a yxrgb that requires a gradient is accepted and gets none
    yx = case.yx.clone().requires_grad_(True)
    still = superpixel_crf(on_gpu(case.unaries), case.graph, yx, case.mem, max_iter=2, params=PARAMS, temporal=True)
    assert still.grad_fn is None
    un = on_gpu(case.unaries).requires_grad_(True)
    superpixel_crf(un, case.graph, yx, case.mem, max_iter=2, params=PARAMS, temporal=True).sum().backward()
    assert yx.grad is None and un.grad is not None
    # a compat given as floats needs no gradient; an unbatched frame is the batch of one
    one = superpixel_crf(on_gpu(case.unaries[0]).requires_grad_(True), csr_tensors(case.rows[:1]), case.yx[0], case.mem[0], max_iter=2,
                         compat=compat_of(3))
    assert one.shape == (3, 70) and one.grad_fn is not None


def test_non_default_stream_and_inputs_unchanged():
    case = Case(31, 2, 5, 129)
    exp = case.grads(3, COUPLED, True, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        q, un, comp, q0 = case.gpu(3, COUPLED, True, True)
        before = [t.detach().clone() for t in (un, comp, q0, case.yx, case.mem) + case.graph]
        kept = q.detach().clone()
        (q * on_gpu(case.weight)).sum().backward()
    side.synchronize()
    assert torch.equal(q, kept) and torch.equal(q, exp["q"])
    assert torch.equal(un.grad, exp["unaries"]) and torch.equal(comp.grad, exp["compat"]) and torch.equal(q0.grad, exp["q0"])
    for t, b in zip((un, comp, q0, case.yx, case.mem) + case.graph, before):
        assert torch.equal(t.detach(), b)


def block_labels(H=48, W=64, bh=6, bw=8):
    """A label map of bh x bw pixel blocks: (H / bh) * (W / bw) segments."""
    yy, xx = np.meshgrid(np.arange(H) // bh, np.arange(W) // bw, indexing="ij")
    return (yy * (W // bw) + xx).astype(np.int32)


def pooled_clusters(lab, K, seed):
    """yxrgb and members of a label map [N, H, W] as the chain pools them."""
    N, H, W = lab.shape
    img = on_gpu(np.random.default_rng(seed).integers(0, 256, (N, 3, H, W)).astype(np.float32))
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
    yxrgb, counts = superpixel_pool(torch.cat([torch.stack([yy, xx]).expand(N, 2, H, W), img], dim=1), lab, K, return_counts=True)
    return yxrgb, counts


def test_no_host_synchronisation():
    K = 64
    lab = on_gpu(np.stack([block_labels(), block_labels()[:, ::-1]]))
    graph = superpixel_graph(lab, K)                                                # (synchronises: the number of edges shapes its result)
    pair = tuple(t.clone() for t in graph.to_batch_csr())
    yxrgb, counts = pooled_clusters(lab, K, 32)
    rng = np.random.default_rng(33)
    un_dev, w = on_gpu(rng.uniform(0.0, 4.0, (2, 3, K)).astype(np.float32)), on_gpu(rng.normal(0, 1, (2, 3, K)).astype(np.float32))
    ones = torch.ones(3, device=DEV)
    params = dict(spatial_w=0.5, spatial_srgb=100.0)

    def run(g):
        un = un_dev.clone().requires_grad_(True)
        comp = ones.clone().requires_grad_(True)
        q = superpixel_crf(un, g, yxrgb, counts, max_iter=3, params=params, compat=comp, temporal=True)
        (q * w).sum().backward()
        return q.detach(), un.grad, comp.grad

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
    assert float(exp[1].abs().max()) > 0 and float(exp[2].abs().max()) > 0


# ---- the chain ----
def test_chain_gradient_reaches_the_logits():
    Cn, H, W, K, iters = 5, 48, 64, 64, 3
    lab_host = block_labels(H, W)
    lab = on_gpu(lab_host)
    rng = np.random.default_rng(34)
    logits_host = rng.normal(0, 2, (Cn, H, W)).astype(np.float32)
    target_host = rng.integers(0, Cn, (H, W))
    yxrgb, counts = pooled_clusters(lab[None], K, 35)
    yxrgb, counts = yxrgb[0], counts[0]
    graph = superpixel_graph(lab, K)
    params = dict(spatial_w=0.5, spatial_srgb=100.0)

    logits = on_gpu(logits_host).requires_grad_(True)
    un = -torch.log(superpixel_pool(torch.softmax(logits, dim=0), lab, K).clamp_min(1e-6))
    q = superpixel_crf(un, graph, yxrgb, counts, max_iter=iters, params=params)
    assert q.grad_fn is not None
    loss = torch.nn.functional.cross_entropy(superpixel_unpool(q, lab)[None], on_gpu(target_host)[None])
    loss.backward()
    assert logits.grad is not None and bool(torch.isfinite(logits.grad).all()) and float(logits.grad.abs().max()) > 0

    off, idx = (t.cpu() for t in graph.to_batch_csr())
    flat = torch.from_numpy(lab_host.reshape(-1).astype(np.int64))

    def reference(dtype):
        lg = torch.from_numpy(logits_host).to(dtype).requires_grad_(True)
        p = torch.softmax(lg, dim=0).reshape(Cn, H * W)
        pooled = torch.zeros(Cn, K, dtype=dtype).index_add(1, flat, p) / counts.cpu().to(dtype)
        u = -torch.log(pooled.clamp_min(1e-6))
        qr = R.mean_field(u[None], off, idx, yxrgb.cpu()[None], counts.cpu()[None], iters, params=params, dtype=dtype)[0]
        out = torch.nn.functional.cross_entropy(qr[:, flat].reshape(1, Cn, H, W), torch.from_numpy(target_host)[None])
        out.backward()
        return out.detach(), lg.grad

    loss64, ref64 = reference(torch.float64)
    _, ref32 = reference(torch.float32)
    err, b = R.rel_err(logits.grad, ref64), R.rel_err(ref32, ref64)
    print("chain dlogits: err %.3g  b %.3g  bound %.3g  loss %.6f against %.6f" % (err, b, max(8 * b, FLOOR), float(loss.detach()), float(loss64)))
    assert err <= max(8 * b, FLOOR)
