"""Soft superpixel assignment on the MI355X (fast_slic_amd/soft.py, csrc/soft.hip) against the float64 model of tests/soft_ref.py.

Per function, one stage each, so nothing compounds.  The kernels have no bit-equal reference, so the bound is measured against the
model inside the test: with err = max |x - ref64| / max |ref64| and b the err of the SAME model evaluated in float32 on the CPU, the
kernel must satisfy err <= max(8 b, 2^-20): three bits for two float32 evaluations that differ in summation order and in the
exponential, and a floor of a few ulps of the largest element.  Every figure is printed before it is asserted (pytest -s shows them).
Beside that: exact checks by == on the bits (invalid slots, the one-hot Q against superpixel_pool / superpixel_unpool, repeated calls,
batch position, streams, channel permutations), the side conditions (no host synchronisation, inputs untouched, no grad_fn without a
gradient), soft_slic end to end and the chain into pool -> graph -> CRF -> unpool."""
import numpy as np
import pytest
import torch

import soft_ref as R
from fast_slic_amd.compare import label_overlap
from fast_slic_amd.crf_torch import superpixel_crf
from fast_slic_amd.pool import superpixel_pool, superpixel_unpool
from fast_slic_amd.rag import superpixel_graph
from fast_slic_amd.soft import _pool_raw, soft_assign, soft_labels, soft_pool, soft_slic, soft_unpool, with_coords
from fast_slic_amd.synth import variant as synth
from soft_cases import DEV, FLOOR, Case, bits_equal, hold, rel                     # shared with test_gpu_soft_edges.py

pytestmark = pytest.mark.gpu
N = 3                                       # Case's default number of frames
# the smallest shapes at which the kernels can go wrong: cell sizes that do not divide; K = 1 (only slot 4 is valid); a strip each
# way; one-pixel-tall and 65-pixel-wide cells with rows that cross a wavefront; a window of 36 864 pixels, past the staging buffer
SHAPES = [(37, 53, (3, 5)), (9, 9, (1, 1)), (5, 64, (1, 7)), (64, 5, (7, 1)), (16, 130, (16, 2)), (192, 192, (1, 1))]
CHANNELS = [1, 3, 70]                      # 70 is past a channel chunk of 16
CASES = [(H, W, g, Cc) for (H, W, g) in SHAPES for Cc in CHANNELS]
_cache = {}


def case(H, W, grid, Cc):
    key = (H, W, grid, Cc)
    if key not in _cache:
        _cache[key] = Case(H, W, grid, Cc)
    return _cache[key]


# ---- every stage against the model, and the properties that hold bit for bit ----
WORST = {}


@pytest.mark.parametrize("H,W,grid,Cc", CASES)
def test_stages_against_the_model(H, W, grid, Cc):
    c = case(H, W, grid, Cc)
    got = c.gpu()
    torch.cuda.synchronize()
    print("\n%dx%d grid %s C=%d" % (H, W, grid, Cc))
    failures = []
    for name in sorted(got):
        try:
            r = hold(name, got[name], c.ref[torch.float64][name], c.ref[torch.float32][name])
            WORST[name] = max(WORST.get(name, 0.0), r)
        except AssertionError as e:
            failures.append(str(e))
    print("worst err/bound so far: " + ", ".join("%s %.3f" % (k, WORST[k]) for k in sorted(WORST)))
    assert not failures, "; ".join(failures)
    # invalid slots: Q is +0.0 there, and so is every gradient with respect to Q
    _, ok = R.slots(H, W, grid)
    bad = (~ok).to(DEV).unsqueeze(0).expand(N, 9, H, W)
    for name in ("assign Q", "pool gQ", "unpool gQ"):
        assert bool((got[name][bad].view(torch.int32) == 0).all()), name + " is not +0.0 on an invalid slot"
    s = got["assign Q"].sum(1)
    assert float((s - 1).abs().max()) <= 1e-6
    # repeated calls, and frame 1 alone against frame 1 of the batch
    again, alone = c.gpu(), c.gpu(slice(1, 2))
    for name in got:
        assert bits_equal(again[name], got[name]), name + " differs between two calls"
        assert bits_equal(alone[name][0], got[name][1]), name + " depends on the batch position"


@pytest.mark.parametrize("H,W,grid", SHAPES)
def test_one_hot_q_is_hard_pooling(H, W, grid):
    K = grid[0] * grid[1]
    g = torch.Generator().manual_seed(H + W)
    lab = R.cell_labels(H, W, grid).to(DEV)
    labn = lab.unsqueeze(0).expand(N, H, W).contiguous()
    q = R.one_hot(N, H, W, torch.float32).to(DEV)
    assert torch.equal(soft_labels(q, grid), labn) and soft_labels(q, grid).dtype == torch.int32
    assert torch.equal(soft_labels(q[0], grid), lab)
    for Cc in (3, 70):
        F = torch.randint(0, 256, (N, Cc, H, W), generator=g).float().to(DEV)           # integer sums below 2^24: exact in any order
        sums, weights = soft_pool(F, q, grid, normalize=False, return_weights=True)
        want, counts = superpixel_pool(F, labn, K, "sum", return_counts=True)
        assert bits_equal(sums, want) and torch.equal(weights, counts.float())
        mean = soft_pool(F, q, grid)
        assert bits_equal(mean, want / counts.float().unsqueeze(1))
        V = torch.randn(N, Cc, K, generator=g).to(DEV)
        assert bits_equal(soft_unpool(V, q, grid), superpixel_unpool(V, labn))
        assert bits_equal(soft_unpool(V[0], q[0], grid), superpixel_unpool(V[0], lab))


@pytest.mark.parametrize("H,W,grid", [(37, 53, (3, 5)), (192, 192, (1, 1))])
def test_pool_ignores_the_other_channels(H, W, grid):
    c = case(H, W, grid, 70)
    F, Q, S = c.F.to(DEV), c.Q.to(DEV), c.S.to(DEV)
    perm = torch.randperm(70, generator=torch.Generator().manual_seed(1))
    base = soft_pool(F, Q, grid, normalize=False)
    assert bits_equal(soft_pool(F[:, perm].contiguous(), Q, grid, normalize=False), base[:, perm])
    assert bits_equal(soft_pool(F[:, 17:18].contiguous(), Q, grid, normalize=False), base[:, 17:18])
    # and the centred form (the pass behind the gradient of the centres), on the same weights
    full = _pool_raw(F, Q, grid, centres=S, weights=False)[0]
    assert float(full.abs().max()) > 0 and not bits_equal(full, base)
    assert bits_equal(_pool_raw(F[:, perm].contiguous(), Q, grid, centres=S[:, perm].contiguous(), weights=False)[0], full[:, perm])
    assert bits_equal(_pool_raw(F[:, 17:18].contiguous(), Q, grid, centres=S[:, 17:18].contiguous(), weights=False)[0], full[:, 17:18])


def test_on_a_non_default_stream():
    c = case(37, 53, (3, 5), 3)
    exp = c.gpu()
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        got = c.gpu()
    st.synchronize()
    for name in exp:
        assert bits_equal(got[name], exp[name]), name


def test_no_host_synchronisation():
    c = case(37, 53, (3, 5), 3)
    t = c.tensors(DEV)                                    # uploaded before the check: a copy from pageable memory synchronises
    F = t["F"]

    def run():
        out = c.gpu(t=t)
        f = F.clone().requires_grad_(True)
        q, cen = soft_slic(with_coords(f, c.grid, 10.0), c.grid, max_iter=2)
        (soft_unpool(soft_pool(f, q, c.grid), q, c.grid) - f).pow(2).sum().backward()
        out.update(slic_q=q.detach(), slic_centres=cen.detach(), slic_grad=f.grad, labels=soft_labels(q, c.grid).float())
        return out

    exp = run()
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
            got = run()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error')")
    for name in exp:
        assert bits_equal(got[name], exp[name]), name


def test_inputs_untouched_and_no_grad_fn_without_a_gradient():
    c = case(5, 64, (1, 7), 3)
    F, S, Q, V = (t.to(DEV) for t in (c.F, c.S, c.Q, c.V))
    keep = [t.clone() for t in (F, S, Q, V)]
    q = soft_assign(F, S, c.grid)
    sums, w = soft_pool(F, Q, c.grid, return_weights=True)
    o = soft_unpool(V, Q, c.grid)
    sq, sc = soft_slic(F, c.grid, max_iter=1)
    assert all(t.grad_fn is None and not t.requires_grad for t in (q, sums, w, o, sq, sc))
    Fg = F.clone().requires_grad_(True)
    assert soft_assign(Fg, S, c.grid).grad_fn is not None and soft_pool(Fg, Q, c.grid).grad_fn is not None
    with torch.no_grad():
        assert soft_assign(Fg, S, c.grid).grad_fn is None
    gq = soft_assign(Fg, S, c.grid)
    torch.autograd.grad((gq * c.gQ.to(DEV)).sum(), Fg)
    torch.cuda.synchronize()
    for t, k in zip((F, S, Q, V), keep):
        assert bits_equal(t, k)
    # unbatched tensors lose the batch dimension and give the batch's bits
    assert bits_equal(soft_assign(F[1], S[1], c.grid), q[1]) and bits_equal(soft_unpool(V[1], Q[1], c.grid), o[1])
    s1, w1 = soft_pool(F[1], Q[1], c.grid, return_weights=True)
    assert bits_equal(s1, sums[1]) and bits_equal(w1, w[1])
    # a non-contiguous input is made contiguous
    Ft = F.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not Ft.is_contiguous() and bits_equal(soft_assign(Ft, S, c.grid), q)


# ---- soft_slic end to end ----
def slic_input(H, W, grid):
    img = torch.from_numpy(np.ascontiguousarray(synth("A", H, W))).permute(2, 0, 1).float() * 0.26
    return with_coords(img.unsqueeze(0).contiguous(), grid, 10.0)                # float32 [1, 5, H, W] on the CPU: one input for all


@pytest.mark.parametrize("H,W,grid", [(96, 128, (6, 8)), (37, 53, (3, 5)), (120, 160, (10, 10))])
def test_soft_slic_end_to_end(H, W, grid):
    x = slic_input(H, W, grid)
    K = grid[0] * grid[1]
    g = torch.Generator().manual_seed(H)
    Wq, Vc = torch.randn(1, 9, H, W, generator=g), torch.randn(1, 5, K, generator=g)

    def model(dtype):
        xl = x.to(dtype).requires_grad_(True)
        q, cen = R.soft_slic(xl, grid, max_iter=5)
        grad, = torch.autograd.grad((q * Wq.to(dtype)).sum() + (cen * Vc.to(dtype)).sum(), xl)
        return q.detach(), cen.detach(), grad

    q64, c64, g64 = model(torch.float64)
    q32, c32, g32 = model(torch.float32)
    xl = x.to(DEV).requires_grad_(True)
    q, cen = soft_slic(xl, grid, max_iter=5)
    grad, = torch.autograd.grad((q * Wq.to(DEV)).sum() + (cen * Vc.to(DEV)).sum(), xl)
    torch.cuda.synchronize()
    print("\nsoft_slic %dx%d grid %s" % (H, W, grid))
    hold("Q", q, q64, q32)
    hold("centres", cen, c64, c32)
    hold("grad features", grad, g64, g32)
    # the labels, wherever the model's two largest Q differ by more than twice the tolerance
    tol = max(8.0 * rel(q32, q64), FLOOR) * float(q64.abs().max())
    top = q64.topk(2, dim=1).values
    sure = (top[:, 0] - top[:, 1]) > 2.0 * tol
    left_out = 1.0 - float(sure.double().mean())
    lab, lab64 = soft_labels(q, grid).cpu(), R.soft_labels(q64, grid)
    print("labels: %.4f %% of the pixels left out, %d of the others differ" % (100.0 * left_out, int((lab != lab64)[sure].sum())))
    assert left_out <= 0.01
    assert bool((lab == lab64)[sure].all())
    # [C, H, W] in, no batch dimension out, the same bits
    q1, cen1 = soft_slic(x[0].to(DEV), grid, max_iter=5)
    assert q1.shape == (9, H, W) and cen1.shape == (5, K) and bits_equal(q1, q[0].detach()) and bits_equal(cen1, cen[0].detach())


# ---- the chain ----
def test_chain_into_pool_graph_crf_unpool():
    H, W, grid, Cn = 96, 128, (6, 8), 4
    K = grid[0] * grid[1]
    img = torch.from_numpy(np.ascontiguousarray(synth("A", H, W))).to(DEV)
    rgb = img.permute(2, 0, 1).float().contiguous()
    q, _ = soft_slic(with_coords(rgb * 0.26, grid, 10.0), grid, max_iter=5)
    lab = soft_labels(q, grid)
    assert lab.dtype == torch.int32 and int(lab.min()) >= 0 and int(lab.max()) < K
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV).float(), torch.arange(W, device=DEV).float(), indexing="ij")
    yxrgb, counts = superpixel_pool(torch.cat([torch.stack([yy, xx]), rgb]), lab, K, "mean", return_counts=True)
    graph = superpixel_graph(lab, K)
    table = label_overlap(lab, R.cell_labels(H, W, grid).to(DEV), K, K)
    assert table is not None
    logits = torch.randn(Cn, H, W, generator=torch.Generator().manual_seed(2)).to(DEV)
    un = -torch.log(superpixel_pool(torch.softmax(logits, dim=0), lab, K).clamp_min(1e-6))
    out = superpixel_unpool(superpixel_crf(un, graph, yxrgb, counts, max_iter=3), lab)
    assert out.shape == (Cn, H, W) and bool(torch.isfinite(out).all())


def test_reconstruction_loss_reaches_the_features():
    H, W, grid = 37, 53, (3, 5)
    F = slic_input(H, W, grid).to(DEV).requires_grad_(True)
    q, _ = soft_slic(F, grid, max_iter=3)
    loss = (soft_unpool(soft_pool(F, q, grid), q, grid) - F).pow(2).mean()
    loss.backward()
    assert F.grad is not None and F.grad.shape == F.shape and bool(torch.isfinite(F.grad).all()) and float(F.grad.abs().max()) > 0
