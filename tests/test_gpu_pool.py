"""Superpixel pooling on the MI355X (fast_slic_amd/pool.py, csrc/pool.hip) against the float64 numpy reference (tests/pool_ref.py):
sum / mean / max / counts / argmax / unpool on Slic label maps, noise maps, maps with -1 and labels >= K, edge shapes, many channels and
batches; the determinism properties bitwise; gradients; the get_mask_density cross-check; a non-default stream; non-finite containment;
and the Slic -> pool -> SimpleCRF -> unpool chain."""
import numpy as np
import pytest
import torch

import pool_ref as R
from fast_slic_amd.pool import superpixel_pool, superpixel_unpool

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_slic_cache = {}


def slic_labels(H, W, K, variant="A", seed=0):
    key = (H, W, K, variant, seed)
    if key not in _slic_cache:
        from fast_slic_amd import Slic
        from fast_slic_amd.synth import variant as synth
        _slic_cache[key] = Slic(num_components=K).iterate(synth(variant, H, W, seed=seed))
    return _slic_cache[key]


def features(shape, seed=0, kind="normal"):
    rng = np.random.default_rng(seed)
    if kind == "binary":
        return (rng.random(shape) < 0.5).astype(np.float32)
    return (rng.standard_normal(shape) * 3.0 + 0.5).astype(np.float32)


def pool_all(x, lab, K):
    """(sum, mean, max, counts) from the package, as numpy."""
    xt = torch.from_numpy(x).to(DEV)
    s, cnt = superpixel_pool(xt, lab, K, reduce="sum", return_counts=True)
    m, cnt2 = superpixel_pool(xt, lab, K, reduce="mean", return_counts=True)
    mx, cnt3 = superpixel_pool(xt, lab, K, reduce="max", return_counts=True)
    torch.cuda.synchronize()
    assert torch.equal(cnt, cnt2) and torch.equal(cnt, cnt3)
    return s.cpu().numpy(), m.cpu().numpy(), mx.cpu().numpy(), cnt.cpu().numpy()


def check_against_ref(x, lab, K, exact=False):
    """x [N, C, H, W] / [C, H, W]; lab numpy of the matching shape."""
    s, m, mx, cnt = pool_all(x, lab, K)
    X = x if x.ndim == 4 else x[None]
    Lb = lab if lab.ndim == 3 else lab[None]
    ref = R.pool(X, Lb, K)
    if x.ndim == 3:
        s, m, mx, cnt = s[None], m[None], mx[None], cnt[None]
    assert np.array_equal(cnt, ref["counts"]), "counts"
    err = np.abs(s.astype(np.float64) - ref["sum"])
    if exact:
        assert np.array_equal(s.astype(np.float64), ref["sum"]), "sum not exact (max error %g)" % err.max()
    else:
        bad = err > 4e-6 * ref["abs"]
        assert not bad.any(), "sum off at %d entries, worst %g of sum|x| %g" % (bad.sum(), err[bad].max(), ref["abs"][bad].max())
    c = cnt[:, None, :]
    want_mean = np.where(c > 0, s / np.maximum(c, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    assert np.array_equal(m.view(np.uint32), want_mean.view(np.uint32)), "mean != sum / count in f32"
    assert np.array_equal(mx.view(np.uint32), ref["max"].view(np.uint32)), "max"
    return ref


def max_argmax(x, lab, K):
    """The argmax the backward pass uses: gradient of sum(max) w.r.t. x, via the package, as flat indices per (n, c, k)."""
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    v = superpixel_pool(xt, lab, K, reduce="max")
    v.sum().backward()
    return xt.grad.cpu().numpy()


def check_argmax(x, lab, K, ref):
    g = max_argmax(x, lab, K)
    X = x if x.ndim == 4 else x[None]
    G = g if g.ndim == 4 else g[None]
    N, Cc, H, W = X.shape
    want = np.zeros_like(G)
    for n in range(N):
        for c in range(Cc):
            am = ref["argmax"][n, c]
            sel = am >= 0
            want[n, c].reshape(-1)[am[sel]] = 1.0
    assert np.array_equal(G, want), "max gradient is not on the lowest-index argmax (%d entries differ)" % int((G != want).sum())


# ---- agreement with the reference ----
def test_slic_1280x720_k1600_c21():
    lab = slic_labels(720, 1280, 1600)
    x = features((21, 720, 1280), 1)
    ref = check_against_ref(x, lab, 1600)
    check_argmax(x[:3], lab, 1600, R.pool(x[None, :3], lab[None], 1600))
    assert ref["counts"].sum() == (lab.view(np.uint16) < 1600).sum()


def test_slic_3840x2160_k6000():
    lab = slic_labels(2160, 3840, 6000, "B")
    x = features((8, 2160, 3840), 2)
    check_against_ref(x, lab, 6000)


def test_noise_map_k4096_batch():
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 4096, (3, 257, 300)).astype(np.int32)
    x = features((3, 3, 257, 300), 4)
    ref = check_against_ref(x, lab, 4096)
    check_argmax(x, torch.from_numpy(lab), 4096, ref)


def test_missing_and_out_of_range_labels():
    rng = np.random.default_rng(5)
    lab = rng.integers(-1, 60, (2, 131, 97)).astype(np.int16)
    lab[0, :20] = -1
    lab[1, :, 50:] = 59
    x = features((2, 5, 131, 97), 6)
    ref = check_against_ref(x, lab, 50)                        # 50..59 and -1: no segment
    assert ref["counts"][1, :].sum() < 131 * 97
    lab64 = rng.integers(-(1 << 40), 1 << 40, (2, 131, 97)).astype(np.int64)
    lab64[:, ::3] = rng.integers(0, 50, lab64[:, ::3].shape)
    check_against_ref(x, lab64, 50)


def test_k1_4k_binary_is_exact():
    lab = np.zeros((2160, 3840), np.int16)
    x = features((2, 2160, 3840), 7, "binary")
    check_against_ref(x, lab, 1, exact=True)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 721), (721, 1), (7, 65), (63, 63), (65, 7), (65, 721), (721, 63)])
def test_edge_shapes(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    lab = rng.integers(-1, 9, (2, H, W)).astype(np.int32)
    lab[:, : H // 2] = 3
    x = features((2, 3, H, W), H + W)
    ref = check_against_ref(x, lab, 8)
    check_argmax(x, lab, 8, ref)


@pytest.mark.parametrize("Cc", [1, 3, 21, 64, 257])
def test_channel_counts(Cc):
    lab = slic_labels(63, 130, 40)
    x = features((Cc, 63, 130), Cc)
    check_against_ref(x, lab, 40)


@pytest.mark.parametrize("N", [1, 3, 8])
def test_batch_sizes(N):
    labs = np.stack([slic_labels(72, 128, 30, seed=s) for s in range(N)])
    x = features((N, 4, 72, 128), N)
    ref = check_against_ref(x, labs, 30)
    check_argmax(x, labs, 30, ref)


def test_label_dtypes_agree():
    lab = slic_labels(96, 160, 50)
    x = torch.from_numpy(features((5, 96, 160), 9)).to(DEV)
    u = lab.view(np.uint16).astype(np.int64)
    forms = [lab, torch.from_numpy(lab), torch.from_numpy(lab).to(DEV), torch.from_numpy(np.where(u < 65535, u, -1).astype(np.int32)),
             torch.from_numpy(np.where(u < 65535, u, 1 << 33)).to(DEV)]
    for reduce in ("sum", "mean", "max"):
        outs = [superpixel_pool(x, f, 50, reduce=reduce) for f in forms]
        for o in outs[1:]:
            assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32)), reduce


# ---- determinism, bitwise ----
def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_determinism(reduce):
    labs = np.stack([slic_labels(720, 1280, 1600, seed=s) for s in range(3)])
    x = torch.from_numpy(features((3, 21, 720, 1280), 11)).to(DEV)
    first = bits(superpixel_pool(x, labs, 1600, reduce=reduce))
    for _ in range(3):                                                     # repeated calls
        assert np.array_equal(bits(superpixel_pool(x, labs, 1600, reduce=reduce)), first)
    for n in range(3):                                                     # a frame alone == the frame inside the batch
        assert np.array_equal(bits(superpixel_pool(x[n], labs[n], 1600, reduce=reduce)), first[n])
    perm = np.random.default_rng(12).permutation(1600)                     # label ids permuted: the output permuted the same way
    u = labs.view(np.uint16).astype(np.int64)
    plabs = np.where(u < 1600, perm[np.minimum(u, 1599)], -1).astype(np.int32)
    got = bits(superpixel_pool(x, plabs, 1600, reduce=reduce))
    assert np.array_equal(got[:, :, perm], first)
    y = x.clone()                                                          # other channels changed: channel 4 unchanged
    y[:, :4] = torch.randn_like(y[:, :4]) * 1e6
    y[:, 5:] = -y[:, 5:] * 3.0
    assert np.array_equal(bits(superpixel_pool(y, labs, 1600, reduce=reduce))[:, 4], first[:, 4])
    assert np.array_equal(bits(superpixel_pool(x[:, 4:5], labs, 1600, reduce=reduce))[:, 0], first[:, 4])


# ---- unpool ----
def test_unpool_is_an_exact_gather():
    rng = np.random.default_rng(13)
    lab = rng.integers(-1, 40, (3, 65, 77)).astype(np.int16)
    lab[0, 5] = 45                                                         # >= K
    vals = features((3, 6, 37), 14)
    vals[0, 0, 3] = -0.0
    for lt in (lab, torch.from_numpy(lab.astype(np.int64)).to(DEV)):
        got = superpixel_unpool(torch.from_numpy(vals).to(DEV), lt, fill=-7.25).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), R.unpool(vals, lab.astype(np.int64), -7.25).view(np.uint32))
    got2 = superpixel_unpool(torch.from_numpy(vals[1]).to(DEV), lab[1]).cpu().numpy()    # [C, K] -> [C, H, W], fill 0
    assert np.array_equal(got2, R.unpool(vals[1], lab[1], 0.0))
    lab4 = rng.integers(0, 37, (2, 3, 5)).astype(np.int32)                 # H * W % 4 != 0: the scalar store path
    assert np.array_equal(superpixel_unpool(torch.from_numpy(vals[:2]).to(DEV), lab4).cpu().numpy(), R.unpool(vals[:2], lab4, 0.0))


# ---- gradients ----
def test_sum_and_mean_gradients_are_the_table():
    lab = slic_labels(72, 128, 30)
    x = torch.from_numpy(features((4, 72, 128), 15)).to(DEV).requires_grad_(True)
    g = torch.from_numpy(features((4, 30), 16)).to(DEV)
    v, cnt = superpixel_pool(x, lab, 30, reduce="sum", return_counts=True)
    (gx,) = torch.autograd.grad(v, x, g)
    assert torch.equal(gx, superpixel_unpool(g, lab))
    v = superpixel_pool(x, lab, 30, reduce="mean")
    (gx,) = torch.autograd.grad(v, x, g)
    want = R.unpool((g / cnt.clamp_min(1).float()).cpu().numpy(), lab, 0.0)
    assert np.array_equal(gx.cpu().numpy(), want)


def test_max_gradient_on_first_raster_pixel_of_constant_features():
    lab = slic_labels(72, 128, 30)
    lab = lab.copy()
    lab[:3, :3] = -1
    x = torch.full((2, 72, 128), 2.5, device=DEV, requires_grad=True)
    v = superpixel_pool(x, lab, 30, reduce="max")
    g = torch.arange(60, dtype=torch.float32, device=DEV).reshape(2, 30) + 1
    (gx,) = torch.autograd.grad(v, x, g)
    want = np.zeros((2, 72, 128), np.float32)
    flat = lab.view(np.uint16).reshape(-1)
    for k in range(30):
        idx = np.flatnonzero(flat == k)
        if idx.size:
            want[:, idx[0] // 128, idx[0] % 128] = g[:, k].cpu().numpy()
    assert np.array_equal(gx.cpu().numpy(), want)


def test_pool_unpool_chain_gradient():
    lab = slic_labels(72, 128, 30)
    x = torch.from_numpy(features((3, 72, 128), 17)).to(DEV).requires_grad_(True)
    w = torch.from_numpy(features((3, 72, 128), 18)).to(DEV)
    y = superpixel_unpool(superpixel_pool(x, lab, 30, reduce="sum"), lab)
    (y * w).sum().backward()
    # d/dx sum(w * unpool(pool(x))) = unpool(pool(w))
    assert torch.equal(x.grad, superpixel_unpool(superpixel_pool(w, lab, 30, reduce="sum"), lab))
    v = torch.from_numpy(features((3, 30), 19)).to(DEV).requires_grad_(True)
    superpixel_unpool(v, lab, fill=3.0).mul(w).sum().backward()
    assert torch.equal(v.grad, superpixel_pool(w, lab, 30, reduce="sum"))


def test_under_deterministic_algorithms():
    lab = slic_labels(72, 128, 30)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        outs = []
        for _ in range(2):
            x = torch.from_numpy(features((3, 72, 128), 20)).to(DEV).requires_grad_(True)
            loss = sum(superpixel_pool(x, lab, 30, reduce=r).square().sum() for r in ("sum", "mean", "max"))
            loss = loss + superpixel_unpool(superpixel_pool(x, lab, 30), lab).sum()
            loss.backward()
            outs.append((loss.detach().cpu(), x.grad.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    finally:
        torch.use_deterministic_algorithms(prev)
    assert torch.are_deterministic_algorithms_enabled() == prev


# ---- against the reference's own mask density ----
def test_matches_get_mask_density():
    from fast_slic_amd import Slic
    from fast_slic_amd.synth import variant
    slic = Slic(num_components=1600)
    lab = slic.iterate(variant("A", 720, 1280))
    mask = (np.random.default_rng(21).random((720, 1280)) * 256).astype(np.uint8)
    mask[:100] = 255
    dens = slic.slic_model.get_mask_density(mask, lab)
    s = superpixel_pool(torch.from_numpy(mask.astype(np.float32)).to(DEV)[None], lab, 1600, reduce="sum")[0].cpu().numpy()
    members = slic.slic_model.cluster_array["num_members"].astype(np.int64)
    mine = np.minimum(255, s.astype(np.int64) // np.maximum(members, 1)).astype(np.uint8)
    assert np.array_equal(mine, dens)


# ---- streams ----
def test_on_a_non_default_stream():
    labs = np.stack([slic_labels(720, 1280, 1600, seed=s) for s in range(2)])
    lab_dev = torch.from_numpy(labs).to(DEV)
    x_host = features((2, 21, 720, 1280), 22)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(DEV)
    with torch.cuda.stream(st):
        x = torch.from_numpy(x_host).to(DEV, non_blocking=False).mul_(1.0)          # produced on st
        lab_s = lab_dev.clone()
        v = superpixel_pool(x, lab_s, 1600, reduce="mean")
        mx = superpixel_pool(x, lab_s, 1600, reduce="max")
        up = superpixel_unpool(v, lab_s, fill=-1.0)
        out = (v.to("cpu", non_blocking=False), mx.cpu(), up[:, :2].cpu())
    st.synchronize()
    ref = R.pool(x_host, labs, 1600)
    cnt = ref["counts"][:, None, :]
    assert np.allclose(out[0].numpy(), np.where(cnt > 0, ref["sum"] / np.maximum(cnt, 1), 0), rtol=1e-5, atol=1e-5)
    assert np.array_equal(out[1].numpy().view(np.uint32), ref["max"].view(np.uint32))
    assert np.array_equal(out[2].numpy(), R.unpool(out[0].numpy()[:, :2], labs, -1.0))


# ---- non-finite containment ----
def test_non_finite_stays_in_its_segment():
    lab = slic_labels(72, 128, 30)
    x = features((3, 72, 128), 23)
    flat = lab.view(np.uint16).reshape(-1)
    hit = {0: 7, 1: 12, 2: 7}
    vals = {0: np.nan, 1: np.inf, 2: -np.inf}
    for c, k in hit.items():
        p = np.flatnonzero(flat == k)[len(np.flatnonzero(flat == k)) // 2]
        x[c].reshape(-1)[p] = vals[c]
    clean = x.copy()
    for c, k in hit.items():
        clean[c].reshape(-1)[flat == k] = 0.0
    s, m, mx, cnt = pool_all(x, lab, 30)
    ref = R.pool(clean[None], lab[None], 30)
    for c in range(3):
        keep = np.arange(30) != hit[c]
        err = np.abs(s[c, keep].astype(np.float64) - ref["sum"][0, c, keep])
        assert (err <= 4e-6 * ref["abs"][0, c, keep]).all()
        assert np.array_equal(mx[c, keep], ref["max"][0, c, keep])


# ---- Slic -> pool -> SimpleCRF -> unpool ----
def test_end_to_end_crf_chain():
    from fast_slic_amd import Slic
    from fast_slic_amd.crf import SimpleCRF
    from fast_slic_amd.synth import variant
    H, W, K, Cc = 240, 320, 200, 4
    slic = Slic(num_components=K)
    lab = slic.iterate(variant("A", H, W, seed=1))
    logits = torch.from_numpy(features((Cc, H, W), 24)).to(DEV)
    proba = torch.softmax(logits, dim=0)
    p = superpixel_pool(proba, lab, K, reduce="mean")
    cnt = superpixel_pool(proba, lab, K, reduce="sum", return_counts=True)[1].cpu().numpy()
    pn = p.cpu().numpy()
    live = cnt > 0
    assert np.allclose(pn[:, live].sum(0), 1.0, atol=1e-5)
    pn[:, ~live] = 1.0 / Cc
    crf = SimpleCRF(Cc, K)
    f = crf.push_slic_frame(slic)
    f.set_proba(np.ascontiguousarray(pn))
    crf.initialize()
    crf.inference(5)
    q = f.get_inferred()
    out = superpixel_unpool(torch.from_numpy(q).to(DEV), lab).cpu().numpy()
    assert np.array_equal(out, R.unpool(q, lab, 0.0))
    seg = out.argmax(0)
    assert seg.shape == (H, W)
