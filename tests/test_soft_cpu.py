"""CPU tests of soft superpixel assignment (fast_slic_amd/soft.py, the fslic_hip_soft_* entries): the float64 model of tests/soft_ref.py
against a brute-force formulation with dense K-way distances, the model's gradients (gradcheck), every argument error refused before
any device work -- ValueError in Python, FSLIC_E_INVALID from the C ABI before its first HIP call -- and the agreement of the header,
EXPORTS and the library on the new names.  No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

import soft_ref as R
from fast_slic_amd import _binding as B
from fast_slic_amd.soft import soft_assign, soft_labels, soft_pool, soft_slic, soft_unpool, with_coords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fslic_hip_soft_assign", "fslic_hip_soft_assign_backward", "fslic_hip_soft_pool", "fslic_hip_soft_unpool", "fslic_hip_soft_dot"]


def test_package_import_stays_torch_free():
    code = "import sys, fast_slic_amd; assert 'torch' not in sys.modules; import fast_slic_amd.soft; assert 'torch' in sys.modules"
    subprocess.check_call([sys.executable, "-c", code])


# ---- the model against a brute-force formulation: dense K-way distances, masked to the 3 x 3 neighbourhood ----
def brute(F, S, grid):
    """dense Q [N, K, H * W]: the softmax of -|F_p - S_k|^2 over the cells k within one cell of the pixel's own."""
    N, Cc, H, W = F.shape
    gh, gw = grid
    cy, cx = R.cells(H, W, grid)
    pcy, pcx = cy.view(H, 1).expand(H, W).reshape(-1), cx.view(1, W).expand(H, W).reshape(-1)
    kcy, kcx = torch.arange(gh * gw) // gw, torch.arange(gh * gw) % gw
    near = ((kcy.view(-1, 1) - pcy.view(1, -1)).abs() <= 1) & ((kcx.view(-1, 1) - pcx.view(1, -1)).abs() <= 1)      # [K, HW]
    D = ((F.reshape(N, Cc, 1, H * W) - S.reshape(N, Cc, -1, 1)) ** 2).sum(1)                                         # [N, K, HW]
    D = torch.where(near.unsqueeze(0), D, torch.full_like(D, float("inf")))
    return torch.softmax(-D, dim=1), near


def dense_of(Q, grid):
    """the model's Q [N, 9, H, W] scattered to [N, K, H * W]"""
    N, _, H, W = Q.shape
    k, ok = R.slots(H, W, grid)
    out = torch.zeros(N, grid[0] * grid[1], H * W, dtype=Q.dtype)
    for j in range(9):
        out.scatter_add_(1, k[j].reshape(1, 1, -1).expand(N, 1, H * W), (Q[:, j] * ok[j]).reshape(N, 1, H * W))
    return out


@pytest.mark.parametrize("H,W,grid", [(13, 17, (3, 4)), (9, 9, (1, 1))])
def test_model_against_brute_force(H, W, grid):
    g = torch.Generator().manual_seed(H * W)
    N, Cc, K = 2, 3, grid[0] * grid[1]
    F = torch.randn(N, Cc, H, W, generator=g, dtype=torch.float64) * 0.5
    S = R.soft_pool(F, R.one_hot(N, H, W), grid) + 0.2 * torch.randn(N, Cc, K, generator=g, dtype=torch.float64)
    Q = R.soft_assign(F, S, grid)
    k, ok = R.slots(H, W, grid)
    assert bool((Q[:, ~ok] == 0).all()) and torch.allclose(Q.sum(1), torch.ones(N, H, W, dtype=torch.float64), atol=1e-14)
    Qd, near = brute(F, S, grid)
    assert torch.allclose(dense_of(Q, grid), Qd, atol=1e-13)
    assert int(near.sum(0).min()) >= 1 and int(near.sum(0).max()) <= 9
    # pooling, unpooling and the labels as dense sums over the pixels and the superpixels
    sums, weights = R.soft_pool_raw(F, Q, grid)
    assert torch.allclose(sums, torch.einsum("nkp,ncp->nck", Qd, F.reshape(N, Cc, -1)), atol=1e-12)
    assert torch.allclose(weights, Qd.sum(2), atol=1e-12)
    mean = R.soft_pool(F, Q, grid)
    assert torch.allclose(mean, sums / weights.unsqueeze(1), atol=1e-12)
    V = torch.randn(N, Cc, K, generator=g, dtype=torch.float64)
    assert torch.allclose(R.soft_unpool(V, Q, grid), torch.einsum("nkp,nck->ncp", Qd, V).reshape(N, Cc, H, W), atol=1e-12)
    assert torch.equal(R.soft_labels(Q, grid).reshape(N, -1), Qd.argmax(1).to(torch.int32))
    # the one-hot Q: the cell means, and the cell map
    lab = R.cell_labels(H, W, grid)
    cellmean = torch.stack([F[:, :, lab == c].mean(-1) for c in range(K)], -1)
    assert torch.allclose(R.soft_pool(F, R.one_hot(N, H, W), grid), cellmean, atol=1e-13)
    assert torch.equal(R.soft_labels(R.one_hot(N, H, W), grid), lab.unsqueeze(0).expand(N, H, W))
    # soft_slic is those steps in a row
    Q2, S2 = R.soft_slic(F, grid, max_iter=2)
    S_ = cellmean
    for _ in range(2):
        Qb, _ = brute(F, S_, grid)
        S_ = torch.einsum("nkp,ncp->nck", Qb, F.reshape(N, Cc, -1)) / Qb.sum(2).unsqueeze(1)
    assert torch.allclose(S2, S_, atol=1e-12) and torch.allclose(dense_of(Q2, grid), brute(F, S_, grid)[0], atol=1e-12)


def test_package_labels_and_coords_match_the_model():
    """soft_labels and with_coords are torch ops: they run on CPU tensors, ties included"""
    g = torch.Generator().manual_seed(5)
    for H, W, grid in [(13, 17, (3, 4)), (9, 9, (1, 1)), (5, 64, (1, 7))]:
        Q = torch.rand(2, 9, H, W, generator=g)
        Q[0, :, 0, :] = 0.25                                                     # ties: the lowest valid slot wins
        Q[1, 5, 1, :] = Q[1, 4, 1, :] = 2.0
        assert torch.equal(soft_labels(Q, grid), R.soft_labels(Q, grid))
        assert torch.equal(soft_labels(Q[1], grid), R.soft_labels(Q, grid)[1])
        assert soft_labels(Q, grid).dtype == torch.int32
        F = torch.randn(2, 3, H, W, generator=g)
        x = with_coords(F, grid, 10.0)
        assert x.shape == (2, 5, H, W) and torch.equal(x[:, :3], F)
        assert torch.allclose(x.double(), R.with_coords(F.double(), grid, 10.0), rtol=1e-6, atol=0)
        assert torch.equal(with_coords(F[0], grid, 10.0), x[0])


# ---- the model's gradients ----
def test_model_gradcheck():
    H, W, grid = 7, 9, (2, 3)
    g = torch.Generator().manual_seed(3)
    F = (torch.randn(1, 2, H, W, generator=g, dtype=torch.float64) * 0.5).requires_grad_(True)
    S = torch.randn(1, 2, 6, generator=g, dtype=torch.float64).mul(0.3).requires_grad_(True)
    Q = torch.rand(1, 9, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    V = torch.randn(1, 2, 6, generator=g, dtype=torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda f, s: R.soft_assign(f, s, grid), (F, S))
    assert torch.autograd.gradcheck(lambda f, q: R.soft_pool_raw(f, q, grid), (F, Q))
    assert torch.autograd.gradcheck(lambda v, q: R.soft_unpool(v, q, grid), (V, Q))

    def composed(f):                                  # soft_slic, then SSN's reconstruction from its own centres
        q, cen = R.soft_slic(f, grid, max_iter=2)
        return q, cen, R.soft_unpool(R.soft_pool(f, q, grid), q, grid)

    assert torch.autograd.gradcheck(composed, (F,), fast_mode=True)


def test_model_gradients_are_the_stated_formulas():
    """gd_j = -Q_j (gQ_j - sum_i gQ_i Q_i); gF = 2 sum_j gd_j (F - S_j); gS[c, k] = -2 sum_p gd_{j_k(p)}(p) (F[c, p] - S[c, k])"""
    H, W, grid = 13, 17, (3, 4)
    g = torch.Generator().manual_seed(11)
    F = (torch.randn(2, 3, H, W, generator=g, dtype=torch.float64) * 0.5).requires_grad_(True)
    S = (R.soft_pool(F.detach(), R.one_hot(2, H, W), grid) + 0.2 * torch.randn(2, 3, 12, generator=g, dtype=torch.float64)).requires_grad_(True)
    gQ = torch.randn(2, 9, H, W, generator=g, dtype=torch.float64)
    Q = R.soft_assign(F, S, grid)
    gF, gS = torch.autograd.grad((Q * gQ).sum(), (F, S))
    Qv, Fv, Sv = Q.detach(), F.detach(), S.detach()
    k, ok = R.slots(H, W, grid)
    gd = -Qv * (gQ - (gQ * Qv).sum(1, keepdim=True))
    wantF, wantS = torch.zeros_like(Fv), torch.zeros_like(Sv)
    for j in range(9):
        diff = Fv - Sv[:, :, k[j].reshape(-1)].reshape(Fv.shape)
        t = (gd[:, j] * ok[j]).unsqueeze(1) * diff
        wantF += 2 * t
        wantS.index_add_(2, k[j].reshape(-1), -2 * t.reshape(2, 3, -1))
    assert torch.allclose(gF, wantF, atol=1e-12) and torch.allclose(gS, wantS, atol=1e-12)


# ---- argument errors in Python: refused before any device work (the tensors are on the CPU) ----
F = torch.zeros(2, 3, 5, 7)
S = torch.zeros(2, 3, 6)
Q = torch.zeros(2, 9, 5, 7)
G = (2, 3)


@pytest.mark.parametrize("grid,match", [
    ((6, 3), "gh <= H"), ((2, 8), "gw <= W"), ((0, 3), "1 <= gh"), ((2, -1), "1 <= gh"), ((2.0, 3), "integers"), ((True, 3), "integers"),
    (6, "pair"), ((2, 3, 1), "pair"), (None, "pair"),
])
def test_bad_grid(grid, match):
    for call in (lambda: soft_assign(F, S, grid), lambda: soft_pool(F, Q, grid), lambda: soft_unpool(S, Q, grid),
                 lambda: soft_labels(Q, grid), lambda: soft_slic(F, grid), lambda: with_coords(F, grid, 1.0)):
        with pytest.raises(ValueError, match=match):
            call()


def test_too_many_cells():
    big = torch.zeros(1, 300, 300)
    with pytest.raises(ValueError, match="at most 65534"):
        soft_slic(big, (256, 256))
    with pytest.raises(ValueError, match="at most 65534"):
        soft_labels(torch.zeros(9, 300, 300), (300, 300))
    with pytest.raises(ValueError, match="at most 65534"):
        soft_slic(big, (257, 255))                                            # 65535 cells
    with pytest.raises(ValueError, match="ROCm GPU"):                         # 65534 cells pass the check
        soft_slic(torch.zeros(1, 302, 302), (217, 302))


@pytest.mark.parametrize("features,centres,match", [
    (F.double(), S, "float32"), (F.numpy(), S, "torch tensor"), (torch.zeros(5, 7), S, r"\[C, H, W\]"), (torch.zeros(0, 3, 5, 7), S, "empty"),
    (F, S.double(), "float32"), (F, torch.zeros(3, 6), r"\[N, C, K\]"), (F, torch.zeros(2, 3, 5), "shape"), (F, torch.zeros(1, 3, 6), "shape"),
    (F, torch.zeros(2, 4, 6), "channels"), (F[0], S, r"\[C, K\]"), (F, None, "torch tensor"),
])
def test_bad_assign_arguments(features, centres, match):
    with pytest.raises(ValueError, match=match):
        soft_assign(features, centres, G)


@pytest.mark.parametrize("features,q,match", [
    (F.half(), Q, "float32"), (F, Q.double(), "float32"), (F, torch.zeros(2, 8, 5, 7), "shape"), (F, torch.zeros(1, 9, 5, 7), "shape"),
    (F, torch.zeros(2, 9, 7, 5), "shape"), (F, Q[0], r"\[N, 9, H, W\]"), (F[0], Q, r"\[9, H, W\]"), (F, [1], "torch tensor"),
])
def test_bad_pool_arguments(features, q, match):
    with pytest.raises(ValueError, match=match):
        soft_pool(features, q, G)


@pytest.mark.parametrize("values,q,match", [
    (S.double(), Q, "float32"), (S, Q.double(), "float32"), (torch.zeros(2, 3, 5), Q, "shape"), (torch.zeros(3, 3, 6), Q, "shape"),
    (S[0], Q, r"\[N, C, K\]"), (S, Q[0], r"\[C, K\]"), (S, torch.zeros(2, 8, 5, 7), "shape"), (S, torch.zeros(5, 7), r"\[9, H, W\]"),
    (S, None, r"\[9, H, W\]"),
])
def test_bad_unpool_arguments(values, q, match):
    with pytest.raises(ValueError, match=match):
        soft_unpool(values, q, G)


def test_other_bad_arguments():
    with pytest.raises(ValueError, match="max_iter"):
        soft_slic(F, G, max_iter=-1)
    with pytest.raises(ValueError, match="max_iter"):
        soft_slic(F, G, max_iter=2.5)
    with pytest.raises(ValueError, match="compactness"):
        with_coords(F, G, "10")
    with pytest.raises(ValueError, match="shape"):
        soft_labels(torch.zeros(2, 8, 5, 7), G)


def test_cpu_tensors_are_refused_after_every_other_check():
    for call in (lambda: soft_assign(F, S, G), lambda: soft_pool(F, Q, G), lambda: soft_unpool(S, Q, G), lambda: soft_slic(F, G),
                 lambda: soft_assign(F[0], S[0], G), lambda: soft_pool(F[0], Q[0], G, normalize=False, return_weights=True)):
        with pytest.raises(ValueError, match="ROCm GPU"):
            call()


# ---- the C ABI: FSLIC_E_INVALID before any HIP call (a bogus non-NULL pointer is never touched) ----
P = C.c_void_p(0x1000)
NUL = None
BAD_GEOMETRY = [dict(device=-1), dict(N=0), dict(Cc=0), dict(H=0), dict(W=-3), dict(H=1 << 16, W=1 << 15), dict(gh=6), dict(gw=8),
                dict(gh=0), dict(gw=0), dict(H=300, W=300, gh=256, gw=256), dict(H=70000, W=2, gh=65535, gw=1)]


def lib():
    return B.load_library()


def geometry(kw):
    a = dict(device=0, N=1, Cc=3, H=5, W=7, gh=2, gw=3)
    a.update({k: v for k, v in kw.items() if k in a})
    return [a["device"], NUL, a["N"], a["Cc"], a["H"], a["W"], a["gh"], a["gw"]]


ENTRIES = {      # name -> its pointer arguments, the optional ones marked
    "soft_assign": [("features", True), ("centres", True), ("q", True)],
    "soft_assign_backward": [("features", True), ("centres", True), ("q", True), ("grad_q", True), ("grad_d", True), ("grad_features", True)],
    "soft_pool": [("features", True), ("q", True), ("centres", False), ("sums", True), ("weights", False)],
    "soft_unpool": [("values", True), ("q", True), ("out", True)],
    "soft_dot": [("a", True), ("b", True), ("bias", False), ("out", True)],
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_capi_refuses(name):
    fn = getattr(lib(), "fslic_hip_" + name)
    ptrs = ENTRIES[name]
    for kw in BAD_GEOMETRY:
        assert fn(*geometry(kw), *[P for _ in ptrs]) == B.FSLIC_E_INVALID, kw
        assert lib().fslic_hip_last_error()
    for i, (arg, required) in enumerate(ptrs):
        if required:
            assert fn(*geometry({}), *[NUL if j == i else P for j in range(len(ptrs))]) == B.FSLIC_E_INVALID, arg
            assert b"NULL" in lib().fslic_hip_last_error()


# ---- the header, EXPORTS and the library agree on the new names ----
def test_header_exports_and_library_agree():
    src = open(os.path.join(ROOT, "include", "fslic_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(fslic_hip_\w+)\s*\(", src)) if n.startswith("fslic_hip_soft_"))
    assert declared == sorted(NAMES)
    assert sorted(n for n in B.EXPORTS if n.startswith("fslic_hip_soft_")) == sorted(NAMES)
    for n in NAMES:
        f = getattr(lib(), n)
        assert f.restype is C.c_int and len(f.argtypes) == 8 + len(ENTRIES[n[len("fslic_hip_"):]])
