"""Soft superpixel assignment on the MI355X at the edges tests/test_gpu_soft.py does not reach (its shapes have K <= 32, N = 3 and
features of randn * 0.5), against the same float64 model (tests/soft_ref.py) under the same measured rule err <= max(8 b, 2^-20)
(`hold`); every other comparison is == on the bits, and every figure is printed before it is asserted (pytest -s).

A. Launch sizes.  A soft kernel runs one 256-thread block per item; the runtime supports no launch of 2^32 or more threads in a
   dimension, so from 2^24 blocks on the launches are issued in slices (soft.h).  The pixel kernels at N = 2^24 + 3 frames of 1 x 2
   pixels and k_soft_pool at 257 frames of K = 65534 are compared with the same frames run in smaller batches.
B. Geometry: the 64-bit cell division (H * gh past 2^32) on each axis, the last shape below it, one-pixel cells and K = 65534.
   Forcing SoftGrid::wide to 0 in soft.hip makes the 70000-row and the 70000-column case fail (tried once on a scratch build).
C. Exact zeros: a superpixel of weight +0.0, a Q that underflows to +0.0 on a valid slot, and features offset by +1000.
D. Footprint: a NaN or a far value in one centre, one feature pixel or one Q entry perturbed: nothing outside the stated pixels and
   superpixels changes a bit, and an invalid slot stays +0.0 whatever centre 0 (the index an invalid slot gathers from) holds."""
import pytest
import torch

import soft_ref as R
from fast_slic_amd.pool import superpixel_pool, superpixel_unpool
from fast_slic_amd.soft import _pool_raw, soft_assign, soft_labels, soft_pool, soft_slic, soft_unpool
from soft_cases import DEV, Case, bits_equal, gpu_stages, hold, model_stages, rel

pytestmark = pytest.mark.gpu
N = 2
_cache = {}


def case(H, W, grid, Cc, tag=None, adjust=None):
    key = (H, W, grid, Cc, tag)
    if key not in _cache:
        _cache[key] = Case(H, W, grid, Cc, n=N, adjust=adjust)
    return _cache[key]


def differing(a, b):
    """the number of elements whose bits differ"""
    assert a.shape == b.shape
    return int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())


def hold_all(c, got):
    failures = []
    for name in sorted(got):
        try:
            hold(name, got[name], c.ref[torch.float64][name], c.ref[torch.float32][name])
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "; ".join(failures)


def invalid_slots_are_plus_zero(got, H, W, grid, n=N):
    _, ok = R.slots(H, W, grid)
    bad = (~ok).to(DEV).unsqueeze(0).expand(n, 9, H, W)
    for name in ("assign Q", "pool gQ", "unpool gQ"):
        assert bool((got[name][bad].view(torch.int32) == 0).all()), name + " is not +0.0 on an invalid slot"


def valid_q(n, H, W, grid, g):
    """a random Q on the device: positive on the valid slots, +0.0 on the others, every pixel's slots sum to 1"""
    _, ok = R.slots(H, W, grid)
    q = (torch.rand(n, 9, H, W, generator=g, device=DEV) + 0.05) * ok.to(DEV).unsqueeze(0)
    return q / q.sum(1, keepdim=True)


# ---- A. launch sizes ----
PIXEL_SLICE = 1 << 20


@pytest.mark.parametrize("frames", [(1 << 24) - 1, (1 << 24) + 3])
def test_pixel_kernels_past_one_launch(frames):
    """H W = 2: one block per frame, so `frames` blocks in every pixel kernel (2^24 - 1 is the last count of a single launch, 2^24 + 3
    the first past it by a ragged amount) and 2 * frames items in the pools behind the gradients.  A frame's results do not depend on
    its batch position, so the batch must equal its slices of 2^20 frames bit for bit."""
    H, W, grid, Cc, K = 1, 2, (1, 2), 1, 2
    g = torch.Generator(device=DEV).manual_seed(frames)
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV)
    t = {"F": rnd(frames, Cc, H, W) * 0.5, "S": rnd(frames, Cc, K) * 0.5, "V": rnd(frames, Cc, K), "gQ": rnd(frames, 9, H, W),
         "gS": rnd(frames, Cc, K), "gW": rnd(frames, K), "gO": rnd(frames, Cc, H, W), "Q": valid_q(frames, H, W, grid, g)}
    got = gpu_stages(t, grid)
    torch.cuda.synchronize()
    wrong = dict.fromkeys(got, 0)
    for lo in range(0, frames, PIXEL_SLICE):
        part = gpu_stages({k: v[lo:lo + PIXEL_SLICE] for k, v in t.items()}, grid)
        for name in got:
            wrong[name] += differing(part[name], got[name][lo:lo + PIXEL_SLICE])
        del part
    print("\n%d frames of 1 x 2 against slices of 2^20 frames, elements that differ: %s" % (frames, wrong))
    # the first and the last 1024 frames against the model
    ends = torch.cat([torch.arange(1024), torch.arange(frames - 1024, frames)])
    sub = {k: v[ends.to(DEV)].cpu() for k, v in t.items()}
    ref64 = model_stages({k: v.double() for k, v in sub.items()}, grid)
    ref32 = model_stages(sub, grid)
    failures = []
    for name in sorted(got):
        try:
            hold(name, got[name][ends.to(DEV)], ref64[name], ref32[name])
        except AssertionError as e:
            failures.append(str(e))
    invalid_slots_are_plus_zero({k: got[k][-1024:] for k in ("assign Q", "pool gQ", "unpool gQ")}, H, W, grid, n=1024)
    del got, t
    torch.cuda.empty_cache()
    assert not any(wrong.values()), "the batch differs from its slices: %s" % wrong
    assert not failures, "; ".join(failures)


def test_pool_kernel_past_one_launch():
    """k_soft_pool at 257 * 65534 = 16 842 238 items (2^24 = 16 777 216; 256 frames are 512 items short of it), one-pixel cells."""
    H, W, grid, Cc, frames, step = 2, 32767, (2, 32767), 1, 257, 32
    K = grid[0] * grid[1]
    g = torch.Generator(device=DEV).manual_seed(257)
    F = torch.randn(frames, Cc, H, W, generator=g, device=DEV)
    S = torch.randn(frames, Cc, K, generator=g, device=DEV)
    Q = valid_q(frames, H, W, grid, g)
    sums, weights = soft_pool(F, Q, grid, normalize=False, return_weights=True)
    centred = _pool_raw(F, Q, grid, centres=S, weights=False)[0]
    wrong = {"sums": 0, "weights": 0, "centred": 0}
    for lo in range(0, frames, step):
        s, w = soft_pool(F[lo:lo + step], Q[lo:lo + step], grid, normalize=False, return_weights=True)
        c = _pool_raw(F[lo:lo + step], Q[lo:lo + step], grid, centres=S[lo:lo + step], weights=False)[0]
        wrong["sums"] += differing(s, sums[lo:lo + step])
        wrong["weights"] += differing(w, weights[lo:lo + step])
        wrong["centred"] += differing(c, centred[lo:lo + step])
    print("\n257 frames of K = 65534 against slices of 32 frames, elements that differ: %s" % wrong)
    # the one-hot Q on integer features: sums below 2^24 are exact in any order, so soft_pool is superpixel_pool bit for bit
    del Q, sums, weights, centred
    Fi = torch.randint(0, 256, (frames, Cc, H, W), generator=g, device=DEV).float()
    q1 = torch.zeros(frames, 9, H, W, device=DEV)
    q1[:, 4] = 1.0
    labn = R.cell_labels(H, W, grid).to(DEV).unsqueeze(0).expand(frames, H, W).contiguous()
    hs, hw = soft_pool(Fi, q1, grid, normalize=False, return_weights=True)
    want, counts = superpixel_pool(Fi, labn, K, "sum", return_counts=True)
    hard = {"sums": differing(hs, want), "weights": int((hw != counts.float()).sum())}
    print("one-hot Q against superpixel_pool, elements that differ: %s" % hard)
    del F, S, Fi, q1, labn, hs, hw, want, counts
    torch.cuda.empty_cache()
    assert not any(wrong.values()), "the batch differs from its slices: %s" % wrong
    assert not any(hard.values()), "the one-hot Q differs from superpixel_pool: %s" % hard


# ---- B. geometry edges ----
# wide on each axis (70000 * 65534 > 2^32); 65537 * 65534 = 4 294 901 758, the 32-bit product's last shape; one-pixel cells, the second
# with K = 65534 in two dimensions
EDGE_SHAPES = [(70000, 1, (65534, 1)), (1, 70000, (1, 65534)), (65537, 1, (65534, 1)), (9, 11, (9, 11)), (2, 32767, (2, 32767))]


@pytest.mark.parametrize("Cc", [1, 3, 20])
@pytest.mark.parametrize("H,W,grid", EDGE_SHAPES)
def test_geometry_edges_against_the_model(H, W, grid, Cc):
    c = case(H, W, grid, Cc)
    got = c.gpu()
    torch.cuda.synchronize()
    print("\n%dx%d grid %s C=%d" % (H, W, grid, Cc))
    hold_all(c, got)
    invalid_slots_are_plus_zero(got, H, W, grid)


@pytest.mark.parametrize("H,W,grid", EDGE_SHAPES)
def test_geometry_edges_one_hot_q_is_hard_pooling(H, W, grid):
    K = grid[0] * grid[1]
    g = torch.Generator().manual_seed(H + W)
    lab = R.cell_labels(H, W, grid).to(DEV)
    labn = lab.unsqueeze(0).expand(N, H, W).contiguous()
    q = R.one_hot(N, H, W, torch.float32).to(DEV)
    assert torch.equal(soft_labels(q, grid), labn) and torch.equal(soft_labels(q[0], grid), lab)
    F = torch.randint(0, 256, (N, 3, H, W), generator=g).float().to(DEV)                # integer sums below 2^24: exact in any order
    sums, weights = soft_pool(F, q, grid, normalize=False, return_weights=True)
    want, counts = superpixel_pool(F, labn, K, "sum", return_counts=True)
    print("\n%dx%d grid %s one-hot: sums differ at %d, weights at %d" % (H, W, grid, differing(sums, want), int((weights != counts.float()).sum())))
    assert bits_equal(sums, want) and torch.equal(weights, counts.float())
    assert bits_equal(soft_pool(F, q, grid), want / counts.float().unsqueeze(1))
    V = torch.randn(N, 3, K, generator=g).to(DEV)
    assert bits_equal(soft_unpool(V, q, grid), superpixel_unpool(V, labn))


# ---- C. exact zeros and underflow ----
def test_strip_with_a_superpixel_of_weight_zero():
    """2 x 12, grid (1, 3), one channel: columns 0 - 5 are +1000 and 6 - 11 are -1000 (frame 1: the negative).  The cell means are
    (1000, 0, -1000); every pixel is 0 away from an outer centre and 10^6 from the middle one, so the middle superpixel's weight is
    exactly 0 after the first round, its centre keeps its value, and every sum is one of integers below 2^24."""
    H, W, grid = 2, 12, (1, 3)
    row = torch.cat([torch.full((6,), 1000.0), torch.full((6,), -1000.0)])
    x = torch.stack([row.expand(H, W), -row.expand(H, W)]).unsqueeze(1).contiguous()                  # [2, 1, 2, 12]
    g = torch.Generator().manual_seed(12)
    Wq, Vc = torch.randn(2, 9, H, W, generator=g), torch.randn(2, 1, 3, generator=g)

    def model(dtype):
        xl = x.to(dtype).requires_grad_(True)
        q, cen = R.soft_slic(xl, grid, max_iter=3)
        grad, = torch.autograd.grad((q * Wq.to(dtype)).sum() + (cen * Vc.to(dtype)).sum(), xl)
        return q.detach(), cen.detach(), grad

    q64, c64, g64 = model(torch.float64)
    q32, c32, g32 = model(torch.float32)
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64).view(2, 1, 1)
    assert torch.equal(c64, sign * torch.tensor([1000.0, 0.0, -1000.0], dtype=torch.float64)) and bool(torch.isfinite(g64).all())
    xd = x.to(DEV)
    # the first round: the cell means, Q, and the pooled means with their weights
    q0 = R.one_hot(2, H, W, torch.float32).to(DEV)
    means = soft_pool(xd, q0, grid)
    q = soft_assign(xd, means, grid)
    pooled, weights = soft_pool(xd, q, grid, normalize=True, return_weights=True)
    print("\nstrip: cell means %s weights %s pooled %s" % (means[0, 0].tolist(), weights[0].tolist(), pooled[0, 0].tolist()))
    assert torch.equal(means.cpu().double(), c64)
    assert bool((weights[:, 1].view(torch.int32) == 0).all()), "the middle weight is not +0.0"
    assert torch.equal(weights.cpu(), torch.tensor([[12.0, 0.0, 12.0]] * 2))
    assert bool((pooled[:, :, 1] == 0).all()) and bool(torch.isfinite(pooled).all())
    assert torch.equal(pooled.cpu()[:, :, [0, 2]].double(), c64[:, :, [0, 2]])
    # soft_slic, three rounds, with the gradient
    xl = xd.clone().requires_grad_(True)
    qs, cen = soft_slic(xl, grid, max_iter=3)
    grad, = torch.autograd.grad((qs * Wq.to(DEV)).sum() + (cen * Vc.to(DEV)).sum(), xl)
    torch.cuda.synchronize()
    print("centres %s" % cen.detach()[0, 0].tolist())
    failures = []
    for name, a, r64, r32 in (("Q", qs, q64, q32), ("grad features", grad, g64, g32)):
        try:
            hold(name, a, r64, r32)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "; ".join(failures)
    assert torch.equal(cen.detach().cpu().double(), c64), "the centres differ from the model's"
    assert bool(torch.isfinite(qs).all()) and bool(torch.isfinite(cen).all()) and bool(torch.isfinite(grad).all())


def test_isolated_centre_underflows_to_zero():
    """one-pixel cells, random centres, centre k0 moved 10^3 away in every channel: its distance is past 10^6 at every pixel, so its Q
    is +0.0 wherever a slot names it (in float64 as well: the exponent is far past -745) and so is its weight."""
    H, W, grid, Cc, k0 = 9, 11, (9, 11), 3, 4 * 11 + 5

    def away(c):
        c.S[:, :, k0] += 1000.0

    c = case(H, W, grid, Cc, "away", away)
    got = c.gpu()
    torch.cuda.synchronize()
    print("\n%dx%d grid %s C=%d, centre %d moved away" % (H, W, grid, Cc, k0))
    k, ok = R.slots(H, W, grid)
    names = (ok & (k == k0)).to(DEV).unsqueeze(0).expand(N, 9, H, W)
    assert int(names.sum()) == 9 * N
    assert bool((c.ref[torch.float64]["assign Q"][names.cpu()] == 0).all())
    print("slots that name centre %d: %d, of them not +0.0: %d; weights of it not +0.0: %d" % (
        k0, int(names.sum()), int((got["assign Q"][names].view(torch.int32) != 0).sum()),
        int((got["pool weights"][:, k0].view(torch.int32) != 0).sum())))
    failures = []
    if not bool((got["assign Q"][names].view(torch.int32) == 0).all()):
        failures.append("Q is not +0.0 on the slots of the centre that is far away")
    if not bool((got["pool weights"][:, k0].view(torch.int32) == 0).all()):
        failures.append("the weight of the centre that is far away is not +0.0")
    assert bool(all(torch.isfinite(v).all() for v in got.values()))
    hold_all(c, got)
    invalid_slots_are_plus_zero(got, H, W, grid)
    assert not failures, "; ".join(failures)


def test_features_offset_by_1000():
    """+1000 on the features and the centres: the distances are the same, their float32 rounding is not; the bound follows the float32
    model's own loss b, printed beside the b of the case without the offset.  It was expected to grow; measured, it moves both ways
    within a factor of 2 (assign Q 1.9e-7 -> 1.1e-7, pool sums 8.5e-7 -> 9.2e-7): F - S is exact for neighbours near 1000."""
    H, W, grid, Cc = 37, 53, (3, 5), 3

    def offset(c):
        c.F += 1000.0
        c.S += 1000.0

    plain, c = case(H, W, grid, Cc), case(H, W, grid, Cc, "offset", offset)
    print("\n%dx%d grid %s C=%d: b without / with the offset" % (H, W, grid, Cc))
    for name in sorted(c.ref[torch.float64]):
        print("%-16s b %.3e / %.3e" % (name, rel(plain.ref[torch.float32][name], plain.ref[torch.float64][name]),
                                       rel(c.ref[torch.float32][name], c.ref[torch.float64][name])))
    got = c.gpu()
    torch.cuda.synchronize()
    hold_all(c, got)
    invalid_slots_are_plus_zero(got, H, W, grid)


# ---- D. footprint ----
FOOT_SHAPES = [(37, 53, (3, 5)), (5, 64, (1, 7))]
PIXEL_NAMES = ("assign Q", "assign gF", "unpool out", "pool gF", "pool gQ", "unpool gQ")          # what the pixel kernels write


def near(H, W, grid, k0):
    """bool [H, W]: the pixels whose nine slots include cell k0, and bool [K]: the superpixels whose window holds such a pixel"""
    cy, cx = R.cells(H, W, grid)
    ky, kx = k0 // grid[1], k0 % grid[1]
    pix = ((cy - ky).abs() <= 1).view(H, 1) & ((cx - kx).abs() <= 1).view(1, W)
    ay, ax = torch.arange(grid[0]), torch.arange(grid[1])
    sup = ((ay - ky).abs() <= 2).view(-1, 1) & ((ax - kx).abs() <= 2).view(1, -1)
    return pix, sup.reshape(-1)


def with_centre(c, k0, value):
    """the case's tensors on the device with entry k0 of every [.., K] table that a pixel kernel gathers from set to `value`: the
    centres, the values, and the two gradients that k_soft_dot reads as its table and its bias"""
    t = c.tensors(DEV)
    for name in ("S", "V", "gS", "gW"):
        t[name] = t[name].clone()
        t[name][..., k0] = value
    return t


def outside_is_untouched(c, clean, got, k0):
    """every per-pixel result outside k0's pixels, and every centre gradient of a superpixel whose window holds none of them"""
    pix, sup = near(c.H, c.W, c.grid, k0)
    out, far = (~pix).to(DEV), (~sup).to(DEV)
    assert int(out.sum()) > 0
    wrong = {name: differing(got[name][:, :, out], clean[name][:, :, out]) for name in PIXEL_NAMES}
    wrong["assign gS"] = differing(got["assign gS"][:, :, far], clean["assign gS"][:, :, far])
    wrong["unpool gV"] = differing(got["unpool gV"], clean["unpool gV"])                 # the values take no part in their own gradient
    print("centre %d: elements that differ outside its pixels: %s" % (k0, wrong))
    assert not any(wrong.values()), "centre %d reaches outside its 3 x 3 cell window: %s" % (k0, wrong)


@pytest.mark.parametrize("H,W,grid", FOOT_SHAPES)
def test_nan_in_centre_zero_and_in_an_interior_centre(H, W, grid):
    """An invalid slot gathers from index 0 and discards what it read: with NaN in centre 0 every invalid slot is still +0.0 at every
    pixel, the pixels of cell 0's window included, and nothing outside that window changes.  The same for an interior centre."""
    c = case(H, W, grid, 3)
    clean = c.gpu()
    interior = (grid[0] // 2) * grid[1] + grid[1] // 2
    print("\n%dx%d grid %s" % (H, W, grid))
    for k0 in (0, interior):
        got = gpu_stages(with_centre(c, k0, float("nan")), grid)
        torch.cuda.synchronize()
        pix, _ = near(H, W, grid, k0)
        assert bool(torch.isnan(got["assign Q"][:, 4][:, pix.to(DEV)]).all())            # the poison did arrive where it belongs
        invalid_slots_are_plus_zero(got, H, W, grid)
        outside_is_untouched(c, clean, got, k0)


@pytest.mark.parametrize("H,W,grid", FOOT_SHAPES)
def test_centre_zero_nearer_than_every_valid_centre(H, W, grid):
    """Every centre but centre 0 is moved by +100 in every channel, so at a pixel with an invalid slot the discarded distance to
    centre 0 is smaller than every valid one by about 3 * 10^4: were it to enter the minimum, every exponential would underflow."""
    def shift(c):
        c.S[:, :, 1:] += 100.0

    c = case(H, W, grid, 3, "shift", shift)
    got = c.gpu()
    torch.cuda.synchronize()
    print("\n%dx%d grid %s, centre 0 nearer than every valid centre" % (H, W, grid))
    assert bool(all(torch.isfinite(v).all() for v in got.values()))
    hold_all(c, got)
    invalid_slots_are_plus_zero(got, H, W, grid)
    assert float((got["assign Q"].sum(1) - 1).abs().max()) <= 1e-6
    # and centre 0 moved along with the others changes nothing outside its window
    t = c.tensors(DEV)
    t["S"] = t["S"].clone()
    t["S"][:, :, 0] += 100.0
    moved = gpu_stages(t, grid)
    out = (~near(H, W, grid, 0)[0]).to(DEV)
    wrong = {name: differing(moved[name][:, :, out], got[name][:, :, out]) for name in ("assign Q", "assign gF")}
    print("centre 0 moved: elements that differ outside its pixels: %s" % wrong)
    assert not any(wrong.values())


@pytest.mark.parametrize("H,W,grid", FOOT_SHAPES)
def test_one_feature_pixel_perturbed(H, W, grid):
    """Only that pixel's Q changes, and only the sums and weights of the superpixels its valid slots name."""
    c = case(H, W, grid, 3)
    n0, c0, y0, x0 = 1, 2, H // 2, W // 2
    F, S = c.F.to(DEV), c.S.to(DEV)
    F2 = F.clone()
    F2[n0, c0, y0, x0] += 0.25
    q, q2 = soft_assign(F, S, grid), soft_assign(F2, S, grid)
    (s, w), (s2, w2) = (soft_pool(f, qq, grid, normalize=False, return_weights=True) for f, qq in ((F, q), (F2, q2)))
    k, ok = R.slots(H, W, grid)
    named = torch.zeros(c.K, dtype=torch.bool)
    named[k[:, y0, x0][ok[:, y0, x0]]] = True
    here = torch.zeros(N, H, W, dtype=torch.bool)
    here[n0, y0, x0] = True
    here, named = here.to(DEV), named.to(DEV)
    qd = (q.view(torch.int32) != q2.view(torch.int32)).any(1)                            # [N, H, W]
    sd = (s.view(torch.int32) != s2.view(torch.int32)).any(1)                            # [N, K]
    wd = w.view(torch.int32) != w2.view(torch.int32)
    print("\n%dx%d grid %s: pixels whose Q changed %d, superpixels whose sums changed %d (weights %d) of %d named" %
          (H, W, grid, int(qd.sum()), int(sd.sum()), int(wd.sum()), int(named.sum())))
    assert bool(qd[here].all()) and not bool(qd[~here].any())
    assert not bool(sd[0].any()) and not bool(wd[0].any())
    assert bool(sd[n0].any()) and not bool(sd[n0][~named].any()) and not bool(wd[n0][~named].any())


@pytest.mark.parametrize("H,W,grid", FOOT_SHAPES)
def test_one_q_entry_perturbed(H, W, grid):
    """Slot j of pixel p: in soft_pool only superpixel k_j(p) changes, in soft_unpool only pixel p.  An invalid slot's entry is never
    read: NaN there changes nothing at all."""
    c = case(H, W, grid, 3)
    n0, j0, y0, x0 = 1, 5, H // 2, W // 2
    k, ok = R.slots(H, W, grid)
    assert bool(ok[j0, y0, x0])
    k0 = int(k[j0, y0, x0])
    t = c.tensors(DEV)
    clean = gpu_stages(t, grid)
    t2 = dict(t)
    t2["Q"] = t["Q"].clone()
    t2["Q"][n0, j0, y0, x0] += 0.125
    got = gpu_stages(t2, grid)
    sd = (got["pool sums"].view(torch.int32) != clean["pool sums"].view(torch.int32)).any(1)           # [N, K]
    wd = got["pool weights"].view(torch.int32) != clean["pool weights"].view(torch.int32)
    ud = (got["unpool out"].view(torch.int32) != clean["unpool out"].view(torch.int32)).any(1)         # [N, H, W]
    print("\n%dx%d grid %s: superpixels whose sums changed %s, weights %s, pixels whose unpooled value changed %s" %
          (H, W, grid, sd.nonzero().tolist(), wd.nonzero().tolist(), ud.nonzero().tolist()))
    assert sd.nonzero().tolist() == [[n0, k0]] and wd.nonzero().tolist() == [[n0, k0]]
    assert ud.nonzero().tolist() == [[n0, y0, x0]]
    t3 = dict(t)
    t3["Q"] = torch.where(ok.to(DEV).unsqueeze(0), t["Q"], torch.full_like(t["Q"], float("nan")))
    t3["gQ"] = torch.where(ok.to(DEV).unsqueeze(0), t["gQ"], torch.full_like(t["gQ"], float("nan")))
    got = gpu_stages(t3, grid)
    wrong = {name: differing(got[name], clean[name]) for name in clean}
    print("NaN on the invalid slots of Q and gQ: elements that differ: %s" % wrong)
    assert not any(wrong.values())
