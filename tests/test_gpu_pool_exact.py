"""Superpixel pooling on the MI355X, bit for bit: the fixed-point accumulator of the sum (fix_add / fix_to_float of csrc/pool.hip)
against the exact model of tests/pool_ref.py over every limb, shift, carry, rounding and the inf cut; the max keys on negative,
zero, subnormal and extreme values; the second trip of both grid-stride loops; and K = 65534 with the int16 map.  Every comparison
is on bits or integers.

The sum cases run as "case tables": case i is a list of at most T tile partials (f32 bit patterns) and owns label i; its partial t is
the single pixel at slot i (row i // 64, column i % 64) of tile t, so a frame of T tiles (side by side, or stacked) holds 1024 cases
and more cases go into further frames of the batch.  A slot a case does not use is either unlabelled or holds +0.0 under the case's
label (alternating), which adds nothing.  This layout depends on the kernel's tile of 16 rows x 64 columns, as exact_pool does."""
import numpy as np
import pytest
import torch

import pool_ref as R
from fast_slic_amd.pool import superpixel_pool, superpixel_unpool
from test_gpu_pool import check_against_ref, check_argmax, slic_labels

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIGN = 0x80000000
FLT_MAX = 0x7F7FFFFF
INF = 0x7F800000
SLOTS = 1024                      # cases per frame: the pixels of one 16 x 64 tile
ORIENTS = ("wide", "tall")


def p2(e):
    """Bits of 2^e, -126 <= e <= 127."""
    assert -126 <= e <= 127
    return (e + 127) << 23


def scaled(m, e):
    """Bits of the f32 that is exactly m * 2^e."""
    return R.f32_bits_of_scaled(m, e)


def neg(case):
    return [b ^ SIGN for b in case]


def both_signs(cases):
    return cases + [neg(c) for c in cases]


# ---- the case table ----
def table_frames(cases, orient, T, perm_seed=None):
    """-> bits uint32 [F, H, W], labels int32 [F, H, W] and the pixel count of every case."""
    F = (len(cases) + SLOTS - 1) // SLOTS
    vals = np.zeros((F * SLOTS, T), np.uint32)
    lab = np.full((F * SLOTS, T), -1, np.int32)
    rng = np.random.default_rng(perm_seed)
    for i, c in enumerate(cases):
        assert len(c) <= T
        order = np.arange(T) if perm_seed is None else rng.permutation(T)      # the tile that holds each partial
        lab[i, order[:len(c)]] = i % SLOTS
        vals[i, order[:len(c)]] = c
        rest = order[len(c):]
        lab[i, rest[(rest + i) % 2 == 0]] = i % SLOTS                           # +0.0 under the case's label; the others unlabelled
    counts = (lab >= 0).sum(1)[:len(cases)]
    vals, lab = vals.reshape(F, 16, 64, T), lab.reshape(F, 16, 64, T)
    if orient == "wide":                                                        # [F, 16, 64 * T]: tile t is columns 64 t ..
        vals, lab = vals.transpose(0, 1, 3, 2).reshape(F, 16, 64 * T), lab.transpose(0, 1, 3, 2).reshape(F, 16, 64 * T)
    else:                                                                       # [F, 16 * T, 64]: tile t is rows 16 t ..
        vals, lab = vals.transpose(0, 3, 1, 2).reshape(F, 16 * T, 64), lab.transpose(0, 3, 1, 2).reshape(F, 16 * T, 64)
    return np.ascontiguousarray(vals), np.ascontiguousarray(lab), counts


def run_table(cases, orient, T=8, perm_seed=None, noise_first=False):
    """-> (sum bits, mean bits, counts) per case, from the package."""
    vals, lab, _ = table_frames(cases, orient, T, perm_seed)
    x = vals.view(np.float32)[:, None]
    if orient == "tall":
        lab = lab.astype(np.int16)                                              # the int16 map in one orientation, int32 in the other
    if noise_first:                                                             # frame 0 of the batch is noise
        rng = np.random.default_rng(99)
        x = np.concatenate([(rng.standard_normal(x[:1].shape) * 1e20).astype(np.float32), x])
        lab = np.concatenate([rng.integers(-1, SLOTS, lab[:1].shape).astype(lab.dtype), lab])
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    s, cnt = superpixel_pool(xt, lab, SLOTS, reduce="sum", return_counts=True)
    m, cnt2 = superpixel_pool(xt, lab, SLOTS, reduce="mean", return_counts=True)
    torch.cuda.synchronize()
    assert torch.equal(cnt, cnt2)
    first = 1 if noise_first else 0
    n = len(cases)
    return (s.cpu().numpy()[first:, 0].reshape(-1).view(np.uint32)[:n], m.cpu().numpy()[first:, 0].reshape(-1).view(np.uint32)[:n],
            cnt.cpu().numpy()[first:].reshape(-1)[:n])


def model_bits(cases):
    return np.array([R.exact_sum_bits(c) for c in cases], np.uint32)


def mean_bits(sum_bits, counts):
    """f32(sum) / f32(count) in f32, 0 for an empty segment, as tests/test_gpu_pool.py states the mean."""
    with np.errstate(all="ignore"):
        q = sum_bits.view(np.float32) / np.maximum(counts, 1).astype(np.float32)
    return np.where(counts > 0, q, np.float32(0)).astype(np.float32).view(np.uint32)


def assert_bits(got, want, cases, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        lines = ["case %d %s: got %08x, want %08x" % (i, ["%08x" % b for b in cases[i]], got[i], want[i]) for i in bad[:8]]
        raise AssertionError("%s: %d of %d cases differ\n%s" % (what, bad.size, len(cases), "\n".join(lines)))


def check_table(cases, T=8, **kw):
    """Both orientations of the table against the model: sum, mean and counts."""
    want = model_bits(cases)
    for orient in ORIENTS:
        s, m, cnt = run_table(cases, orient, T, **kw)
        want_cnt = table_frames(cases, orient, T, kw.get("perm_seed"))[2]
        assert np.array_equal(cnt, want_cnt), "%s: counts" % orient
        assert_bits(s, want, cases, "%s: sum" % orient)
        assert_bits(m, mean_bits(want, want_cnt), cases, "%s: mean" % orient)
    return want


# ---- one partial per case: every exponent field, so every limb and every shift inside a limb ----
def single_partial_cases():
    rng = np.random.default_rng(31)
    cases = []
    for ex in range(0, 255):
        for mant in (0x000000, 0x7FFFFF, 0x000001, 0x400000, int(rng.integers(2, 0x7FFFFF))):
            for sign in (0, 1):
                cases.append([(sign << 31) | (ex << 23) | mant])
    return cases


def test_single_partial_walks_every_limb_and_shift():
    cases = single_partial_cases()
    want = check_table(cases)
    p = np.array([c[0] for c in cases], np.uint32)
    ex = (p >> np.uint32(23)) & np.uint32(0xFF)
    same = ex >= 127 - 73                                   # bit 0 of the mantissa at 2^-96 or above: unchanged
    gone = ex < 127 - 96                                    # below 2^-96, subnormals and zeros: +0.0
    assert np.array_equal(want[same], p[same]) and not want[gone].any()
    cut = ~same & ~gone                                     # in between: truncated to a multiple of 2^-96, towards zero
    v, w = p[cut].view(np.float32).astype(np.float64), want[cut].view(np.float32).astype(np.float64)
    assert np.array_equal(w, np.trunc(v * 2.0 ** 96) * 2.0 ** -96) and (w != v).any() and (w == v).any()
    assert (ex[cut].min(), ex[cut].max(), ex.max()) == (31, 53, 254)


def test_order_of_tiles_and_noise_frame_do_not_change_a_bit():
    cases = single_partial_cases() + rounding_cases()[::7]
    want = model_bits(cases)
    for orient in ORIENTS:
        assert_bits(run_table(cases, orient, perm_seed=41)[0], want, cases, "%s, tiles permuted" % orient)
        assert_bits(run_table(cases, orient, perm_seed=42, noise_first=True)[0], want, cases, "%s, after a noise frame" % orient)


# ---- cancellation across tiles ----
def test_cancellation_across_tiles():
    rng = np.random.default_rng(32)
    cases, exact_c = [], []
    for ea in range(-90, 128):
        a = p2(ea) | int(rng.integers(0, 1 << 23))
        for gap in (40, 52, 73, 97, 130, 200):
            if ea - gap < -126:
                continue
            c = p2(ea - gap) | int(rng.integers(0, 1 << 23)) | (int(rng.integers(0, 2)) << 31)
            for case in ([a, a ^ SIGN, c], [c, a ^ SIGN, a], [a ^ SIGN, c, a]):
                cases.append(case)
                exact_c.append(c if ea - gap - 23 >= -96 else None)
        cases.append([a, a ^ SIGN])
        exact_c.append(0)
        cases.append([a, a ^ SIGN, a, a ^ SIGN, a ^ SIGN, a])
        exact_c.append(0)
    for n in range(1, 9):
        cases.append([SIGN] * n)                                               # only -0.0: +0.0
        exact_c.append(0)
    want = check_table(cases)
    known = np.array([e is not None for e in exact_c])
    assert np.array_equal(want[known], np.array([e for e in exact_c if e is not None], np.uint32))
    assert (want >> np.uint32(31)).any() and known.sum() > 2000                # negative totals are among them


# ---- carries and borrows ----
def carry_cases():
    cases = []
    for pos in range(0, 201):                              # position of the mantissa's bit 0 in the accumulator: every limb, every offset
        e = pos - 96
        if e + 23 <= 126:
            cases.append([scaled(0xFFFFFF, e)] * 7 + [scaled(7, e)])           # 7 * 2^24 * 2^e: the carry runs through the mantissa's limbs
            cases.append([scaled(0xFFFFFF, e)] * 8)
        for gap in (33, 65, 100, 160):                     # 2^(e + gap) - 2^e: a borrow through the limbs in between
            if e >= -96 and e + gap <= 127:
                cases.append([p2(e + gap), p2(e) ^ SIGN])
                cases.append([p2(e + gap), p2(e) ^ SIGN, p2(e + gap - 1) ^ SIGN])
                cases.append([p2(e + gap) ^ SIGN, p2(e), p2(e), p2(e + gap)])
    return both_signs(cases)


def test_carries_and_borrows_through_several_limbs():
    check_table(carry_cases())


def test_nine_partials_straddling_a_limb_boundary():
    # 8 tiles of 0xFFFFFF * 2^e and one of 2^(e - 24), for every e that puts the mantissa across two limbs
    cases = []
    for pos in range(0, 201):
        e = pos - 96
        if pos % 32 >= 9 and e + 23 <= 124 and e - 24 >= -126:
            cases.append([scaled(0xFFFFFF, e)] * 8 + [p2(e - 24)])
            cases.append([scaled(0xFFFFFF, e)] * 4 + neg([scaled(0xFFFFFF, e)] * 4) + [p2(e - 24)])
    assert len(cases) > 200
    check_table(both_signs(cases), T=9)


# ---- the one rounding, with the leading bit at every position of the 224 ----
def rounding_cases():
    cases = []
    for lead in range(0, 24):                              # fewer than 24 bits: nothing to round
        cases.append([p2(lead - 96)] + ([scaled((1 << lead) - 1, -96)] if lead else []))
    for q in range(-96, 104):                              # s = 2^q; the leading bit is at 24 + q + 96 (25 for the last pattern)
        st = p2(max(-96, q - 70))                          # a sticky bit at the bottom of the accumulator or 70 binades down
        down, up, ones = [scaled(1 << 24, q), p2(q)], [scaled((1 << 24) + 2, q), p2(q)], [scaled(0xFFFFFF, q + 1), p2(q)]
        cases += [down, up, ones]                          # ties: to the even 2^24 s; to the even (2^24 + 4) s; into the next binade
        cases += [down + [st], up + [st], ones + [st]]     # the sticky bit decides
        cases += [down + [st ^ SIGN], up + [st ^ SIGN], ones + [st ^ SIGN]]     # just below the tie
        cases += [[scaled(1 << 24, q), p2(q), p2(q)], [scaled((1 << 24) + 2, q), p2(q) ^ SIGN]]
    return both_signs(cases)


def test_rounding_at_every_leading_bit_position():
    cases = rounding_cases()
    want = check_table(cases)
    half = len(cases) // 2
    q = -96 + 50                                           # spot check of what the model says, at s = 2^-46
    i = 24 + 50 * 11
    assert cases[i] == [scaled(1 << 24, q), p2(q)]
    assert [int(w) for w in want[i:i + 11]] == [
        scaled(1 << 24, q), scaled((1 << 24) + 4, q), scaled(1 << 25, q),
        scaled((1 << 24) + 2, q), scaled((1 << 24) + 4, q), scaled(1 << 25, q),
        scaled(1 << 24, q), scaled((1 << 24) + 2, q), scaled(0xFFFFFF, q + 1),
        scaled((1 << 24) + 2, q), scaled(1 << 24, q)]
    assert np.array_equal(want[half:], want[:half] ^ np.uint32(SIGN))


# ---- the inf cut ----
def test_overflow_cut():
    big = p2(127)
    cases = [
        [big, big],                                        # 2^128: inf
        [big, big, big ^ SIGN],                            # the running value passes 2^128 and comes back
        [big] * 8,
        [big] * 4 + [big ^ SIGN] * 4,
        [big] * 4 + [big ^ SIGN] * 3,
        [FLT_MAX, p2(103)],                                # FLT_MAX + half an ulp: ties upward, inf
        [FLT_MAX, scaled((1 << 24) - 1, 79)],              # FLT_MAX + 2^103 - 2^79: FLT_MAX
        [FLT_MAX, p2(103), p2(-96) ^ SIGN],                # one unit of the accumulator below the cut
        [FLT_MAX, p2(102), p2(102)],
        [FLT_MAX, p2(102), p2(101), p2(-96)],
        [FLT_MAX] * 8,
        [FLT_MAX] * 5 + [FLT_MAX ^ SIGN] * 3,
        [FLT_MAX] * 4 + [FLT_MAX ^ SIGN] * 3,
        [FLT_MAX, FLT_MAX, FLT_MAX ^ SIGN, p2(103), p2(-90) ^ SIGN],
    ]
    want = check_table(both_signs(cases))
    n = len(cases)
    assert [int(w) for w in want[:n]] == [INF, big, INF, 0, big, INF, FLT_MAX, FLT_MAX, INF, FLT_MAX, INF, INF, FLT_MAX, FLT_MAX]
    assert np.array_equal(want[n:], np.where(want[:n] == 0, 0, want[:n] ^ np.uint32(SIGN)))


# ---- many pixels per partial: integers in [-1023, 1023] times one power of two per (tile, label, channel) ----
def integer_features(rng, lab, Cc, K, e_lo=-126, e_hi=107, tile=(16, 64)):
    """lab [N, H, W] -> float32 [N, Cc, H, W]: below 2^20 * 2^e inside a tile, so every order of adding a tile's pixels is exact, and
    1024 tiles of 1023 * 2^107 stay finite."""
    N, H, W = lab.shape
    ntx = (W + tile[1] - 1) // tile[1]
    tid = (np.arange(H) // tile[0])[:, None] * ntx + (np.arange(W) // tile[1])[None, :]
    l64, ok = R.valid_labels(lab, K)
    col = np.where(ok, l64, 0)
    x = np.empty((N, Cc, H, W), np.float32)
    for n in range(N):
        for c in range(Cc):
            e = rng.integers(e_lo, e_hi + 1, (int(tid.max()) + 1, K))
            x[n, c] = np.ldexp(rng.integers(-1023, 1024, (H, W)).astype(np.float32), e[tid, col[n]])
    return x


def check_exact_pool(x, lab, K):
    """sum, mean and counts of the package against exact_pool (which also checks that every tile partial is an f32)."""
    want = R.exact_pool(x, lab, K)
    xt = torch.from_numpy(x).to(DEV)
    s, cnt = superpixel_pool(xt, lab, K, reduce="sum", return_counts=True)
    m = superpixel_pool(xt, lab, K, reduce="mean")
    torch.cuda.synchronize()
    l64, ok = R.valid_labels(lab, K)
    want_cnt = np.stack([np.bincount(l64[n][ok[n]], minlength=K) for n in range(lab.shape[0])])
    assert np.array_equal(cnt.cpu().numpy(), want_cnt), "counts"
    got = s.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want), "sum: %d of %d entries differ" % ((got != want).sum(), want.size)
    want_mean = mean_bits(want.reshape(-1), np.repeat(want_cnt[:, None], x.shape[1], 1).reshape(-1)).reshape(want.shape)
    assert np.array_equal(m.cpu().numpy().view(np.uint32), want_mean), "mean"
    return want


@pytest.mark.parametrize("K,top", [(40, 40), (3000, 3000)])
def test_many_pixels_per_partial(K, top):
    rng = np.random.default_rng(33 + K)
    lab = rng.integers(-1, top + 2, (2, 64, 256)).astype(np.int32)              # -1, K and K + 1: no segment
    x = integer_features(rng, lab, 3, K)
    want = check_exact_pool(x, lab, K)
    sign = want[want != 0] >> np.uint32(31)
    assert sign.any() and not sign.all()                                        # totals of both signs


# ---- max and argmax on the values the suite's N(0.5, 3) never produces ----
def check_max(x, lab, K):
    """max against the reference on bits, and the argmax through the gradient; x [N, C, H, W] / [C, H, W]."""
    ref = R.pool(x if x.ndim == 4 else x[None], lab if lab.ndim == 3 else lab[None], K)
    got = superpixel_pool(torch.from_numpy(x).to(DEV), lab, K, reduce="max").cpu().numpy()
    assert np.array_equal(got.reshape(ref["max"].shape).view(np.uint32), ref["max"].view(np.uint32)), "max"
    check_argmax(x, lab, K, ref)
    return ref


def test_max_across_tiles_of_negative_zero_subnormal_and_extreme_values():
    rng = np.random.default_rng(34)
    cases = []
    for n in range(1, 9):                                                       # all negative: the cross-tile atomicMax decides
        for _ in range(40):
            cases.append([SIGN | int(rng.integers(1, 255)) << 23 | int(rng.integers(0, 1 << 23)) for _ in range(n)])
    cases += [[SIGN, 0], [0, SIGN], [SIGN, SIGN, 0, SIGN], [SIGN] * 8, [SIGN], [0, 0, SIGN], [SIGN, SIGN | 1], [SIGN | 1, SIGN],
              [1], [SIGN | 1], [SIGN | 1, SIGN | 2, SIGN | 0x7FFFFF], [1, 2, SIGN | 3], [0x7FFFFF, 0x00800000], [SIGN | 0x7FFFFF] * 3,
              [FLT_MAX], [SIGN | FLT_MAX], [SIGN | FLT_MAX] * 8, [SIGN | FLT_MAX, FLT_MAX], [SIGN | FLT_MAX, SIGN | (FLT_MAX - 1)],
              [FLT_MAX - 1, FLT_MAX, FLT_MAX], [SIGN | FLT_MAX, SIGN, SIGN | 1]]
    vals, lab, _ = table_frames(cases, "wide", 8)
    used = np.zeros(lab.shape, bool)                                            # unused slots stay unlabelled: a +0.0 there would win
    for i, c in enumerate(cases):
        used[0, i // 64, [64 * t + i % 64 for t in range(len(c))]] = True
    lab = np.where(used, lab, -1).astype(np.int32)
    x = vals.view(np.float32)[:, None]
    for xx, ll in ((x, lab), (np.ascontiguousarray(x.reshape(1, 1, 16, 8, 64).transpose(0, 1, 3, 2, 4)).reshape(1, 1, 128, 64),
                              np.ascontiguousarray(lab.reshape(1, 16, 8, 64).transpose(0, 2, 1, 3)).reshape(1, 128, 64))):
        ref = check_max(xx, ll, SLOTS)
        mx = ref["max"][0, 0].view(np.uint32)
        n0 = 8 * 40
        assert (mx[:n0] >> np.uint32(31)).all()                                 # every one of them negative
        assert [int(v) for v in mx[n0:n0 + 8]] == [0, 0, 0, SIGN, SIGN, 0, SIGN, SIGN]
        assert ref["argmax"][0, 0, n0 + 3] == ll.reshape(-1).tolist().index(n0 + 3)      # only -0.0: its first raster pixel


def test_max_inside_a_tile_of_negative_zero_subnormal_and_extreme_values():
    rng = np.random.default_rng(35)
    pools = [[SIGN], [SIGN, 0], [SIGN | 1, SIGN | 0x7FFFFF, SIGN | 0x00800000], [1, SIGN | 1, SIGN, 0x7FFFFF],
             [SIGN | FLT_MAX], [SIGN | FLT_MAX, FLT_MAX, 0], [SIGN | 0x3F800000, SIGN | 0x3F800001, SIGN | 0x40000000],
             [SIGN | FLT_MAX, SIGN | (FLT_MAX - 1)], [SIGN | 1], [0x7FFFFF, 0x7FFFFE]]
    K = len(pools)
    lab = np.repeat(np.repeat(rng.integers(-1, K, (2, 9, 11)), 5, 1), 13, 2)[:, :37, :139].astype(np.int16)     # blocks of 5 x 13
    lab[1] = rng.integers(-1, K, lab[1].shape)                                                                    # and a noise map
    l64 = lab.astype(np.int64)
    x = np.zeros((2, 2) + lab.shape[1:], np.uint32)
    for k, vals in enumerate(pools):
        draw = rng.choice(np.array(vals, np.uint32), size=x.shape)
        x = np.where((l64 == k)[:, None], draw, x)
    x = x.view(np.float32)
    ref = check_max(x, lab, K)
    assert [int(v) for v in ref["max"][0, 0].view(np.uint32)[:2]] == [SIGN, 0]
    first = np.flatnonzero(lab[0].reshape(-1) == 0)[0]
    assert ref["argmax"][0, 0, 0] == first and ref["argmax"][1, 1, 0] == np.flatnonzero(lab[1].reshape(-1) == 0)[0]


def test_max_gradient_of_constant_negative_features_goes_to_the_lowest_index():
    lab = slic_labels(72, 128, 30).copy()
    lab[:3, :3] = -1
    x = np.full((2, 72, 128), -2.5, np.float32)
    ref = check_max(x, lab, 30)
    flat = lab.view(np.uint16).reshape(-1)
    for k in range(30):
        idx = np.flatnonzero(flat == k)
        assert ref["argmax"][0, 0, k] == (idx[0] if idx.size else -1)


# ---- the second trip of the two grid-stride loops, and the upper K ----
def band_labels(rng, H, W, K):
    """Bands of 23 rows with ragged edges, noise pixels and unlabelled ones: between one and many labels per tile."""
    lab = ((np.arange(H)[:, None] // 23 + np.arange(W)[None, :]) % K).astype(np.int32)
    noise = rng.random((H, W))
    lab = np.where(noise < 0.05, rng.integers(0, K, (H, W)), lab)
    lab = np.where(noise > 0.97, rng.integers(-2, 0, (H, W)) * 40000, lab)      # -80000 and -40000: no segment
    lab[5000:5100] = -1
    lab[H // 2: H // 2 + 64] = rng.integers(0, K, (64, W))
    return lab.astype(np.int32)


def test_more_tile_items_than_one_grid_holds():
    # 40 001 tiles of 16 x 3 pixels, one chunk of channels: 40 001 items for the 32 768 wavefronts of the largest grid, so some
    # wavefronts take a second item and build a second label list
    H, W, K = 640005, 3, 50
    rng = np.random.default_rng(36)
    lab = band_labels(rng, H, W, K)
    x = (rng.standard_normal((3, H, W)) * 3.0 - 0.25).astype(np.float32)
    ref = check_against_ref(x, lab, K)
    check_argmax(x, lab, K, ref)
    assert ref["counts"].min() > 1000
    xi = integer_features(rng, lab[None], 3, K, e_lo=-60, e_hi=60)              # 40 001 tiles of 48 * 1023 * 2^60 stay finite
    check_exact_pool(xi, lab[None], K)


def test_more_entries_than_one_finalize_grid_holds_at_k_65534():
    # 33 * 65534 = 2 162 622 entries for the 2 097 152 threads of the largest finalize grid; K = 65534 makes -3 a label of the
    # int16 map (65533) and leaves -2 and -1 as "none"
    Cc, H, W, K = 33, 40, 130, 65534
    rng = np.random.default_rng(37)
    u = rng.integers(0, K, (H, W))
    special = rng.permutation(H * W)[:400].reshape(4, 100)
    for vals, v in zip(special, (65533, 65534, 65535, -1)):
        u.reshape(-1)[vals] = v
    lab16 = u.astype(np.uint16).view(np.int16)                                  # -1 -> 0xFFFF
    lab32 = u.astype(np.int32)
    assert (lab16 == -3).sum() >= 100 and (lab16 == -2).sum() == 100 and (lab16 == -1).sum() == 200
    x = (rng.standard_normal((Cc, H, W)) * 3.0 - 0.25).astype(np.float32)
    ref = check_against_ref(x, lab16, K)
    assert ref["counts"][0, 65533] >= 100 and ref["counts"].sum() == H * W - 300
    check_argmax(x[:2], lab16, K, R.pool(x[None, :2], lab16[None], K))
    ref32 = check_against_ref(x, lab32, K)
    assert np.array_equal(ref32["counts"], ref["counts"])
    xt = torch.from_numpy(x).to(DEV)
    for r in ("sum", "mean", "max"):                                            # the two label types agree bit for bit
        a, b = superpixel_pool(xt, lab16, K, reduce=r), superpixel_pool(xt, torch.from_numpy(lab32), K, reduce=r)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), r
    xi = integer_features(rng, lab32[None], Cc, K, tile=(40, 130))[0]           # one power of two per (label, channel)
    s = superpixel_pool(torch.from_numpy(xi).to(DEV), lab16, K, reduce="sum")
    assert np.array_equal(s.cpu().numpy().view(np.uint32), R.exact_pool(xi[None], lab16[None], K)[0])
    up = superpixel_unpool(s, lab16, fill=-7.25).cpu().numpy()                  # the [33, 65534] table back to the pixels
    assert np.array_equal(up.view(np.uint32), R.unpool(s.cpu().numpy(), lab16, -7.25).view(np.uint32))
    up32 = superpixel_unpool(s, torch.from_numpy(lab32).to(DEV), fill=-7.25).cpu().numpy()
    assert np.array_equal(up32.view(np.uint32), up.view(np.uint32))
