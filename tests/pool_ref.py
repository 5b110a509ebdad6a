"""Float64 numpy reference of superpixel pooling (fast_slic_amd/pool.py): sum, |x| sum, counts, max with its lowest-index argmax,
and unpool.  Per channel np.bincount / one sort per frame, so that 3840x2160 frames take seconds.  And the exact model of the sum
(exact_sum_bits, exact_pool): plain Python integers, one rounding at the end, for bit-for-bit comparisons."""
import numpy as np


def valid_labels(labels, K):
    """int64 labels of [.., H, W] and the mask of those in [0, K) (the int16 map's -1 is 0xFFFF, as the library reads it)."""
    lab = np.asarray(labels)
    if lab.dtype == np.int16:
        lab = lab.view(np.uint16)
    lab = lab.astype(np.int64)
    return lab, (lab >= 0) & (lab < K)


def ordered_key(x):
    """uint32 whose order is the float order (-0.0 below +0.0), as the kernel's."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def from_key(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def pool_frame(x, labels, K):
    """x [C, H, W] float32, labels [H, W] -> dict of sum / abs (float64 [C, K]), counts (int64 [K]), max (float32 [C, K], 0 where
    empty) and argmax (int64 [C, K], -1 where empty)."""
    Cc, H, W = x.shape
    lab, ok = valid_labels(labels, K)
    idx = lab.reshape(-1)[ok.reshape(-1)]
    pos = np.nonzero(ok.reshape(-1))[0]
    counts = np.bincount(idx, minlength=K).astype(np.int64)
    out = dict(sum=np.zeros((Cc, K)), abs=np.zeros((Cc, K)), counts=counts,
               max=np.zeros((Cc, K), np.float32), argmax=np.full((Cc, K), -1, np.int64))
    order = np.argsort(idx, kind="stable")               # by label, then by flat index
    pos_s = pos[order]
    nonempty = np.nonzero(counts)[0]
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])[nonempty]
    for c in range(Cc):
        v = x[c].reshape(-1)[pos].astype(np.float64)
        out["sum"][c] = np.bincount(idx, weights=v, minlength=K)
        out["abs"][c] = np.bincount(idx, weights=np.abs(v), minlength=K)
        if idx.size == 0:
            continue
        key = ordered_key(x[c].reshape(-1)[pos_s]).astype(np.int64)
        kmax = np.maximum.reduceat(key, starts)
        at_max = key == np.repeat(kmax, counts[nonempty])
        first = np.minimum.reduceat(np.where(at_max, pos_s, np.iinfo(np.int64).max), starts)
        out["max"][c, nonempty] = from_key(kmax.astype(np.uint32))
        out["argmax"][c, nonempty] = first
    return out


def pool(x, labels, K):
    """[N, C, H, W] / [N, H, W] -> the dict of pool_frame with a leading N axis."""
    frames = [pool_frame(x[n], labels[n], K) for n in range(x.shape[0])]
    return {k: np.stack([f[k] for f in frames]) for k in frames[0]}


def unpool(values, labels, fill):
    """values [C, K] / [N, C, K], labels [H, W] / [N, H, W] -> [C, H, W] / [N, C, H, W]: a gather, `fill` where the label is not in
    [0, K)."""
    values = np.asarray(values, dtype=np.float32)
    batched = values.ndim == 3
    V, L = (values, labels) if batched else (values[None], np.asarray(labels)[None])
    lab, ok = valid_labels(L, V.shape[-1])
    out = np.empty(V.shape[:2] + L.shape[-2:], np.float32)
    for n in range(V.shape[0]):
        out[n] = np.where(ok[n][None], V[n][:, np.where(ok[n], lab[n], 0)], np.float32(fill))
    return out if batched else out[0]


# ---- the exact model of the sum ----
# The sum of a segment is specified on the per-tile partials (one f32 per tile, label and channel): every finite, normal partial p
# counts as the integer trunc(p * 2^96) (towards zero, the same for both signs; zero, subnormals and anything below 2^-96 count as
# nothing), T is the sum of these integers, and the result is T * 2^-96 rounded once to f32, nearest with ties to even.  T == 0 is
# +0.0 and |T * 2^-96| >= 2^128 - 2^103 (FLT_MAX plus half an ulp, which ties upward) is +-inf.
FIX_LSB = -96


def fixed_of_bits(bits):
    """trunc(p * 2^-FIX_LSB) as a Python int, for the f32 p with these bits; NaN / Inf are refused."""
    u = int(bits) & 0xFFFFFFFF
    ex = (u >> 23) & 0xFF
    if ex == 0xFF:
        raise ValueError("non-finite partial %08x" % u)
    if ex == 0:
        return 0
    mag = (u & 0x7FFFFF) | 0x800000                       # p = mag * 2^(ex - 150)
    up = ex - 150 - FIX_LSB
    mag = mag << up if up >= 0 else mag >> -up
    return -mag if u >> 31 else mag


def round_to_f32_bits(T, lsb=FIX_LSB):
    """Bits of T * 2^lsb (T a Python int) rounded to the nearest f32, ties to even; +-inf from 2^128 - 2^103 on; 0 is +0.0.  Results
    below the normal range are refused (with lsb = -96 there are none)."""
    if T == 0:
        return 0
    sign = 0x80000000 if T < 0 else 0
    a = -T if T < 0 else T
    top = a.bit_length() - 1                              # position of the leading one
    if top > 23:
        drop = top - 23
        mant, rest, half = a >> drop, a & ((1 << drop) - 1), 1 << (drop - 1)
        if rest > half or (rest == half and mant & 1):
            mant += 1
            if mant == 1 << 24:
                mant, top = mant >> 1, top + 1
    else:
        mant = a << (23 - top)
    e = top + lsb                                         # the value is mant * 2^(e - 23), 2^23 <= mant < 2^24
    if e > 127:
        return sign | 0x7F800000
    if e < -126:
        raise ValueError("result below the normal range of f32")
    return sign | ((e + 127) << 23) | (mant & 0x7FFFFF)


def exact_sum_bits(partials):
    """The f32 bit pattern of the pooled sum of one (n, c, k), from its tile partials as f32 bit patterns (any order)."""
    return round_to_f32_bits(sum(fixed_of_bits(b) for b in partials))


def f32_bits_of_scaled(S, q):
    """Bits of the f32 that equals S * 2^q exactly (S a Python int); ValueError when no f32 does."""
    if S == 0:
        return 0
    sign = 0x80000000 if S < 0 else 0
    a = -S if S < 0 else S
    tz = (a & -a).bit_length() - 1
    a, q = a >> tz, q + tz
    n = a.bit_length()
    e = q + n - 1
    if n > 24 or e > 127 or q < -149:
        raise ValueError("tile partial %d * 2^%d is not representable in f32" % (S if sign == 0 else -S, q))
    if e < -126:                                          # subnormal: a * 2^q = (a << (q + 149)) * 2^-149
        return sign | (a << (q + 149))
    return sign | ((e + 127) << 23) | ((a << (24 - n)) & 0x7FFFFF)


def exact_pool(x, labels, K, tile=(16, 64)):
    """x [N, C, H, W] float32 (finite), labels [N, H, W] -> uint32 [N, C, K]: the bits of the pooled sums by the model above.

    Depends on the kernel's geometry: a partial is the sum of one label's pixels inside one tile of 16 rows x 64 columns (kPoolRows
    and the 64 lanes of a wavefront in csrc/pool.hip), the tiles aligned at the frame's origin.  Every partial is formed exactly, as
    an integer times a power of two, and must be representable in f32 (ValueError otherwise): only then is the f32 partial of the
    kernel the partial of the model, provided the input is built so that no order of adding a tile's pixels can round."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    N, Cc, H, W = x.shape
    if not np.isfinite(x).all():
        raise ValueError("exact_pool takes finite features")
    th, tw = tile
    ntx = (W + tw - 1) // tw
    tile_id = ((np.arange(H) // th)[:, None] * ntx + (np.arange(W) // tw)[None, :]).reshape(-1)
    out = np.zeros((N, Cc, K), np.uint32)
    for n in range(N):
        lab, ok = valid_labels(labels[n], K)
        pos = np.nonzero(ok.reshape(-1))[0]
        if pos.size == 0:
            continue
        key = tile_id[pos] * K + lab.reshape(-1)[pos]                    # (tile, label), sorted by it
        order = np.argsort(key, kind="stable")
        pos, key = pos[order], key[order]
        starts = np.concatenate([[0], np.nonzero(np.diff(key))[0] + 1])
        group_label = (key[starts] % K).tolist()
        sizes = np.diff(np.concatenate([starts, [key.size]]))
        for c in range(Cc):
            frac, ex = np.frexp(x[n, c].reshape(-1)[pos].astype(np.float64))
            mant = np.ldexp(frac, 24).astype(np.int64)                   # the pixel is mant * 2^(ex - 24), exactly
            ex = np.where(mant != 0, ex.astype(np.int64) - 24, np.int64(1 << 20))
            emin = np.minimum.reduceat(ex, starts)
            up = np.where(mant != 0, ex - np.repeat(emin, sizes), 0)
            narrow = np.maximum.reduceat(up, starts) <= 28               # 24 + 28 bits and 2^10 pixels stay inside int64
            S = np.add.reduceat(np.where(np.repeat(narrow, sizes), mant << np.minimum(up, 28), 0), starts).tolist()
            for g in np.nonzero(~narrow)[0]:                             # a wide spread of exponents: Python integers
                lo, hi = starts[g], starts[g] + sizes[g]
                S[g] = sum(int(m) << int(u) for m, u in zip(mant[lo:hi], up[lo:hi]))
            lists = {}
            for k, s, q in zip(group_label, S, emin.tolist()):
                lists.setdefault(k, []).append(f32_bits_of_scaled(s, q) if s else 0)
            for k, parts in lists.items():
                out[n, c, k] = exact_sum_bits(parts)
    return out
