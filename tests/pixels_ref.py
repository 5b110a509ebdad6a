"""The numpy model of fast_slic_amd/pixels.py's rules, float32 operation by operation (every numpy float32 array operation rounds each
element once; a fold runs over slot s, or channel c, of every pixel at once, which keeps the order inside each pixel).  The exponential
is the library's own host entry (attention_ref.expf).  No GPU.

Arrays: labels integer [N, H, W]; offsets int64 [N * K + 1] and indices int32 [nnz] of any content; pixel features float32
[N, C, H, W], node features float32 [N, C, K], per-slot arrays float32 [N, Hd, S, H, W].  slots() is rule 0, the terms: int64
[N, S, H, W], the node of every slot and -1 where it is empty.

dot, softmax, mix and the softmax's backward are bit for bit.  For the scatter the model offers two things:
  scatter_exact  the products in float32, then per (tile of 16 x 64, label, slot, channel) the partial as an exact integer multiple of
                 2^-149, which must be a float32 (ValueError otherwise: then, and only then, is it the kernel's partial whatever order
                 the kernel adds in -- provided the inputs are built so that no partial sum inside a tile can round), and the
                 partials of a node added with pool_ref.fixed_of_bits / round_to_f32_bits -> uint32 bits [N, C, K].
  scatter_sum64  the float64 sum of the float32 products -> (sum [N, C, K], sum of |products| [N, C, K]).  The kernel's result lies
                 within gamma(1026) * sum |w x| of the exact sum of the exact products, u = 2^-24: a product is rounded once, a
                 partial is a sum of at most 1024 products in some order (1023 additions), and the total is rounded once more; the
                 truncation of a partial to 2^-96 is below all of this for inputs of ordinary size.  gamma(n) = n u / (1 - n u):
                 1025 roundings at the most, one to spare for the float64 side (aggregate_ref.gamma(d) is gamma(d + 1)).

The bounds of the comparisons with float64 are attention_ref's, with the slots of a pixel in the place of the entries of a row:
  dot and mix: |fold - exact| <= gamma(n) * sum |terms|, n the terms of the fold.
  alpha of a pixel of d non-empty slots, Delta = max |s - m|: rel(alpha) <= 2 (Delta + 2) u + gamma(d)           (alpha_bound)
  softmax backward with A = sum |alpha g|: |grad - exact| <= alpha ((gamma(d) + rel) A + (rel + 2 u) |g - t|)     (softmax_backward_bound)
Each is multiplied by 1 + 2^-10 for the products of these first-order terms."""
import numpy as np

import pool_ref as P
from aggregate_ref import gamma
from attention_ref import SLACK, U, expf

F32 = np.float32
TILE = (16, 64)


def slots(labels, offsets, indices, N, K, S):
    """The terms -> int64 [N, S, H, W]: the node of every slot, -1 where it is empty."""
    labels = np.asarray(labels).astype(np.int64).reshape((N,) + tuple(np.shape(labels)[-2:]))
    offsets, indices = np.asarray(offsets, np.int64), np.asarray(indices, np.int64)
    nnz = len(indices)
    assert len(offsets) == N * K + 1 and 1 <= S <= 32
    has = (labels >= 0) & (labels < K)
    row = np.arange(N).reshape(N, 1, 1) * K + np.where(has, labels, 0)
    lo, hi = np.clip(offsets[row], 0, nnz), np.clip(offsets[row + 1], 0, nnz)
    out = np.full((N, S) + labels.shape[1:], -1, np.int64)
    out[:, 0] = np.where(has, labels, -1)
    for s in range(1, S):
        p = lo + s - 1
        ok = has & (p < hi)
        j = np.where(ok, indices[np.minimum(p, max(nnz - 1, 0))] if nnz else -1, -1)
        out[:, s] = np.where(ok & (j >= 0) & (j < K), j, -1)
    return out


def at_nodes(t, sl):
    """t [N, C, K] read at the node of every slot -> [N, C, S, H, W] (node 0 where the slot is empty)."""
    N = t.shape[0]
    return np.moveaxis(t[np.arange(N).reshape(N, 1, 1, 1), :, np.maximum(sl, 0)], -1, 1)


def dot(a, b, sl, Hd):
    """Rule 1 -> float32 [N, Hd, S, H, W]."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    N, Cc, H, W = a.shape
    D, S = Cc // Hd, sl.shape[1]
    bj = at_nodes(b, sl)
    out = np.zeros((N, Hd, S, H, W), F32)
    for h in range(Hd):
        acc = np.zeros((N, S, H, W), F32)
        for c in range(h * D, h * D + D):                                  # every pixel and slot at once, the channels in order
            acc = acc + a[:, c, None] * bj[:, c]
        out[:, h] = np.where(sl >= 0, acc, F32(0))
    return out


def softmax(s, sl):
    """Rule 2 -> float32 [N, Hd, S, H, W]."""
    s = np.asarray(s, F32)
    v = np.broadcast_to((sl >= 0)[:, None], s.shape)
    m = np.where(v, s, F32(-np.inf)).max(axis=2, keepdims=True)
    e = np.zeros_like(s)
    e[v] = expf((s - np.where(np.isfinite(m), m, F32(0)))[v])
    Z = np.zeros_like(m[:, :, 0])
    for k in range(s.shape[2]):                                            # an empty slot adds +0.0 to Z >= 0: nothing
        Z = Z + e[:, :, k]
    alpha = np.zeros_like(s)
    alpha[v] = (e / np.where(Z > 0, Z, F32(1))[:, :, None])[v]
    return alpha


def softmax_backward(alpha, g, sl):
    """Rule 5 -> float32 [N, Hd, S, H, W]."""
    alpha, g = np.asarray(alpha, F32), np.asarray(g, F32)
    v = np.broadcast_to((sl >= 0)[:, None], alpha.shape)
    t = np.zeros_like(alpha[:, :, 0])
    for k in range(alpha.shape[2]):
        t = np.where(v[:, :, k], t + alpha[:, :, k] * g[:, :, k], t)
    return np.where(v, alpha * (g - t[:, :, None]), F32(0))


def mix(values, weight, sl):
    """Rule 3 -> float32 [N, C, H, W]."""
    values, weight = np.asarray(values, F32), np.asarray(weight, F32)
    N, Cc, _ = values.shape
    Hd, S = weight.shape[1:3]
    D = Cc // Hd
    vj = at_nodes(values, sl)
    out = np.zeros((N, Cc) + sl.shape[2:], F32)
    for c in range(Cc):
        acc = np.zeros((N,) + sl.shape[2:], F32)
        for k in range(S):                                                 # every pixel at once, the slots in order
            acc = np.where(sl[:, k] >= 0, acc + weight[:, c // D, k] * vj[:, c, k], acc)
        out[:, c] = acc
    return out


def products(x, weight):
    """The float32 products of rule 4 -> [N, C, S, H, W]."""
    x, weight = np.asarray(x, F32), np.asarray(weight, F32)
    D = x.shape[1] // weight.shape[1]
    return np.repeat(weight, D, axis=1) * x[:, :, None]


def scatter_sum64(x, weight, sl, K):
    """-> (float64 [N, C, K] sum of the float32 products per node, float64 [N, C, K] sum of their magnitudes)."""
    prod = products(x, weight).astype(np.float64)
    N, Cc = prod.shape[:2]
    out, mag = np.zeros((N, Cc, K)), np.zeros((N, Cc, K))
    v = sl >= 0
    for n in range(N):
        j = sl[n][v[n]]
        for c in range(Cc):
            t = prod[n, c][v[n]]
            out[n, c] = np.bincount(j, weights=t, minlength=K)
            mag[n, c] = np.bincount(j, weights=np.abs(t), minlength=K)
    return out, mag


def scatter_bound(mag):
    return gamma(1026 - 1) * mag       # aggregate_ref.gamma(d) = (d + 1) u / (1 - (d + 1) u): the module's gamma(1026)


def scatter_exact(x, weight, labels, sl, K, tile=TILE):
    """Rule 4 -> uint32 [N, C, K], the bits of the result, where every tile partial is a float32 (ValueError otherwise)."""
    prod = products(x, weight)
    if not np.isfinite(prod).all():
        raise ValueError("scatter_exact takes finite products")
    N, Cc, S, H, W = prod.shape
    labels = np.asarray(labels).astype(np.int64).reshape(N, H, W)
    th, tw = tile
    tile_id = (np.arange(H) // th)[:, None] * ((W + tw - 1) // tw) + (np.arange(W) // tw)[None, :]
    frac, ex = np.frexp(prod.astype(np.float64))
    mant = np.ldexp(frac, 24).astype(np.int64)                             # a product is mant * 2^(ex - 24), exactly
    up = ex.astype(np.int64) - 24 + 149                                    # >= 0 for every non-zero float32
    total = {}
    for n in range(N):
        for s in range(S):
            ok = sl[n, s] >= 0
            if not ok.any():
                continue
            key = (tile_id[ok] * K + labels[n][ok]) * K + sl[n, s][ok]       # (tile, label, node); the slot is this loop's
            order = np.argsort(key, kind="stable")
            starts = np.concatenate([[0], np.nonzero(np.diff(key[order]))[0] + 1])
            nodes = (key[order][starts] % K).tolist()
            for c in range(Cc):
                ints = [int(m) << int(u) if m else 0 for m, u in zip(mant[n, c, s][ok][order].tolist(), up[n, c, s][ok][order].tolist())]
                bounds = starts.tolist() + [len(ints)]
                for q, j in enumerate(nodes):
                    part = sum(ints[bounds[q]:bounds[q + 1]])
                    bits = P.f32_bits_of_scaled(part, -149)                # ValueError: this partial is no float32
                    total[(n, c, j)] = total.get((n, c, j), 0) + P.fixed_of_bits(bits)
    out = np.zeros((N, Cc, K), np.uint32)
    for (n, c, j), T in total.items():
        out[n, c, j] = P.round_to_f32_bits(T)
    return out


# ---- the bounds against float64 ----
def alpha_bound(s, sl):
    """rel(alpha) of every (pixel, head) -> float64 [N, Hd, 1, H, W]."""
    s = np.asarray(s, np.float64)
    v = np.broadcast_to((sl >= 0)[:, None], s.shape)
    hi = np.where(v, s, -np.inf).max(axis=2, keepdims=True)
    lo = np.where(v, s, np.inf).min(axis=2, keepdims=True)
    d = (sl >= 0).sum(axis=1)[:, None, None]
    delta = np.where(d > 0, hi - lo, 0.0)
    return (2.0 * (delta + 2.0) * U + gamma(d)) * SLACK


def softmax_backward_bound(alpha64, g, rel, sl):
    alpha64, g = np.asarray(alpha64, np.float64), np.asarray(g, np.float64)
    v = (sl >= 0)[:, None]
    d = (sl >= 0).sum(axis=1)[:, None, None]
    t = (alpha64 * g * v).sum(axis=2, keepdims=True)
    A = np.abs(alpha64 * g * v).sum(axis=2, keepdims=True)
    return alpha64 * ((gamma(d) + rel) * A + (rel + 2.0 * U) * np.abs(g - t)) * SLACK
