"""Float64 numpy model of the LSC variant, stage by stage, restated from the reference (src/lsc.cpp, src/context.cpp).

The yardstick of tests/test_gpu_lsc_stages.py; tests/test_lsc_ref_cpu.py pins it against the reference's own fixtures.  Slow and obvious
on purpose.  The tables are built with the reference's expressions and rounded to float32 where the reference stores float32; everything
from the tables on is float64: the feature means, the weight w = sum_q mean_q F_q, the features G = F / w, the seed centroids, the
distances sum (G - C)^2 and the centroid update sum w G / sum w = sum F / sum w.  Every stage takes its inputs as arguments, so a test
can start each one from the state of the implementation under test and nothing compounds.

Feature order: l1 l2 a1 a2 b1 b2 x1 x2 y1 y2 (src/lsc.h:12).  Labels are uint16, 0xFFFF = none."""
import math

import numpy as np

from oracle import oracle as orc

C_COLOR = np.float32(20.0)          # src/lsc.h:8
NONE = 0xFFFF
FLT_MAX = float(np.finfo(np.float32).max)


def lab_plane(image, convert_to_lab=True):
    """[H, W, 3] uint8 of the three planes the features are looked up from (src/context.cpp:113-127)."""
    image = np.ascontiguousarray(image)
    return orc.rgb_to_lab(image)[:, :, :3].copy() if convert_to_lab else image.copy()


def tables(H, W, S, compactness):
    """The eight float32 tables of src/lsc.cpp:25-28, 70-101: theta in float32 steps, cos / sin of it in double (the unqualified
    cos(float) of the reference is the C one), products as the reference forms them."""
    f32 = np.float32
    PI = f32(3.1415926)
    halfPI = f32(PI / f32(2))
    ratio = f32(f32(compactness) / f32(100.0))
    C_spatial = f32(C_COLOR * ratio)
    t = {}
    theta = [float(f32(halfPI * f32(f32(X) / f32(255.0)))) for X in range(256)]
    cosine = np.array([math.cos(v) for v in theta], np.float64)
    sine = np.array([math.sin(v) for v in theta], np.float64)
    # float cosine = cos(theta); C_color * cosine * 2.55f: float32 all the way
    t["ab_cos"] = ((C_COLOR * cosine.astype(f32)).astype(f32) * f32(2.55)).astype(f32)
    t["ab_sin"] = ((C_COLOR * sine.astype(f32)).astype(f32) * f32(2.55)).astype(f32)
    # C_color * cos(theta): a double product, rounded by the store
    t["L_cos"] = (float(C_COLOR) * cosine).astype(f32)
    t["L_sin"] = (float(C_COLOR) * sine).astype(f32)
    step = f32(halfPI / f32(S))
    for name, n in (("x", W), ("y", H)):
        th = [float(f32(f32(i) * step)) for i in range(n)]
        t[name + "_cos"] = (float(C_spatial) * np.array([math.cos(v) for v in th], np.float64)).astype(f32)
        t[name + "_sin"] = (float(C_spatial) * np.array([math.sin(v) for v in th], np.float64)).astype(f32)
    return t


def features(lab, t):
    """F [H, W, 10] float64: the table values of every pixel (src/lsc.cpp:103-135), exact float32 numbers."""
    H, W, _ = lab.shape
    F = np.empty((H, W, 10), np.float64)
    L, a, b = lab[:, :, 0], lab[:, :, 1], lab[:, :, 2]
    F[:, :, 0] = t["L_cos"][L]
    F[:, :, 1] = t["L_sin"][L]
    F[:, :, 2] = t["ab_cos"][a]
    F[:, :, 3] = t["ab_sin"][a]
    F[:, :, 4] = t["ab_cos"][b]
    F[:, :, 5] = t["ab_sin"][b]
    F[:, :, 6] = t["x_cos"][None, :]
    F[:, :, 7] = t["x_sin"][None, :]
    F[:, :, 8] = t["y_cos"][:, None]
    F[:, :, 9] = t["y_sin"][:, None]
    return F


def feature_means(F):
    """The ten means over the frame (src/lsc.cpp:143-149), float64."""
    return F.reshape(-1, 10).mean(axis=0)


def weights(F, means):
    """w [H, W] = sum_q mean_q F_q (src/lsc.cpp:154-160) for the given means."""
    return F @ np.asarray(means, np.float64)


def clamp_centres(y, x, H, W):
    """Integer centres as assign() sees them: the safeguard's clamp, then the cast (src/context.cpp:208-211, src/lsc.cpp:200)."""
    cy = np.clip(np.asarray(y, np.float64), 0, H - 1).astype(np.int64)
    cx = np.clip(np.asarray(x, np.float64), 0, W - 1).astype(np.int64)
    return cy, cx


def seed_centroids(G, cy, cx, S):
    """[K, 10]: the unweighted mean of G over the (2 (S / 4) + 1)^2 window, clipped to the image (src/lsc.cpp:165-195)."""
    H, W, _ = G.shape
    q4 = S // 4
    C = np.empty((len(cy), 10), np.float64)
    for k, (y, x) in enumerate(zip(cy, cx)):
        win = G[max(y - q4, 0):min(y + q4 + 1, H), max(x - q4, 0):min(x + q4 + 1, W)]
        C[k] = win.reshape(-1, 10).mean(axis=0)
    return C


def seed_window_sizes(cy, cx, S, H, W):
    q4 = S // 4
    cy, cx = np.asarray(cy), np.asarray(cx)
    return (np.minimum(cy + q4 + 1, H) - np.maximum(cy - q4, 0)) * (np.minimum(cx + q4 + 1, W) - np.maximum(cx - q4, 0))


def visit_rank(cy, cx, S, H, W):
    """Position of every cluster in assign()'s visit order as a pixel meets it (src/context.cpp:214-242): the phase of its cell of
    2 S + 32 pixels, then its number (two clusters of one phase that reach the same pixel share a cell)."""
    T = 2 * S + 32
    phase = 2 * ((np.asarray(cy) // T) % 2) + (np.asarray(cx) // T) % 2
    return phase * len(cy) + np.arange(len(cy))


def distances(G, rows, cy, cx, C, S):
    """D [K, R, W] float64: sum (G - C_k)^2 where cluster k is a candidate of the pixel -- |i - cy| <= S, |j - cx| <= S, finite centroid
    (a NaN distance never passes `min_dist > dist`, src/lsc.cpp:203-217) -- and +inf elsewhere.  `rows`: the R visited rows."""
    H, W, _ = G.shape
    rows = np.asarray(rows, np.int64)
    D = np.full((len(cy), len(rows), W), np.inf, np.float64)
    for k in range(len(cy)):
        if not np.isfinite(C[k]).all():
            continue
        sel = np.nonzero(np.abs(rows - cy[k]) <= S)[0]
        x_lo, x_hi = max(cx[k] - S, 0), min(cx[k] + S + 1, W)
        if sel.size == 0 or x_lo >= x_hi:
            continue
        diff = G[rows[sel], x_lo:x_hi] - C[k]
        D[k][sel[:, None], np.arange(x_lo, x_hi)[None, :]] = (diff * diff).sum(axis=-1)
    return D


def assign(D, rank, prev):
    """Labels [R, W] of the visited rows from their distances: the smallest, the first in visit order among equals (strict `>`); a
    pixel without a candidate keeps `prev` (src/lsc.cpp:217-220 never touches it)."""
    order = np.argsort(rank, kind="stable")
    best = order[np.argmin(D[order], axis=0)]
    covered = np.isfinite(D).any(axis=0)
    return np.where(covered, best, prev).astype(np.uint16), covered


def update(labels, rows, lab, F, w, K, cy, cx, colour, members):
    """update() + after_update() over the visited rows of a label plane (src/context.cpp:301-381 with all clusters active,
    src/lsc.cpp:226-307).  Returns (cy, cx, colour [K, 3], members [K], C [K, 10]): round_int centres and colours and the member count
    exactly; C = sum w G / sum w = sum F / sum w.  A cluster without a member keeps its integer fields, takes num_members = 0 and a NaN
    centroid (0 / 0)."""
    rows = np.asarray(rows, np.int64)
    lbl = labels[rows].astype(np.int64)
    ok = lbl != NONE
    l = lbl[ok]
    yy = np.broadcast_to(rows[:, None], lbl.shape)[ok]
    xx = np.broadcast_to(np.arange(labels.shape[1])[None, :], lbl.shape)[ok]
    n = np.bincount(l, minlength=K).astype(np.int64)
    sums = [np.bincount(l, weights=v.astype(np.float64), minlength=K).astype(np.int64)
            for v in (yy, xx, lab[rows][ok][:, 0], lab[rows][ok][:, 1], lab[rows][ok][:, 2])]
    has = n > 0
    nn = np.where(has, n, 1)
    rnd = [(s + nn // 2) // nn for s in sums]          # round_int, src/fast-slic-common.h:63-65
    cy2 = np.where(has, rnd[0], cy)
    cx2 = np.where(has, rnd[1], cx)
    colour2 = np.where(has[:, None], np.stack(rnd[2:], axis=1), colour)
    sF = np.stack([np.bincount(l, weights=F[rows][ok][:, q], minlength=K) for q in range(10)], axis=1)
    sw = np.bincount(l, weights=w[rows][ok], minlength=K)
    with np.errstate(invalid="ignore", divide="ignore"):
        C = np.where(has[:, None], sF / np.where(has, sw, 1.0)[:, None], np.nan)
    return cy2, cx2, colour2, n, C


def visited_rows(H, rem, stride):
    return np.arange(rem, H, stride)


def run(image, clusters, max_iter, compactness=10.0, subsample_stride=3, convert_to_lab=True):
    """The whole of iterate() up to full_assign in float64 (src/context.cpp:108-181): returns (pre-connectivity labels, cy, cx, members).
    `clusters`: the initialised Cluster array (its y, x are read)."""
    H, W, _ = image.shape
    K = clusters.shape[0]
    S = orc.S_of(H, W, K)
    lab = lab_plane(image, convert_to_lab)
    F = features(lab, tables(H, W, S, compactness))
    means = feature_means(F).astype(np.float32)         # the reference keeps them in float32
    w = weights(F, means)
    G = F / w[:, :, None]
    cy, cx = clamp_centres(clusters["y"], clusters["x"], H, W)
    C = seed_centroids(G, cy, cx, S)
    colour = lab[cy, cx].astype(np.int64)
    members = np.zeros(K, np.int64)
    labels = np.full((H, W), NONE, np.uint16)
    rem = 0
    for _ in range(max_iter):
        rows = visited_rows(H, rem, subsample_stride)
        labels[rows], _ = assign(distances(G, rows, cy, cx, C, S), visit_rank(cy, cx, S, H, W), labels[rows])
        cy, cx, colour, members, C = update(labels, rows, lab, F, w, K, cy, cx, colour, members)
        rem = (rem + 1) % subsample_stride
    rows = np.arange(H)
    labels[rows], _ = assign(distances(G, rows, cy, cx, C, S), visit_rank(cy, cx, S, H, W), labels[rows])
    return labels, cy, cx, members
