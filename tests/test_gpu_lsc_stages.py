"""The LSC kernels (fast_slic_amd/csrc/lsc.hip) stage by stage against the float64 model of the reference's operation (tests/lsc_ref.py).

tests/test_gpu_lsc.py compares whole runs with the reference's fixtures by floors (0.99 agreement after ten compounded iterations); one
percent of a frame hides a table read at the wrong byte, a window one pixel short or an accumulator shifted by one.  Here every stage
starts from the GPU's OWN previous state, so nothing compounds, and is held to a bound that follows from float arithmetic:

  a  feature means           |mean - mean64| <= 4 * 2^-24 * mean|F_q|: the kernel forms the exact mean in double; one rounding to f32 and
                             half an ulp per table entry remain.
  b  seed centroids          per component (n_win + 16) * 2^-24 * mean|G_q| over the window: the worst case of summing n_win f32 terms in
                             any order, plus 16 units for the weight chain, the reciprocal, the product and the final divide.
  c  full assignment         under (cfeat_m, centres_m), every m.  tol(p, k) = 256 * 2^-24 * (|G_p|^2 + |C_k|^2) bounds the f32 evaluation
                             error of the distance in ANY algebraic form, the form around a block origin included: with both operands at
                             most twice |G| from the origin, about 12 roundings on terms of total size (|a| + |b|)^2 <= 16 |G|^2 are 192
                             units, the rest covers the 3-unit relative error of G itself.  A pixel is DECIDED when the float64 best
                             candidate beats every other candidate by more than the sum of the two tolerances: it must carry exactly the
                             model's label.  Every other covered pixel must carry a candidate within tolerance of the best.  A pixel no
                             window reaches keeps what it had (src/lsc.cpp:217-220 never touches it): 0xFFFF unless an earlier pass
                             labelled it.
  d  subsampled assignment   the recorder's plane after iteration t: rule c on the rows = t (mod stride) under state t, the other rows
                             equal to iteration t - 1's plane (0xFFFF before iteration 0); the recorded min-dist of a visited covered
                             pixel within tol + 5e-6 relative (the report prints six digits) of the float64 distance of its label, and
                             FLT_MAX as the report prints it everywhere else (assign() refills the plane on entry, src/context.cpp:200-206,
                             and src/recorder.h:73-78 copies it whole).
  e  update                  the model's update over the recorder's plane of iteration m - 1 against state m: centres, colours and
                             num_members EXACTLY; cfeat_m within the bound of `update_bound` below, derived from the documented fixed point.
  f  groups                  a frame's means and centroids inside a group of four: byte-equal to its single run.

State m comes from a plain run with max_iter = m (the variant is deterministic, so run m's first m iterations are run n's); the planes
and min-dists from one debug_mode run with max_iter = n, whose final result must equal the plain run's.  In every stage at most 3 % of
the covered pixels may be undecided, so that the exact rule carries the test.  preemptive=True is out of scope (other masks)."""
import json

import numpy as np
import pytest

import lsc_ref
from fast_slic_amd import Engine, make_params
from fast_slic_amd import _binding as B
from fast_slic_amd.synth import variant
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                       # half an ulp of a float32 in [1, 2): the unit of every bound here
DIST_TOL = 256 * U                   # stage c
MAX_UNDECIDED = 0.03
FLT_MAX_PRINTED = float("3.40282e+38")      # numeric_limits<float>::max() through operator<< at the default precision


def piled_7(cl):
    i = np.arange(70)
    cl["y"][:70] = 26 + 2 * (i // 10)
    cl["x"][:70] = 30 + 3 * (i % 10)


def piled_8(cl):
    i = np.arange(16)
    cl["y"][:16] = 10 + 4 * (i // 4)
    cl["x"][:16] = 10 + 4 * (i % 4)


# the smallest shapes that reach each path
CASES = {
    "default_120x160_k40": dict(kind="A", H=120, W=160, K=40, stride=3, n=3, c=10.0),
    "ragged_61x83_k20": dict(kind="B", H=61, W=83, K=20, stride=1, n=3, c=10.0),                       # last block partial both ways
    "small_S_96x128_k300": dict(kind="A", H=96, W=128, K=300, stride=1, n=3, c=5.0, want_nan=True),    # S = 6; memberless clusters
    "tall_200x70_k9_stride5": dict(kind="A", H=200, W=70, K=9, stride=5, n=2, c=10.0),                 # S = 39; pixels no window reaches
    "flat_33x200_k7": dict(kind="A", H=33, W=200, K=7, stride=1, n=2, c=10.0),                         # fewer rows than two blocks
    "narrow_300x41_k9": dict(kind="A", H=300, W=41, K=9, stride=1, n=3, c=10.0),                       # narrower than a tile
    "piled_64x96_k80": dict(kind="C", H=64, W=96, K=80, stride=2, n=2, c=10.0, centres=piled_7, want_walk=True),      # > 64 candidates per block
    "stale_120x120_k16": dict(kind="B", H=120, W=120, K=16, stride=1, n=5, c=40.0, centres=piled_8, want_stale=True),   # the `extra` accumulators
}


@pytest.fixture(scope="module")
def eng():
    """An engine of ONE slot: every call runs on slot 0, and four frames of iterate_batch form one launch group."""
    e = Engine(0, 1)
    yield e
    e.close()


def params(case, max_iter, debug=False):
    return make_params(max_iter, case["c"], 0.25, case["stride"], True, debug_mode=debug, variant=B.VARIANT_LSC)


def initial_clusters(case, img):
    cl = np.zeros(case["K"], B.CLUSTER_DTYPE)
    B._check(B.load_library().fslic_hip_initialize_clusters(case["H"], case["W"], case["K"], img.ctypes.data, cl.ctypes.data))
    if case.get("centres"):
        case["centres"](cl)
    return cl


def cluster_state(y, x, colour, members):
    return dict(y=np.asarray(y, np.float64), x=np.asarray(x, np.float64), colour=np.asarray(colour, np.int64), members=np.asarray(members, np.int64))


def gpu_trajectory(eng, case, img, cl0):
    """states[m] (m = 0 .. n) from plain runs, planes / dists / rec_clusters [t + 1] (t = -1 .. n - 1) from one recording run."""
    H, W, K, n = case["H"], case["W"], case["K"], case["n"]
    states = []
    for m in range(n + 1):
        cl = cl0.copy()
        labels = eng.iterate(img, cl, params(case, m))
        means, cfeat = eng.debug_lsc_state(K)
        st = cluster_state(cl["y"], cl["x"], np.stack([cl["r"], cl["g"], cl["b"]], axis=1), cl["num_members"])
        st.update(means=means, cfeat=cfeat, pre=eng.last_prelabels(H, W), labels=labels, clusters=cl)
        states.append(st)
    cl = cl0.copy()
    labels = eng.iterate(img, cl, params(case, n, debug=True))
    rec_means, rec_cfeat = eng.debug_lsc_state(K)
    doc = json.loads(eng.last_recorder_report())
    # the recording run is the plain run (tests/test_gpu_recorder.py::test_recording_changes_no_result claims it; everything below rests on it)
    assert np.array_equal(labels, states[n]["labels"]) and cl.tobytes() == states[n]["clusters"].tobytes(), "the recording run's result differs from the plain run's"
    assert np.array_equal(eng.last_prelabels(H, W), states[n]["pre"])
    assert rec_means.tobytes() == states[n]["means"].tobytes() and rec_cfeat.tobytes() == states[n]["cfeat"].tobytes(), "LSC state after the recording run"
    assert (doc["height"], doc["width"]) == (H, W) and [s["iteration"] for s in doc["snapshots"]] == list(range(-1, n))
    planes = [np.array(s["assignment"], np.int64).astype(np.uint16).reshape(H, W) for s in doc["snapshots"]]
    dists = [np.array(s["min_dists"], np.float64).reshape(H, W) for s in doc["snapshots"]]
    rec_clusters = [cluster_state([c["yx"][0] for c in s["clusters"]], [c["yx"][1] for c in s["clusters"]], [c["color"] for c in s["clusters"]],
                                  [c["num_members"] for c in s["clusters"]]) for s in doc["snapshots"]]
    return dict(states=states, planes=planes, dists=dists, rec_clusters=rec_clusters)


# ---- the checks (pure numpy: they see the trajectory only) -------------------------------------------------------------------------------

def ratio(err, bound):
    """err / bound; where the bound is 0 (a table entry that is exactly 0 over the whole window), 0 for no error and inf for any."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))


def take(A, idx):
    return np.take_along_axis(A, idx[None], axis=0)[0]


def judge_assignment(D, Gn2, Cn2, got, prev):
    """Rule c for the R visited rows: D [K, R, W] the float64 distances (+inf: no candidate), got / prev [R, W].  Returns the counts of
    violations, the masks and what the min-dist check needs."""
    K = D.shape[0]
    covered = np.isfinite(D).any(axis=0)
    tol = DIST_TOL * (Gn2[None] + np.where(np.isfinite(Cn2), Cn2, 0.0)[:, None, None])
    best = np.argmin(D, axis=0)
    d_best, t_best = take(D, best), take(tol, best)
    low = D - tol
    np.put_along_axis(low, best[None], np.inf, axis=0)
    decided = covered & (low.min(axis=0) > d_best + t_best)
    g = got.astype(np.int64)
    valid = g < K
    gi = np.where(valid, g, 0)
    d_got, t_got = take(D, gi), take(tol, gi)
    with np.errstate(invalid="ignore"):
        near = valid & np.isfinite(d_got) & (d_got - d_best <= t_got + t_best)
    return dict(covered=covered, decided=decided, d_got=d_got, t_got=t_got,
                bad_decided=covered & decided & (g != best), bad_undecided=covered & ~decided & ~near, bad_uncovered=~covered & (got != prev),
                undecided_share=float((covered & ~decided).sum()) / max(1, int(covered.sum())))


def describe(mask, rows, *arrays):
    p = np.argwhere(mask)[:5]
    return "; ".join("(%d, %d): %s" % (rows[i], j, ", ".join(str(a[i, j]) for a in arrays)) for i, j in p)


def block_fixed_point(compactness):
    """The fixed point of a block's accumulators, restated from its rule (kernels.h, LscDev::blk_fix_*): the largest powers of two, never
    finer than the global 2^-20 / 2^-12, that keep 1024 pixels' sum of a feature inside 31 bits and of the biased weight inside 32; the
    bias is ceil(4 C_spatial^2).  Returns (bits_f, bits_w, f_max)."""
    C = 20.0
    Cs = C * compactness / 100.0
    f_max = max(C, 2.55 * C, abs(Cs))
    w_max = 2 * C * C + 4 * (2.55 * C) ** 2 + 4 * Cs * Cs
    bias = np.ceil(4 * Cs * Cs)
    bits_f = max(b for b in range(21) if b == 0 or 1024.0 * f_max * 2.0 ** b < 2.0 ** 31)
    bits_w = max(b for b in range(13) if b == 0 or 1024.0 * (w_max + bias) * 2.0 ** b < 2.0 ** 32)
    return bits_f, bits_w, f_max, w_max + bias


def update_bound(compactness, n, sw, w_abs_sum, C):
    """Bound of |cfeat - sum F / sum w| per cluster and component, from the fixed point (lsc.hip, "update(), fused").

    Numerator: a pixel's feature enters a block accumulator in units of 2^-bits_f, alone or after an f32 sum over the two rows of a pair
    or the eight pixels of a quad.  Alone: half a unit.  Summed: f_max < 64 keeps the eight-term total below 2^9, so the tree's seven
    roundings are at most 4 * 2^-18 + 2 * 2^-17 + 2^-16 = 3 * 2^-16 and the total lies on the grid -- 4 * 2^-16 for eight pixels, 1.25 *
    2^-16 for two: never more than half a unit (2^-16 at bits_f = 15) per pixel.  The `extra` path (2^-20) is finer.  The shift to the
    global 2^-20 is exact.
    Denominator: w is ten FMAs from zero, each rounding at most 2^-24 of sum_q |mean_q F_q|, plus the rounding of the bias add (2^-24 of
    w + bias <= w_cap); then half a unit of 2^-bits_w per pixel, alone or summed (w_cap < 2^14: the eight-term tree costs 4 * 2^-10 + 2 *
    2^-9 + 2^-8 = 3 * 2^-8, plus half a unit 2^-9 at bits_w = 8, over eight pixels: below half a unit each).
    Quotient: the two sums are converted to f32 (one rounding each) and divided (one more): 3 units of 2^-24, 4 with the second order.
    n: members, sw: the float64 sum of w, w_abs_sum: sum over the members of sum_q |mean_q F_q|, C: the float64 centroid [10]."""
    bits_f, bits_w, f_max, w_cap = block_fixed_point(compactness)
    assert f_max < 64 and w_cap < 2 ** 14
    e_num = n * 2.0 ** -(bits_f + 1)
    e_den = n * 2.0 ** -(bits_w + 1) + 10 * U * w_abs_sum + n * U * w_cap
    return (e_num + np.abs(C) * e_den) / (sw - e_den) + 4 * U * np.abs(C)


def check_trajectory(case, img, cl0, traj):
    """Stages a .. e.  Returns the measurement lines (also printed)."""
    H, W, K, n, stride = case["H"], case["W"], case["K"], case["n"], case["stride"]
    S = orc.S_of(H, W, K)
    states, planes, dists, rec_clusters = traj["states"], traj["planes"], traj["dists"], traj["rec_clusters"]
    lab = lsc_ref.lab_plane(img)
    F = lsc_ref.features(lab, lsc_ref.tables(H, W, S, case["c"]))
    lines = []

    def note(fmt, *a):
        lines.append(fmt % a)
        print(case["name"] + ": " + lines[-1])

    # ---- a. means
    means = states[0]["means"]
    for st in states:
        assert st["means"].tobytes() == means.tobytes(), "the means depend on max_iter"
    m64 = lsc_ref.feature_means(F)
    m_bound = 4 * U * np.abs(F).reshape(-1, 10).mean(axis=0)
    m_err = np.abs(means.astype(np.float64) - m64)
    note("a means: largest error %.3f of its bound", float(ratio(m_err, m_bound).max()))
    assert (m_err <= m_bound).all(), (means, m64, ratio(m_err, m_bound))

    # everything below: the model on the GPU's own means
    mg = means.astype(np.float64)
    w = lsc_ref.weights(F, mg)
    w_abs = np.abs(F) @ np.abs(mg)
    G = F / w[:, :, None]
    Gn2 = (G * G).sum(axis=-1)

    def centres(st):
        return lsc_ref.clamp_centres(st["y"], st["x"], H, W)

    # ---- b. seeds
    cy, cx = centres(states[0])
    seeds = lsc_ref.seed_centroids(G, cy, cx, S)
    q4 = S // 4
    s_bound = np.empty((K, 10))
    for k in range(K):
        win = np.abs(G[max(cy[k] - q4, 0):min(cy[k] + q4 + 1, H), max(cx[k] - q4, 0):min(cx[k] + q4 + 1, W)]).reshape(-1, 10)
        s_bound[k] = (win.shape[0] + 16) * U * win.mean(axis=0)
    s_err = np.abs(states[0]["cfeat"].astype(np.float64) - seeds)
    note("b seeds: largest error %.3f of its bound", float(ratio(s_err, s_bound).max()))
    assert (s_err <= s_bound).all(), "seed centroid of cluster %d: error / bound %s" % (int(np.argmax(ratio(s_err, s_bound).max(axis=1))), ratio(s_err, s_bound).max())

    # the recorder's cluster blocks are the plain runs' states (snapshot t + 1 = state t + 1; snapshot -1: the caller's positions)
    for m in range(1, n + 1):
        for f in ("y", "x", "colour", "members"):
            assert np.array_equal(rec_clusters[m][f], states[m][f]), "recorder snapshot %d, clusters' %s" % (m - 1, f)
    assert (planes[0] == lsc_ref.NONE).all(), "snapshot -1 carries labels"

    # ---- d. the subsampled passes, e. the updates
    n_stale = 0
    n_walk_blocks = 0
    nan_rows = 0
    for t in range(n):
        st = states[t]
        cy, cx = centres(st)
        C = st["cfeat"].astype(np.float64)
        rows = lsc_ref.visited_rows(H, t % stride, stride)
        other = np.setdiff1d(np.arange(H), rows)
        prev, cur, dist = planes[t], planes[t + 1], dists[t + 1]
        assert np.array_equal(cur[other], prev[other]), "iteration %d changed %d labels on rows it does not visit" % (t, int((cur[other] != prev[other]).sum()))
        assert (dist[other] == FLT_MAX_PRINTED).all(), "iteration %d: min-dists on unvisited rows" % t
        D = lsc_ref.distances(G, rows, cy, cx, C, S)
        j = judge_assignment(D, Gn2[rows], (C * C).sum(axis=1), cur[rows], prev[rows])
        cov = j["covered"]
        allowed = j["t_got"] + 5e-6 * np.abs(dist[rows])
        with np.errstate(invalid="ignore"):
            d_err = np.where(cov & np.isfinite(j["d_got"]), np.abs(dist[rows] - j["d_got"]) / allowed, 0.0)
        note("d iteration %d: undecided %.4f of %d covered, %d uncovered; largest min-dist error %.3f of its bound", t, j["undecided_share"], int(cov.sum()),
             int((~cov).sum()), float(d_err.max()))
        assert not j["bad_decided"].any(), "iteration %d: %d decided pixels carry another label than the model's: %s" % (
            t, int(j["bad_decided"].sum()), describe(j["bad_decided"], rows, cur[rows], np.argmin(D, axis=0)))
        assert not j["bad_undecided"].any(), "iteration %d: %d pixels carry a label that is no candidate within tolerance: %s" % (
            t, int(j["bad_undecided"].sum()), describe(j["bad_undecided"], rows, cur[rows], np.argmin(D, axis=0)))
        assert not j["bad_uncovered"].any(), "iteration %d: %d pixels no window reaches changed their label: %s" % (
            t, int(j["bad_uncovered"].sum()), describe(j["bad_uncovered"], rows, cur[rows], prev[rows]))
        assert j["undecided_share"] <= MAX_UNDECIDED
        assert (d_err <= 1.0).all(), "iteration %d: recorded min-dist off by %.3f of its bound: %s" % (t, float(d_err.max()), describe(d_err > 1.0, rows, dist[rows], j["d_got"]))
        assert (dist[rows][~cov] == FLT_MAX_PRINTED).all(), "iteration %d: min-dist of a pixel no window reaches" % t
        n_stale += int((~cov & (cur[rows] != lsc_ref.NONE)).sum())
        n_walk_blocks += blocks_over_64(cy, cx, S, H, W, rows)
        # e. state t + 1 from this plane
        nx = states[t + 1]
        ey, ex, ecol, en, eC = lsc_ref.update(cur, rows, lab, F, w, K, cy, cx, st["colour"], st["members"])
        for name, exp, got in (("y", ey, nx["y"]), ("x", ex, nx["x"]), ("colour", ecol, nx["colour"]), ("num_members", en, nx["members"])):
            assert np.array_equal(exp, got), "update %d: %s differs at clusters %s: %s, expected %s" % (
                t, name, np.argwhere(exp != got)[:4].tolist(), got[np.nonzero(exp != got)[0][:4]].tolist(), exp[np.nonzero(exp != got)[0][:4]].tolist())
        gC = nx["cfeat"].astype(np.float64)
        assert np.array_equal(np.isnan(gC).any(axis=1), en == 0) and np.array_equal(np.isnan(gC).all(axis=1), en == 0), "update %d: the NaN centroids are not the memberless clusters" % t
        nan_rows += int((en == 0).sum())
        lbl = cur[rows].astype(np.int64)
        ok = lbl != lsc_ref.NONE
        sw = np.bincount(lbl[ok], weights=w[rows][ok], minlength=K)
        swa = np.bincount(lbl[ok], weights=w_abs[rows][ok], minlength=K)
        worst, worst_rel, worst_n = 0.0, 0.0, 0
        for k in np.nonzero(en > 0)[0]:
            bound = update_bound(case["c"], float(en[k]), sw[k], swa[k], eC[k])
            rel = float(bound.max() / np.abs(eC[k]).max())
            assert rel <= 1e-4, "update %d cluster %d: the derived bound is %.3g relative: the case checks nothing" % (t, k, rel)
            err = ratio(np.abs(gC[k] - eC[k]), bound)
            assert (err <= 1.0).all(), "update %d: centroid of cluster %d (%d members) off by %.3f of its bound (%.3g relative): %s vs %s" % (
                t, k, en[k], float(err.max()), float(np.abs(gC[k] - eC[k]).max() / np.abs(eC[k]).max()), gC[k], eC[k])
            if float(err.max()) > worst:
                worst, worst_n = float(err.max()), int(en[k])
            worst_rel = max(worst_rel, rel)
        note("e update %d: largest centroid error %.3f of its bound, in a cluster of %d members (the bound: at most %.1f units of 2^-24 of max|C|); %d memberless",
             t, worst, worst_n, worst_rel / U, int((en == 0).sum()))

    # ---- c. the full assignment of every run
    rows = np.arange(H)
    n_final_stale = 0
    for m in range(n + 1):
        st = states[m]
        cy, cx = centres(st)
        C = st["cfeat"].astype(np.float64)
        D = lsc_ref.distances(G, rows, cy, cx, C, S)
        j = judge_assignment(D, Gn2, (C * C).sum(axis=1), st["pre"], planes[m])
        note("c full assignment under state %d: undecided %.4f of %d covered, %d uncovered (%d of them labelled earlier)", m, j["undecided_share"],
             int(j["covered"].sum()), int((~j["covered"]).sum()), int((~j["covered"] & (planes[m] != lsc_ref.NONE)).sum()))
        assert not j["bad_decided"].any(), "state %d: %d decided pixels carry another label than the model's: %s" % (
            m, int(j["bad_decided"].sum()), describe(j["bad_decided"], rows, st["pre"], np.argmin(D, axis=0)))
        assert not j["bad_undecided"].any(), "state %d: %d pixels carry a label that is no candidate within tolerance: %s" % (
            m, int(j["bad_undecided"].sum()), describe(j["bad_undecided"], rows, st["pre"], np.argmin(D, axis=0)))
        assert not j["bad_uncovered"].any(), "state %d: %d pixels no window reaches do not carry what they had: %s" % (
            m, int(j["bad_uncovered"].sum()), describe(j["bad_uncovered"], rows, st["pre"], planes[m]))
        assert j["undecided_share"] <= MAX_UNDECIDED
        n_final_stale += int((~j["covered"] & (st["pre"] != lsc_ref.NONE)).sum())
        n_walk_blocks += blocks_over_64(cy, cx, S, H, W, rows)

    # ---- that the case reaches what it is here for
    note("visited, labelled pixels no window reaches: %d ahead of an update, %d in full passes; blocks of more than 64 candidates: %d; NaN centroid rows: %d",
         n_stale, n_final_stale, n_walk_blocks, nan_rows)
    if case.get("want_walk"):
        assert n_walk_blocks >= 1, "no block of this case has more than 64 candidates"
    if case.get("want_stale"):
        assert n_stale >= 1, "no visited pixel of this case keeps a label whose window has left it"
    if case.get("want_nan"):
        assert nan_rows >= 1, "no cluster of this case loses all its members"
    return lines


def blocks_over_64(cy, cx, S, H, W, rows):
    """Blocks of 64 columns x 16 visited rows (the assign kernel's block) that more than 64 cluster windows reach."""
    count = 0
    for v0 in range(0, len(rows), 16):
        y_lo, y_hi = rows[v0], rows[min(v0 + 16, len(rows)) - 1]
        for x0 in range(0, W, 64):
            x_hi = min(x0 + 63, W - 1)
            reach = (cy + S >= y_lo) & (cy - S <= y_hi) & (cx + S >= x0) & (cx - S <= x_hi)
            count += int(reach.sum() > 64)
    return count


@pytest.mark.parametrize("name", list(CASES))
def test_lsc_stages(eng, name):
    case = dict(CASES[name], name=name)
    img = np.ascontiguousarray(variant(case["kind"], case["H"], case["W"]))
    cl0 = initial_clusters(case, img)
    check_trajectory(case, img, cl0, gpu_trajectory(eng, case, img, cl0))


@pytest.mark.parametrize("name", ["default_120x160_k40", "ragged_61x83_k20"])
def test_lsc_state_in_a_group_of_four_equals_single_runs(eng, name):
    case = dict(CASES[name], name=name)
    H, W, K = case["H"], case["W"], case["K"]
    imgs = [np.ascontiguousarray(variant(case["kind"], H, W, seed=s)) for s in range(4)]
    p = params(case, case["n"])
    singles = []
    for im in imgs:
        cl = initial_clusters(case, im)
        labels = eng.iterate(im, cl, p)
        singles.append((labels, cl) + eng.debug_lsc_state(K))
    with pytest.raises(ValueError):
        eng.debug_lsc_state(K, z=1)                 # the last group held one frame
    cls = [initial_clusters(case, im) for im in imgs]
    out = [np.zeros((H, W), np.uint16) for _ in imgs]
    eng.iterate_batch([im.ctypes.data for im in imgs], cls, [o.ctypes.data for o in out], H, W, p, False)
    assert eng.last_group_frames(0) == 4
    for z in range(4):
        means, cfeat = eng.debug_lsc_state(K, z=z)
        assert means.tobytes() == singles[z][2].tobytes(), "frame %d: means differ from the single run" % z
        assert cfeat.tobytes() == singles[z][3].tobytes(), "frame %d: centroids differ from the single run" % z
        assert np.array_equal(out[z], singles[z][0]) and cls[z].tobytes() == singles[z][1].tobytes(), "frame %d" % z
    with pytest.raises(ValueError):
        eng.debug_lsc_state(K, z=4)
    # a slot whose last group was not LSC has no LSC state
    eng.iterate(imgs[0], initial_clusters(case, imgs[0]), make_params(1, 10.0, 0.25, 3))
    with pytest.raises(ValueError):
        eng.debug_lsc_state(K)
