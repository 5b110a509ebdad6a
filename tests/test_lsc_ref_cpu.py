"""The float64 LSC model (tests/lsc_ref.py) against the reference's own fixtures (tests/golden/lsc_cases.npz, the unmodified
`fast_slic.LSC`, arch "standard", one thread): run end to end it must agree with them at least as well as tests/test_gpu_lsc.py asks
of the HIP kernels.  That makes the model the reference's operation and not a restatement of lsc.hip, which is what lets
tests/test_gpu_lsc_stages.py use it as the yardstick of every stage.  No GPU."""
import json
import os

import numpy as np
import pytest

import lsc_ref
from fast_slic_amd.synth import variant
from oracle import oracle as orc
from util import best_overlap, boundary_iou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tests/test_gpu_lsc.py: FLOORS["default"], CENTRE_SHIFT_FLOOR_PX, and the seed-only floor
PRE_AGREE, BEST_OVERLAP, BOUNDARY_IOU, CENTRE_SHIFT_PX, SEED_ONLY_AGREE = 0.99, 0.99, 0.95, 0.1, 0.995

SMALL_CASES = ["A_120x160_k40", "A_97x131_k25_rgb", "B_200x150_k30_stride2_c20", "D_128x192_k16_iter3", "A_96x128_k300_small_S"]


@pytest.fixture(scope="module")
def lsc_cases():
    return np.load(os.path.join(ROOT, "tests", "golden", "lsc_cases.npz"), allow_pickle=False)


def model_run(cases, name):
    H, W, K = (int(v) for v in cases[name + "/shape"])
    kw = json.loads(str(cases[name + "/kwargs"]))
    img = variant(str(cases[name + "/variant"]), H, W)
    pre, cy, cx, members = lsc_ref.run(img, orc.initialize_clusters(img, K), kw.get("max_iter", 10), kw.get("compactness", 10.0),
                                       kw.get("subsample_stride", 3), kw.get("convert_to_lab", True))
    S = orc.S_of(H, W, K)
    labels = orc.enforce_connectivity(pre, K, int(round(float(S * S) * kw.get("min_size_factor", 0.25))))
    return pre, labels, cy, cx, members


@pytest.mark.parametrize("name", SMALL_CASES)
def test_model_reproduces_reference_fixture(lsc_cases, name):
    pre, labels, cy, cx, members = model_run(lsc_cases, name)
    r_labels, r_pre, r_cl = lsc_cases[name + "/labels"], lsc_cases[name + "/prelabels"], lsc_cases[name + "/clusters"]
    agree = float((pre == r_pre).mean())
    bo = min(best_overlap(labels, r_labels), best_overlap(r_labels, labels))
    iou = boundary_iou(labels, r_labels)
    dyx = float(np.mean(np.hypot(cy - r_cl["y"], cx - r_cl["x"])))
    print("%s: pre-agree %.4f best-overlap %.4f boundary-IoU %.4f mean centre shift %.3f px" % (name, agree, bo, iou, dyx))
    assert agree >= PRE_AGREE and bo >= BEST_OVERLAP and iou >= BOUNDARY_IOU and dyx <= CENTRE_SHIFT_PX, (agree, bo, iou, dyx)


def test_model_seed_only_pass(lsc_cases):
    name = "A_150x200_k50_iter0"
    pre = model_run(lsc_cases, name)[0]
    agree = float((pre == lsc_cases[name + "/prelabels"]).mean())
    print("%s: pre-agree %.5f" % (name, agree))
    assert agree >= SEED_ONLY_AGREE, agree


def test_tables_follow_the_reference_expressions():
    # spot values by hand: theta = 0 gives C, 0; X = 255 gives theta = halfPI (float32 of 3.1415926 / 2)
    t = lsc_ref.tables(40, 50, 7, 10.0)
    assert t["L_cos"][0] == np.float32(20.0) and t["L_sin"][0] == 0.0 and t["x_cos"][0] == np.float32(2.0) and t["y_sin"][0] == 0.0
    half_pi = float(np.float32(np.float32(3.1415926) / np.float32(2)))
    assert t["L_sin"][255] == np.float32(20.0 * np.sin(half_pi))
    assert t["ab_cos"][0] == np.float32(np.float32(20.0) * np.float32(2.55))
    th = float(np.float32(np.float32(3) * np.float32(np.float32(half_pi) / np.float32(7))))
    assert t["x_sin"][3] == np.float32(2.0 * np.sin(th)) and t["y_cos"][3] == np.float32(2.0 * np.cos(th))
    assert all(v.dtype == np.float32 for v in t.values())


def test_update_and_assign_by_hand():
    # 4 x 6 plane, two clusters, S = 1: windows, the keep-previous rule, round_int, NaN centroid of a memberless cluster
    H, W, K, S = 4, 6, 3, 1
    rng = np.random.RandomState(1)
    G = rng.rand(H, W, 10)
    cy, cx = np.array([1, 2, 0]), np.array([1, 4, 0])
    C = np.stack([G[1, 1], G[2, 4], np.full(10, np.nan)])
    rows = np.arange(H)
    D = lsc_ref.distances(G, rows, cy, cx, C, S)
    assert np.isinf(D[2]).all() and np.isfinite(D[0][0:3, 0:3]).all() and np.isinf(D[0][3]).all() and np.isinf(D[0][:, 3:]).all()
    assert D[0][1, 1] == 0.0 and D[1][2, 4] == 0.0 and np.isclose(D[0][0, 2], ((G[0, 2] - G[1, 1]) ** 2).sum())
    prev = np.full((H, W), 7, np.uint16)
    labels, covered = lsc_ref.assign(D, lsc_ref.visit_rank(cy, cx, S, H, W), prev)
    assert (labels[~covered] == 7).all() and labels[1, 1] == 0 and labels[2, 4] == 1 and not covered[3, 0] and covered[0, 0]
    lab = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    F, w = rng.rand(H, W, 10), 1.0 + rng.rand(H, W)
    plane = np.full((H, W), lsc_ref.NONE, np.uint16)
    plane[0, 0:3] = 0
    plane[2, 1] = 0
    plane[1, 5] = 0           # (not a visited row below)
    ny, nx, col, n, C2 = lsc_ref.update(plane, [0, 2], lab, F, w, K, cy, cx, np.zeros((K, 3), np.int64), np.zeros(K, np.int64))
    assert list(n) == [4, 0, 0] and ny[0] == (2 + 2) // 4 and nx[0] == (0 + 1 + 2 + 1 + 2) // 4 and (ny[1], nx[1]) == (2, 4)
    members = [(0, 0), (0, 1), (0, 2), (2, 1)]
    assert col[0, 0] == (sum(int(lab[p][0]) for p in members) + 2) // 4
    assert np.isnan(C2[1]).all() and np.isnan(C2[2]).all()
    assert np.allclose(C2[0], sum(F[p] for p in members) / sum(w[p] for p in members), rtol=1e-14)
