"""SimpleCRF (fast_slic_amd.crf), the part that needs no GPU: the reference's test/test_crf.py surface, bookkeeping, errors, the host
setters / energies / reset_inferred bit-equal to the fixtures (tests/golden/crf_cases.npz and crf_edge_cases.npz, make_golden_crf.py),
what the edge fixtures claim to contain, crf_expf against the
host libm's expf, and -- where the reference sources are present -- the live reference on random cases."""
import gc
import os
import shutil
import tempfile
import threading
import zlib

import numpy as np
import pytest

import crf_cases as CC
from fast_slic_amd import _binding as B
from fast_slic_amd.crf import SimpleCRF, SimpleCRFFrame

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crf_cases.npz"))
EDGE_GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crf_edge_cases.npz"))


# ---- the reference's test/test_crf.py, restated --------------------------------------------------------------------------------------
def test_crf_basic():
    crf = SimpleCRF(3, 100)
    assert crf.space_size == 300
    assert crf.first_time == -1
    assert crf.last_time == -1
    assert crf.num_frames == 0
    with pytest.raises(IndexError):
        crf.get_frame(10)
    assert crf.pop_frame() == -1


def test_crf_frame():
    crf = SimpleCRF(3, 100)
    frame = crf.push_frame()
    assert crf.num_frames == 1
    assert crf.first_time == frame.time
    assert crf.last_time == frame.time
    assert frame.space_size == 300
    assert frame.time == 0
    assert crf.get_frame(0).time == 0
    assert frame.num_nodes == 100 and frame.num_classes == 3


def test_crf_frame_2():
    crf = SimpleCRF(3, 100)
    frame_1 = crf.push_frame()
    frame_2 = crf.push_frame()
    assert crf.num_frames == 2
    assert crf.first_time == frame_1.time
    assert crf.last_time == frame_2.time
    assert crf.pop_frame() == 0
    assert crf.first_time == crf.last_time == 1
    with pytest.raises(IndexError):
        frame_1.unaries                       # popped: the reference would read freed memory
    assert crf.push_frame().time == 2


def test_gc():
    crf = SimpleCRF(3, 100)
    frame = crf.push_frame()
    del crf
    gc.collect()
    frame.unaries
    frame.get_inferred()


def test_unaries():
    crf = SimpleCRF(3, 3)
    frame = crf.push_frame()
    frame.set_unbiased()
    assert (frame.unaries == np.float32(np.log(3))).all()      # (float32 logf; NumPy 2 compares in float64)
    frame.set_mask(np.array([0, 1, 2], np.int32), 0.5)
    exp_unaries = -np.log(np.array([[2 / 3., 1 / 6., 1 / 6.], [1 / 6., 2 / 3., 1 / 6.], [1 / 6., 1 / 6., 2 / 3.]]))
    assert np.isclose(frame.unaries, exp_unaries).all()
    prob = np.array([[0.7, 0.5, 0.1], [0.1, 0.3, 0.15], [0.2, 0.2, 0.75]], np.float32)
    frame.set_proba(prob)
    assert np.isclose(frame.unaries, -np.log(prob)).all()


def test_proba():
    crf = SimpleCRF(3, 3)
    frame = crf.push_frame()
    prob = np.array([[0.7, 0.5, 0.1], [0.1, 0.3, 0.15], [0.2, 0.2, 0.75]], np.float32)
    frame.set_proba(prob)
    assert np.isclose(frame.get_inferred(), 0).all()
    crf.initialize()
    assert np.isclose(frame.get_inferred(), prob).all()


def test_initial_inferred():
    crf = SimpleCRF(3, 3)
    frame = crf.push_frame()
    frame.set_unbiased()
    assert (frame.get_inferred() == 0).all()
    frame.reset_inferred()
    assert np.isclose(frame.get_inferred(), 1 / 3.).all()


def test_set_yxmrgb():
    crf = SimpleCRF(3, 3)
    frame = crf.push_frame()
    frame.set_yxmrgb(np.array([[1, 2, 1, 3, 4, 5], [6, 7, 2, 8, 9, 10], [11, 12, 3, 13, 14, 15]], np.int32))
    res = frame.get_yxmrgb()
    assert len(res) == 3
    assert res[0] == [1, 2, 1, 3, 4, 5]
    assert res[1] == [6, 7, 2, 8, 9, 10]
    assert res[2] == [11, 12, 3, 13, 14, 15]
    with pytest.raises(ValueError):
        frame.set_yxmrgb(np.zeros((3, 6), np.float64))
    with pytest.raises(ValueError):
        frame.set_yxmrgb(np.zeros((2, 6), np.int32))


def test_set_connectivity():
    crf = SimpleCRF(3, 3)
    frame = crf.push_frame()
    assert frame.get_connectivity() == [[], [], []]
    with pytest.raises(TypeError):
        frame.set_connectivity([None, None, None])
    frame.set_connectivity([[0, 1], [2], [0]])
    assert frame.get_connectivity() == [[0, 1], [2], [0]]
    with pytest.raises(ValueError):
        frame.set_connectivity([[0, 1]])
    with pytest.raises(ValueError):                 # index >= num_nodes: the reference indexes q with it unchecked
        frame.set_connectivity([[0, 3], [], []])
    assert frame.get_connectivity() == [[0, 1], [2], [0]]
    frame.set_connectivity(B.NodeConnectivity(np.array([2, 0, 1], np.int32), np.array([[1, 1], [0, 0], [2, 0]], np.uint32)))
    assert frame.get_connectivity() == [[1, 1], [], [2]]


def test_spatial_energy():
    spatial_srgb, spatial_w, spatial_sxy = 3.5, 1.9, 2.4
    crf = SimpleCRF(3, 2)
    crf.spatial_srgb = spatial_srgb
    crf.spatial_w = spatial_w
    crf.spatial_sxy = spatial_sxy
    assert np.isclose(crf.spatial_srgb, spatial_srgb)
    assert np.isclose(crf.spatial_w, spatial_w)
    assert np.isclose(crf.spatial_sxy, spatial_sxy)
    frame = crf.push_frame()
    frame.set_yxmrgb(np.array([[1, 1, 1, 1, 2, 6], [0, 0, 1, 4, 5, 3]], np.int32))
    energy = spatial_w * np.exp(-((1 - 4) ** 2 + (2 - 5) ** 2 + (6 - 3) ** 2) / (2 * spatial_srgb ** 2)
                                - ((1 - 0) ** 2 + (1 - 0) ** 2) / (2 * spatial_sxy ** 2))
    assert np.isclose(frame.spatial_pairwise_energy(0, 1), energy)
    assert np.isclose(frame.spatial_pairwise_energy(1, 0), energy)
    assert frame.spatial_pairwise_energy(0, 0) == 0
    assert frame.spatial_pairwise_energy(1, 1) == 0
    with pytest.raises(ValueError):
        frame.spatial_pairwise_energy(0, 2)


def test_temporal_energy():
    temporal_srgb, temporal_w = 3.5, 1.9
    crf = SimpleCRF(3, 1)
    crf.temporal_srgb = temporal_srgb
    crf.temporal_w = temporal_w
    assert np.isclose(crf.temporal_srgb, temporal_srgb)
    assert np.isclose(crf.temporal_w, temporal_w)
    frame_1 = crf.push_frame()
    frame_2 = crf.push_frame()
    frame_1.set_yxmrgb(np.array([[0, 0, 1, 1, 2, 6]], np.int32))
    frame_2.set_yxmrgb(np.array([[0, 0, 1, 4, 5, 3]], np.int32))
    energy = temporal_w * np.exp(-(((1 - 4) ** 2 + (2 - 5) ** 2 + (6 - 3) ** 2) / (2 * temporal_srgb ** 2)))
    assert np.isclose(frame_1.temporal_pairwise_energy(0, frame_2), energy)
    assert np.isclose(frame_2.temporal_pairwise_energy(0, frame_1), energy)
    assert frame_1.temporal_pairwise_energy(0, frame_1) == 0
    with pytest.raises(TypeError):
        frame_1.temporal_pairwise_energy(0, None)
    with pytest.raises(ValueError):
        frame_1.temporal_pairwise_energy(1, frame_2)


# ---- bookkeeping and errors ------------------------------------------------------------------------------------------------------
def test_params_defaults_and_compat():
    crf = SimpleCRF(4, 5)
    assert [getattr(crf, n) for n in CC.PARAM_NAMES] == [10, 10, 13, 13, 80, 0, 3]      # simple-crf.hpp:81-87
    assert [crf.get_compat(c) for c in range(4)] == [1, 1, 1, 1]
    crf.set_compat(2, 0.25)
    crf.spatial_smooth_w = 1.5
    assert crf.get_compat(2) == 0.25 and crf.spatial_smooth_w == 1.5
    with pytest.raises(ValueError):
        crf.set_compat(4, 1.0)
    cp = crf.copy()
    crf.set_compat(2, 3.0)
    assert cp.get_compat(2) == 0.25 and cp.spatial_smooth_w == 1.5


def test_invalid_sizes_and_inputs():
    with pytest.raises(ValueError):
        SimpleCRF(0, 10)
    with pytest.raises(ValueError):
        SimpleCRF(3, 0)
    with pytest.raises(ValueError):
        SimpleCRF(1 << 16, 1 << 16)                  # C * K overflows 32-bit indexing
    crf = SimpleCRF(3, 4)
    with pytest.raises(ValueError):
        crf.inference(1)                             # no frame (the reference dereferences a missing one)
    crf.inference(0)
    frame = crf.push_frame()
    with pytest.raises(ValueError):
        frame.set_mask(np.array([0, 1, 3, 0], np.int32), 0.5)
    with pytest.raises(ValueError):
        frame.set_mask(np.array([0, 1, 2], np.int32), 0.5)
    with pytest.raises(ValueError):
        frame.unaries = np.zeros((3, 4), np.float64)
    with pytest.raises(ValueError):
        frame.set_proba(np.ones((4, 3), np.float32))


def test_sliding_window_times():
    crf = SimpleCRF(2, 5)
    frames = [crf.push_frame() for _ in range(3)]
    assert [f.time for f in frames] == [0, 1, 2]
    assert crf.pop_frame() == 0
    f3 = crf.push_frame()
    assert f3.time == 3 and crf.first_time == 1 and crf.last_time == 3 and crf.num_frames == 3
    assert crf.get_frame(3).time == 3
    with pytest.raises(IndexError):
        crf.get_frame(0)
    assert (f3.get_inferred() == 0).all()


def test_frames_on_threads():
    errors = []

    def work(seed):
        try:
            rng = np.random.default_rng(seed)
            crf = SimpleCRF(3, 50)
            for _ in range(20):
                f = crf.push_frame()
                u = rng.uniform(0, 3, (3, 50)).astype(np.float32)
                f.unaries = u
                f.reset_inferred()
                assert np.array_equal(f.unaries, u)
                if crf.num_frames > 3:
                    crf.pop_frame()
        except Exception as e:               # pragma: no cover
            errors.append(e)
    th = [threading.Thread(target=work, args=(s,)) for s in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.CASE_NAMES + CC.EDGE_CASE_NAMES)
def test_host_side_matches_the_fixtures(name):
    """Unaries (host logf), spatial / temporal energies and reset_inferred (crf_expf) bit-equal to the reference's; max_iter 0 too.
    The edge cases (crf_edge_cases.npz) as well; one with a script up to its first inference."""
    gold = GOLD if name in CC.CASE_BY_NAME else EDGE_GOLD
    case, frames = CC.unpack_frames(gold, name)
    crf = CC.PkgCRF(case["C"], case["K"])
    rec = CC.replay(crf, case, frames, host_only=True)
    for j, u in enumerate(rec["unaries"]):
        key = "%s/f%d/unaries" % (name, j)
        exp = gold[key] if key in gold.files else frames[j]["udata"]
        assert u.tobytes() == exp.tobytes(), "frame %d unaries" % j
    assert rec["spatial"].tobytes() == gold[name + "/spatial"].tobytes()
    if case["T"] > 1:
        assert rec["temporal"].tobytes() == gold[name + "/temporal"].tobytes()
    for j, q in enumerate(rec["q0"]):
        assert q.tobytes() == gold["%s/q0/%d" % (name, j)].tobytes(), "frame %d after initialize / reset_inferred" % j
    if "steps" in rec:                                # max_iter 0: no GPU, nothing changes
        for j, q in enumerate(rec["steps"][0]):
            assert q.tobytes() == gold["%s/step0/%d" % (name, j)].tobytes()


def test_edge_cases_contain_what_they_claim():
    """The recorded q of the reference, not this package's: the clamp case really has clamped rows (their sum stays below 1), rows
    the clamp leaves alone, denormal entries and nothing that is not finite; the hub case has its two long rows, with duplicates and
    self-loops; the window case records one step per "infer" of its script with the window sizes the script goes through."""
    name = "clamp_c3_k130_t3"
    case = CC.EDGE_CASE_BY_NAME[name]
    q = np.stack([EDGE_GOLD["%s/step0/%d" % (name, j)] for j in range(case["T"])])          # [T][C][K]
    assert np.isfinite(q).all()
    sums = q.astype(np.float64).sum(axis=1).reshape(-1)
    assert sums.size == case["T"] * case["K"]
    assert np.count_nonzero(sums < 0.999) >= 0.2 * sums.size
    assert np.count_nonzero(np.abs(sums - 1.0) <= 1e-5) >= 0.2 * sums.size
    assert np.count_nonzero((q != 0) & (np.abs(q) < np.finfo(np.float32).tiny)) >= 1
    assert np.count_nonzero(q.max(axis=1) == 0) >= 1                                         # rows of zeros

    name = "hub_c5_k200_t2"
    K = CC.EDGE_CASE_BY_NAME[name]["K"]
    for j in range(2):
        off, idx = EDGE_GOLD["%s/f%d/off" % (name, j)], EDGE_GOLD["%s/f%d/idx" % (name, j)]
        for i in (0, K - 1):
            row = idx[off[i]:off[i + 1]]
            assert row.size == CC.HUB_ENTRIES and np.unique(row).size < row.size and (row == i).any()
        assert np.diff(off)[1:K - 1].max() <= 12

    name = "window_c3_k40"
    sizes = []
    s = 0
    while "%s/step%d/0" % (name, s) in EDGE_GOLD.files:
        sizes.append(sum(1 for k in EDGE_GOLD.files if k.startswith("%s/step%d/" % (name, s))))
        s += 1
    assert sizes == [2, 3, 1, 4, 4, 3]
    assert sizes == window_sizes(CC.EDGE_CASE_BY_NAME[name])


def window_sizes(case):
    """The number of live frames at each "infer" of a case's script."""
    T, out = case["T"], []
    for op in case["script"]:
        T += {"push": 1, "pop": -1}.get(op[0], 0)
        if op[0] == "infer":
            out.append(T)
    return out


# ---- crf_expf ------------------------------------------------------------------------------------------------------------------
def expf_pair(u32):
    lib = B.load_library()
    x = u32.view(np.float32)
    ours, libm = np.empty_like(x), np.empty_like(x)
    B._check(lib.fslic_hip_crf_expf_host(x.ctypes.data, ours.ctypes.data, x.size, 0))
    B._check(lib.fslic_hip_crf_expf_host(x.ctypes.data, libm.ctypes.data, x.size, 1))
    return ours.view(np.uint32), libm.view(np.uint32)


def test_crf_expf_equals_the_host_expf_on_a_strided_sample():
    """2^28 inputs, every 16th bit pattern (the whole 2^32: scripts/crf_expf_sweep.py)."""
    chunk = 1 << 24
    for c in range(16):
        u = (np.arange(chunk, dtype=np.uint64) + c * chunk) * 16 + 5
        ours, libm = expf_pair(u.astype(np.uint32))
        bad = np.nonzero(ours != libm)[0]
        assert bad.size == 0, "crf_expf differs at %d inputs, first 0x%08x" % (bad.size, int(u[bad[0]]))


def test_crf_expf_edges():
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0x42b17217, 0x42b17218,
                        0xc2cff1b4, 0xc2cff1b5, 0xc2ce8ed0, 0x42b00000, 0xc2b00000, 0x00000001, 0x3f800000], np.uint32)
    ours, libm = expf_pair(special)
    assert np.array_equal(ours, libm)


# ---- the live reference ----------------------------------------------------------------------------------------------------------
REF = os.environ.get("REF", "/root/reference")


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "src", "simple-crf.cpp")) or shutil.which("g++") is None,
                    reason="reference sources / g++ not present")
def test_live_reference_random_cases():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_crf as M
    tmp = tempfile.mkdtemp(prefix="fslic_crf_ref_")
    try:
        lib = M.build_reference(tmp)
        for seed in range(6):
            rng = np.random.default_rng(seed)
            case = dict(name="live%d" % seed, C=int(rng.integers(1, 8)), K=int(rng.integers(1, 300)), T=int(rng.integers(1, 4)),
                        iters=[2], graph=["none", "random", "long"][seed % 3], umode=["unary", "mask", "proba", "unbiased"],
                        init="initialize" if seed % 2 else "reset", params=list(rng.uniform(0.5, 40, 7).astype(np.float32).tolist()),
                        compat=list(rng.uniform(0, 2, 8).astype(np.float32).tolist()))
            case["compat"] = case["compat"][:case["C"]]
            if case["C"] == 1:
                case["umode"] = ["unary", "proba", "unbiased"]
            frames = CC.make_inputs(case, np.random.default_rng(zlib.crc32(case["name"].encode())))
            ref = M.RefCRF(lib, case["C"], case["K"])
            exp = CC.replay(ref, case, frames, host_only=True)
            ref.close()
            got = CC.replay(CC.PkgCRF(case["C"], case["K"]), case, frames, host_only=True)
            for key in ("unaries", "q0"):
                for a, b in zip(got[key], exp[key]):
                    assert a.tobytes() == b.tobytes(), (seed, key)
            assert got["spatial"].tobytes() == exp["spatial"].tobytes(), seed
            if case["T"] > 1:
                assert got["temporal"].tobytes() == exp["temporal"].tobytes(), seed
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
