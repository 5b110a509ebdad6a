"""SimpleCRF inference on the MI355X (crf.hip), bit-equal to the reference's (tests/golden/crf_cases.npz, make_golden_crf.py): every
fixture, repeated calls, setters between calls (the per-frame uploads), two CRFs on two threads, the Slic -> push_slic_frame chain,
and the device crf_expf against the host libm's expf."""
import os
import threading

import numpy as np
import pytest

import crf_cases as CC
from fast_slic_amd import _binding as B

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crf_cases.npz"))


def expected(name, step):
    case = CC.CASE_BY_NAME[name]
    n = case["T"]
    return [GOLD["%s/step%d/%d" % (name, step, j)] for j in range(n)]


def check_q(got, exp, what):
    for j, (g, e) in enumerate(zip(got, exp)):
        bad = np.count_nonzero(g.view(np.uint32) != e.view(np.uint32))
        assert bad == 0, "%s: frame %d differs at %d of %d entries" % (what, j, bad, g.size)


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_inference_matches_the_reference(name):
    case, frames = CC.unpack_frames(GOLD, name)
    rec = CC.replay(CC.PkgCRF(case["C"], case["K"]), case, frames)
    for s, qs in enumerate(rec["steps"]):
        check_q(qs, expected(name, s), "%s step %d" % (name, s))


def build(name, gold=GOLD):
    case, frames = CC.unpack_frames(gold, name)
    crf = CC.PkgCRF(case["C"], case["K"])
    if case.get("params"):
        crf.set_params(case["params"])
    for cls, v in enumerate(case.get("compat") or []):
        crf.set_compat(cls, v)
    handles = []
    for j in range(case["T"]):
        f = crf.push()
        CC._fill(crf, f, frames[j])
        handles.append(f)
    crf.initialize()
    return case, crf, handles


def test_repeated_calls_equal_one_longer_call():
    case, crf, handles = build("k150_c21_t4")
    crf.inference(4)
    [f.get_inferred() for f in handles[:1]]          # a read in between (q comes home, stays current on the device)
    crf.inference(1)
    crf.inference(5)
    check_q([f.get_inferred() for f in handles], expected("k150_c21_t4", 0), "4 + 1 + 5 iterations")


def test_setters_between_calls():
    """A CRF changed after an inference (unaries, clusters, neighbour lists, params, compat, q of one frame) and inferred again equals
    a deep copy of it inferred from scratch (the copy uploads everything, the original only what changed)."""
    rng = np.random.default_rng(5)
    case, crf, handles = build("slic300_c3_t4")
    crf.inference(3)
    K, C = case["K"], case["C"]
    handles[1].unaries = rng.uniform(0, 3, (C, K)).astype(np.float32)
    cl = handles[2].get_clusters()
    cl["r"] += np.float32(4.5)
    handles[2].set_clusters(cl)
    conn = handles[3].get_connectivity()
    conn[0] = conn[0] + [1, 1, 0]
    handles[3].set_connectivity(conn)
    crf.crf.spatial_w = 7.5
    crf.crf.set_compat(1, 0.5)
    handles[0].reset_inferred()
    twin = crf.crf.copy()
    crf.inference(3)
    twin.inference(3)
    got = [f.get_inferred() for f in handles]
    exp = [twin.get_frame(f.time).get_inferred() for f in handles]
    check_q(got, exp, "after setters")
    assert not all(np.array_equal(g, GOLD["slic300_c3_t4/step0/%d" % j]) for j, g in enumerate(got))


def test_two_crfs_on_two_threads():
    names = ["k150_c21_t4", "slic150_c21_t2"]
    out, errors = {}, []

    def work(name):
        try:
            for _ in range(3):
                case, crf, handles = build(name)
                crf.inference(case["iters"][0])
                out.setdefault(name, []).append([f.get_inferred() for f in handles])
        except Exception as e:               # pragma: no cover
            errors.append(e)
    th = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for name in names:
        for qs in out[name]:
            check_q(qs, expected(name, 0), name)


def test_slic_chain_push_slic_frame():
    """Slic(K).iterate(img) -> push_slic_frame x 4 -> inference(10), against the reference on the same clusters and neighbour lists."""
    from fast_slic_amd import Slic
    from fast_slic_amd.crf import SimpleCRF
    from fast_slic_amd.synth import variant
    name = "chain_k100_c3_t4"
    case, frames = CC.unpack_frames(GOLD, name)
    crf = SimpleCRF(case["C"], case["K"])
    handles = []
    for j, v in enumerate(CC.CHAIN_VARIANTS):
        slic = Slic(num_components=CC.CHAIN_K)
        slic.iterate(variant(v, CC.CHAIN_H, CC.CHAIN_W, seed=3))
        f = crf.push_slic_frame(slic)
        assert f.get_clusters().tobytes() == frames[j]["clusters"].tobytes(), "Slic clusters of frame %d" % j
        off, idx = frames[j]["off"], frames[j]["idx"]
        assert f.get_connectivity() == [list(map(int, idx[off[i]:off[i + 1]])) for i in range(case["K"])]
        f.set_mask(frames[j]["udata"], frames[j]["conf"])
        handles.append(f)
    crf.initialize()
    crf.inference(10)
    check_q([f.get_inferred() for f in handles], expected(name, 0), name)


def test_device_expf_equals_the_host_expf():
    """2^24 inputs across the whole float range (every 256th bit pattern, offset 131)."""
    lib = B.load_library()
    eng = B.default_engine(0)
    u = (np.arange(1 << 24, dtype=np.uint64) * 256 + 131).astype(np.uint32)
    x = u.view(np.float32)
    dev, host = np.empty_like(x), np.empty_like(x)
    B._check(lib.fslic_hip_crf_expf_device(eng._h, x.ctypes.data, dev.ctypes.data, x.size))
    B._check(lib.fslic_hip_crf_expf_host(x.ctypes.data, host.ctypes.data, x.size, 1))
    bad = np.nonzero(dev.view(np.uint32) != host.view(np.uint32))[0]
    assert bad.size == 0, "device crf_expf differs at %d inputs, first 0x%08x: 0x%08x vs 0x%08x" % (
        bad.size, int(u[bad[0]]), int(dev.view(np.uint32)[bad[0]]), int(host.view(np.uint32)[bad[0]]))
