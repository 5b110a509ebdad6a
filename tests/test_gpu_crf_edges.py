"""SimpleCRF inference on the MI355X at the edges of its kernels, the tensor CRF's edge pass and sweep (crf.hip, crf_tensor.hip),
bit-equal to the reference's (tests/golden/crf_edge_cases.npz, crf_cases.EDGE_CASES, make_golden_crf.py): the sweep with its
messages in a plane of the CRF's workspace (more than 128 classes: 129, and the 255 to 300 classes around the cut of the kernels
SimpleCRF ran before) and with the largest LDS form (128 classes, 64 KB of dynamic LDS), 127 and 17 classes, one class, windows on
the block edges of both kernels, the clamp of the class sum, neighbour rows of thousands of entries, a window that grows, shrinks
and slides while q lives on the device, setters on the plane path, a CRF that changes its engine, and two plane-path CRFs on two
threads.  No tolerance anywhere: crf.h promises the reference's bits."""
import os
import threading

import numpy as np
import pytest

import crf_cases as CC
from fast_slic_amd import _binding as B
from test_gpu_crf import GOLD, build, check_q

pytestmark = pytest.mark.gpu
EDGE_GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crf_edge_cases.npz"))
_ENGINES = []                                 # engines a test made that a CRF may still be bound to when the test fails


def recorded(gold, name):
    """Every step of a case as the fixture holds it: one list of q per step, however many frames were live at that step."""
    steps = []
    while "%s/step%d/0" % (name, len(steps)) in gold.files:
        s, qs = len(steps), []
        while "%s/step%d/%d" % (name, s, len(qs)) in gold.files:
            qs.append(gold["%s/step%d/%d" % (name, s, len(qs))])
        steps.append(qs)
    return steps


@pytest.mark.parametrize("name", CC.EDGE_CASE_NAMES)
def test_edge_cases_match_the_reference(name):
    """Every recorded step of the case.  Reading q after an inference brings it to the host, so a replay that records every step
    never moves a frame whose q lives on the device alone: a case of several steps is replayed once more per step, reading q only
    after that step's inference (crf_cases.replay, only_step)."""
    case, frames = CC.unpack_frames(EDGE_GOLD, name)
    rec = CC.replay(CC.PkgCRF(case["C"], case["K"]), case, frames)
    exp = recorded(EDGE_GOLD, name)
    assert len(rec["steps"]) == len(exp) > 0
    for s, (qs, es) in enumerate(zip(rec["steps"], exp)):
        assert len(qs) == len(es), "%s step %d: %d frames, the fixture has %d" % (name, s, len(qs), len(es))
        check_q(qs, es, "%s step %d" % (name, s))
    for s in range(1, len(exp)):
        qs = CC.replay(CC.PkgCRF(case["C"], case["K"]), case, frames, only_step=s)["steps"][s]
        assert len(qs) == len(exp[s])
        check_q(qs, exp[s], "%s step %d, q unread until then" % (name, s))


def test_scratch_and_lds_forms_agree_with_a_fresh_twin():
    """test_setters_between_calls with the messages in the workspace's plane (257 classes): after two iterations one frame gets new
    unaries and one neighbour list grows (the index buffer and the workspace, which holds the per-entry energies and that plane, are
    allocated anew; the window's buffers stay), then two more iterations equal those of a deep copy taken before them, which uploads
    everything into buffers of its own."""
    rng = np.random.default_rng(11)
    case, crf, handles = build("c257_k65_t2_long", EDGE_GOLD)
    crf.inference(2)
    before = [f.get_inferred() for f in handles]
    handles[1].unaries = rng.uniform(0, 3, (case["C"], case["K"])).astype(np.float32)
    conn = handles[0].get_connectivity()
    conn[7] = conn[7] + [3, 3, 7, 64]
    handles[0].set_connectivity(conn)
    twin = crf.crf.copy()
    crf.inference(2)
    twin.inference(2)
    got = [f.get_inferred() for f in handles]
    exp = [twin.get_frame(f.time).get_inferred() for f in handles]
    check_q(got, exp, "after setters, messages in the workspace")
    assert not any(np.array_equal(g, b) for g, b in zip(got, before))


def test_rebinding_to_a_second_engine_carries_q():
    """4 iterations on the default engine, 3 on a second one (q comes home from the first engine's buffers, which are released, and
    goes up to the second's), 3 on the default one again: the fixture's 10 iterations."""
    lib = B.load_library()
    name = "k150_c21_t4"
    second = B.Engine(0, 1)
    _ENGINES.append(second)                   # outlives the CRF whatever happens below
    case, crf, handles = build(name)
    crf.inference(4)
    B._check(lib.fslic_hip_crf_inference(crf.crf._h, second._h, 3))
    crf.inference(3)
    got = [f.get_inferred() for f in handles]
    check_q(got, [GOLD["%s/step0/%d" % (name, j)] for j in range(case["T"])], "4 + 3 (second engine) + 3 iterations")
    del crf, handles                          # bound to the default engine again, and gone before `second` is
    _ENGINES.remove(second)
    second.close()


def test_two_scratch_path_crfs_on_two_threads():
    """The workspace with the message plane belongs to the CRF, not to the engine's slot: two CRFs with more than 128 classes infer
    side by side."""
    names = ["c257_k65_t2_long", "c300_k33_t3_slide"]
    out, errors = {}, []

    def work(name):
        try:
            case, frames = CC.unpack_frames(EDGE_GOLD, name)
            for _ in range(2):
                out.setdefault(name, []).append(CC.replay(CC.PkgCRF(case["C"], case["K"]), case, frames)["steps"])
        except Exception as e:               # pragma: no cover
            errors.append(e)
    th = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for name in names:
        exp = recorded(EDGE_GOLD, name)
        assert len(out[name]) == 2
        for steps in out[name]:
            assert len(steps) == len(exp)
            for s, (qs, es) in enumerate(zip(steps, exp)):
                check_q(qs, es, "%s step %d" % (name, s))
