"""Overlapped groups of the submit / drain pipeline (DESIGN.md "Overlapped groups"; pipeline.cpp: slot_worker, group.cpp: group_wait /
group_complete).

A slot thread begins the next submission of the same work behind the group it still has running and collects the running one
afterwards, on the slot's other pinned set.  Nothing a caller sees may depend on it: every label map and every Cluster byte is compared
with the oracle and with the same submissions driven one by one (submit_group / wait_group: depth one).  Engine.overlapped_groups
proves that the path ran -- or, where the rules decline it, that it did not.

Shapes: two frames of 160x96 with K = 40 (the block kernel; tests/test_gpu_assign_forms.py), two of 640x360 for the host top-K step, the 8 x 540x960 K = 900 group of
tests/test_gpu_deferred_labels.py where the label-free passes and their redo are the point, one 8 x 1280x720 K = 1600 group where the
replay of the benched sequence is.
"""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as orc
from fast_slic_amd import _binding as B
from fast_slic_amd import make_params
from fast_slic_amd.synth import variant
from util import describe_mismatch, cluster_fields_equal

pytestmark = pytest.mark.gpu

GRAPHS_OFF = os.environ.get("FSLIC_GRAPH") == "0"


@functools.lru_cache(maxsize=None)
def ref(kind, H, W, K, seed, max_iter=10, stride=3, min_size_factor=0.25, scatter=None, compactness=10.0):
    """One frame, its seeds and the oracle's label map and Cluster block: computed once per distinct frame and left unchanged."""
    img = variant(kind, H, W, seed=seed)
    cl0 = orc.initialize_clusters(img, K)
    if scatter is not None:      # centres anywhere in the frame (tests/test_gpu_deferred_labels.py: reference)
        rng = np.random.RandomState(scatter)
        cl0["y"] = rng.randint(0, H, K).astype(np.float32)
        cl0["x"] = rng.randint(0, W, K).astype(np.float32)
    labels, cl = orc.slic_iterate(img, cl0.copy(), max_iter=max_iter, compactness=compactness, subsample_stride=stride, min_size_factor=min_size_factor)[:2]
    for a in (img, cl0, labels, cl):
        a.setflags(write=False)
    return img, cl0, labels, cl


class Sub:
    """One submission: its frames on the device, its own label maps and Cluster blocks, and the parameters it asks for."""

    def __init__(self, e, refs, max_iter=10, stride=3, min_size_factor=0.25, cache=None, compactness=10.0):
        import torch
        self.refs = refs
        self.H, self.W = refs[0][0].shape[:2]
        self.K = refs[0][1].shape[0]
        self.p = make_params(max_iter, compactness, min_size_factor, stride)
        cache = {} if cache is None else cache
        self.d_rgb = [cache.setdefault(id(r[0]), torch.from_numpy(np.array(r[0])).cuda()) for r in refs]
        self.d_lab = torch.full((len(refs), self.H, self.W), -7, dtype=torch.int16, device="cuda")
        self.cls = np.stack([r[1].copy().view(B.CLUSTER_DTYPE) for r in refs])
        self.arrays = (e.pointer_array([t.data_ptr() for t in self.d_rgb]),
                       e.pointer_array([self.cls[i].ctypes.data for i in range(len(refs))]),
                       e.pointer_array([self.d_lab[i].data_ptr() for i in range(len(refs))]))

    def args(self):
        return self.arrays + (len(self.refs), self.H, self.W, self.K, self.p)

    def check(self, tag):
        got = self.d_lab.cpu().numpy().view(np.uint16)
        for i, r in enumerate(self.refs):
            assert np.array_equal(got[i], r[2]), describe_mismatch("%s frame %d" % (tag, i), got[i], r[2])
            assert self.cls[i].tobytes() == r[3].tobytes(), "%s frame %d: %s" % (tag, i, "; ".join(cluster_fields_equal(self.cls[i], r[3])))


def through_pipeline(e, subs, tag):
    import torch
    torch.cuda.synchronize()
    for s in subs:
        e.pipeline_submit(*s.args())
    tot = e.pipeline_drain()
    assert tot["groups"] == len(subs) and tot["frames"] == sum(len(s.refs) for s in subs), tot
    for j, s in enumerate(subs):
        s.check("%s, submission %d" % (tag, j))
    return tot


def one_by_one(e, subs, tag, slot=0):
    """The same submissions at depth one; returns the frames that took the host's top-K step."""
    import torch
    torch.cuda.synchronize()
    topk = 0
    for j, s in enumerate(subs):
        e.submit_group(slot, *s.args())
        e.wait_group(slot)
        topk += e.last_host_topk_frames(slot)
        s.check("%s, submission %d" % (tag, j))
    return topk


def small(kind, seed, **kw):
    return ref(kind, 96, 160, 40, seed, **kw)


def topk_frame(seed, min_size_factor):
    return ref("A", 360, 640, 400, seed, min_size_factor=min_size_factor)


def same_work_run(overlap, n_subs=12):
    """n_subs submissions of one work on two slots; the counter after the drain."""
    from fast_slic_amd import Engine
    frames = [[small("A", 1), small("B", 2)], [small("B", 3), small("A", 4)], [small("A", 5), small("A", 1)]]
    e = Engine(0, 2)
    try:
        e.pipeline_overlap(overlap)
        cache = {}
        subs = [Sub(e, frames[j % 3], cache=cache) for j in range(n_subs)]
        through_pipeline(e, subs, "pipeline")
        again = [Sub(e, frames[j % 3], cache=cache) for j in range(n_subs)]
        one_by_one(e, again, "one by one")
        for a, b in zip(subs, again):
            assert np.array_equal(a.d_lab.cpu().numpy(), b.d_lab.cpu().numpy()) and a.cls.tobytes() == b.cls.tobytes()
        return e.overlapped_groups()
    finally:
        e.close()


def test_overlapped_submissions_equal_the_serial_ones_and_the_oracle():
    assert same_work_run(True) > 0


def test_the_switch_gives_the_serial_loop():
    """Engine.pipeline_overlap(False): the same submissions, nothing begun behind a running group; and on again on the same engine."""
    from fast_slic_amd import Engine
    assert same_work_run(False) == 0
    a = [small("A", 1), small("B", 2)]
    e = Engine(0, 1)
    try:
        e.pipeline_overlap(False)
        through_pipeline(e, [Sub(e, a) for _ in range(5)], "off")
        assert e.overlapped_groups() == 0
        e.pipeline_overlap(True)
        through_pipeline(e, [Sub(e, a) for _ in range(5)], "on again")
        assert e.overlapped_groups() > 0
    finally:
        e.close()


def test_a_flagged_frame_is_redone_after_its_successor():
    """Scattered centres leave visited pixels uncovered in a label-free group (tests/test_gpu_deferred_labels.py): the frames come back
    flagged while the next group is already running over the slot's device state.  The successor is collected first, the flagged
    frames are computed again with storing passes; the counter moves as in the serial run and every submission is the oracle's."""
    from fast_slic_amd import Engine
    H, W, K, stride, max_iter = 540, 960, 900, 3, 4
    grid = [ref("A", H, W, K, 11, max_iter, stride), ref("B", H, W, K, 12, max_iter, stride)] * 4
    scat = [ref("A", H, W, K, 11, max_iter, stride, scatter=40), ref("B", H, W, K, 12, max_iter, stride, scatter=41)] * 4
    order = [grid, grid, scat, grid, grid, grid]
    counts = []
    for run in (through_pipeline, one_by_one):
        e = Engine(0, 1)
        try:
            cache = {}
            run(e, [Sub(e, refs, max_iter, stride, cache=cache) for refs in order], run.__name__)
            counts.append(e.uncovered_redos())
            if run is through_pipeline:
                assert e.overlapped_groups() > 0
        finally:
            e.close()
    assert counts[0] == counts[1] > 0, counts


def test_host_topk_frames_in_the_middle_of_a_run():
    """min_size_factor = 0 makes every component a candidate, more than the device sorts at 640x360 (tests/test_gpu_pipeline.py): the
    frames want the host's partial_sort after a successor has run over their candidate lists."""
    from fast_slic_amd import Engine
    plain = [topk_frame(1, 0.25), topk_frame(2, 0.25)]
    zero = [topk_frame(1, 0.0), topk_frame(2, 0.0)]
    msf = [0.25, 0.25, 0.0, 0.0, 0.25, 0.0, 0.25, 0.25]
    e = Engine(0, 1)
    try:
        cache = {}
        mk = lambda: [Sub(e, zero if m == 0.0 else plain, min_size_factor=m, cache=cache) for m in msf]
        tot = through_pipeline(e, mk(), "pipeline")
        assert e.overlapped_groups() > 0
        serial = one_by_one(e, mk(), "one by one")
        assert tot["host_topk_frames"] == serial > 0, (tot, serial)
    finally:
        e.close()


def test_same_work_with_host_topk_in_every_group_overlaps():
    from fast_slic_amd import Engine
    zero = [topk_frame(1, 0.0), topk_frame(2, 0.0)]
    e = Engine(0, 1)
    try:
        tot = through_pipeline(e, [Sub(e, zero, min_size_factor=0.0) for _ in range(5)], "pipeline")
        assert tot["host_topk_frames"] == 10 and e.overlapped_groups() > 0
    finally:
        e.close()


def test_other_work_is_never_begun_behind_a_running_group():
    """One slot, so every submission follows its predecessor on the same stream: alternating shapes, alternating iteration counts,
    a generic-kernel shape (S < 8) between block-kernel ones.  No pair may be counted, and everything is the oracle's."""
    from fast_slic_amd import Engine
    e = Engine(0, 1)
    try:
        a = [small("A", 1), small("B", 2)]
        b = [ref("A", 112, 128, 36, 6), ref("B", 112, 128, 36, 7)]
        a4 = [small("A", 1, max_iter=4), small("B", 2, max_iter=4)]
        gen = [ref("A", 40, 63, 100, 8), ref("B", 40, 63, 100, 9)]
        through_pipeline(e, [Sub(e, r) for r in (a, b, a, b, a, b)], "shapes")
        through_pipeline(e, [Sub(e, a4 if j & 1 else a, max_iter=4 if j & 1 else 10) for j in range(6)], "max_iter")
        through_pipeline(e, [Sub(e, r) for r in (a, gen, a, gen, a)], "generic between")
        assert e.overlapped_groups() == 0
        # The sequences above also change the workload the slot thread keeps its flight history for, so it never even looks for a
        # successor.  Another compactness is another work (same_work compares the parameter block) under the SAME history: the thread
        # looks at the queue behind every one of these groups, and only the comparison of the work declines the head.
        c20 = [small("A", 1, compactness=20.0), small("B", 2, compactness=20.0)]
        through_pipeline(e, [Sub(e, a) for _ in range(2)], "history")
        before = e.overlapped_groups()
        through_pipeline(e, [Sub(e, c20 if j & 1 else a, compactness=20.0 if j & 1 else 10.0) for j in range(8)], "compactness")
        assert e.overlapped_groups() == before
        through_pipeline(e, [Sub(e, a) for _ in range(4)], "same work at last")
        assert e.overlapped_groups() > 0
    finally:
        e.close()


def test_nothing_is_recorded_in_the_steady_state():
    """bench.py's order: three explicit rounds per slot (direct, recorded, replayed), then submissions to the queue.  Every later group
    replays the slot's one recorded sequence, whichever pinned set it runs on."""
    from fast_slic_amd import Engine
    H, W, K = 720, 1280, 1600
    refs = [ref("A", H, W, K, 0), ref("A", H, W, K, 1)] * 4
    e = Engine(0, 2)
    try:
        cache = {}
        for slot in range(2):
            one_by_one(e, [Sub(e, refs, cache=cache) for _ in range(3)], "setup, slot %d" % slot, slot)
            assert e.last_launch_mode(slot) == 2 or GRAPHS_OFF
        # last_launch_mode shows a slot's last begun group only; the form record shows EVERY launch that is enqueued directly or recorded
        # into a graph (a replay notes nothing, DESIGN.md "The form record"): it must stay empty over all the later groups
        B.forms_seen(clear=True)
        for rnd in range(3):      # (an odd number of groups per slot and round: both sets meet both positions)
            through_pipeline(e, [Sub(e, refs, cache=cache) for _ in range(6)], "round %d" % rnd)
            assert [e.last_launch_mode(s) for s in range(2)] == [2, 2] or GRAPHS_OFF
        assert B.forms_seen() == set() or GRAPHS_OFF, sorted(B.forms_seen())
        assert e.overlapped_groups() > 0
    finally:
        e.close()


def test_odd_counts_drain_and_reuse():
    from fast_slic_amd import Engine
    a = [small("A", 1), small("B", 2)]
    e = Engine(0, 2)
    try:
        cache = {}
        for n in (1, 3, 7):
            through_pipeline(e, [Sub(e, a, cache=cache) for _ in range(n)], "%d submissions" % n)
        img, cl0, labels, cl = a[0]
        got_cl = cl0.copy().view(B.CLUSTER_DTYPE)
        got = e.iterate(np.array(img), got_cl, make_params(10, 10.0, 0.25, 3))
        assert np.array_equal(got, labels) and got_cl.tobytes() == cl.tobytes()
        through_pipeline(e, [Sub(e, a, cache=cache) for _ in range(4)], "after a synchronous call")
        assert e.pipeline_drain()["groups"] == 0
    finally:
        e.close()


# what fslic_hip_debug_fail_group makes fail (engine_internal.h), and the submission of the run it is armed for
FAILURES = {"begin_untouched": 0, "begin_enqueued": 1, "complete": 2}


@pytest.mark.parametrize("point", list(FAILURES))
def test_a_failing_group_is_reported_once_and_the_engine_goes_on(point):
    """One group of a run fails on the slot thread while its neighbours are in flight on the same stream (a testing aid makes it fail:
    every failure an input can cause is caught on the caller's thread first).  Nothing faults on the device.  The drain returns, reports
    the error once, every other submission that was accepted is the oracle's -- the predecessor that was running when the begin failed,
    the successor that was already enqueued when the finish failed -- and the next run on the same engine is served in full."""
    from fast_slic_amd import Engine
    lib = B.load_library()
    a = [small("A", 1), small("B", 2)]
    e = Engine(0, 1)
    try:
        cache = {}
        through_pipeline(e, [Sub(e, a, cache=cache) for _ in range(3)], "history")
        before = e.overlapped_groups()
        k = 3
        assert lib.fslic_hip_debug_fail_group(e._h, FAILURES[point], k) == 0
        import torch
        torch.cuda.synchronize()
        subs, accepted = [Sub(e, a, cache=cache) for _ in range(8)], []
        for j, s in enumerate(subs):
            try:
                e.pipeline_submit(*s.args())      # (refused once the error is known: it is reported again by the drain)
                accepted.append(j)
            except RuntimeError:
                break
        assert k in accepted
        with pytest.raises(RuntimeError, match="testing aid"):
            e.pipeline_drain()
        tot = e.pipeline_drain()                  # reported once; nothing is left in flight on either set
        assert tot["groups"] == 0 and tot["frames"] == 0
        for j in accepted:
            if j != k:
                subs[j].check("%s, submission %d beside the failing one" % (point, j))
        assert e.overlapped_groups() > before     # the failing group had neighbours on the stream
        through_pipeline(e, [Sub(e, a, cache=cache) for _ in range(6)], "the next run")
        img, cl0, labels, cl = a[0]
        got_cl = cl0.copy().view(B.CLUSTER_DTYPE)
        assert np.array_equal(e.iterate(np.array(img), got_cl, make_params(10, 10.0, 0.25, 3)), labels) and got_cl.tobytes() == cl.tobytes()
    finally:
        e.close()

