"""SimpleCRF cases shared by the fixture maker (tests/golden/make_golden_crf.py, against the reference) and the tests (against this
package): the case list, the deterministic inputs of a case, and one replay of a case against either implementation."""
import json

import numpy as np

PARAM_NAMES = ("spatial_w", "temporal_w", "spatial_srgb", "temporal_srgb", "spatial_sxy", "spatial_smooth_w", "spatial_smooth_sxy")

CHAIN_H, CHAIN_W, CHAIN_K = 120, 160, 100
CHAIN_VARIANTS = ("A", "B", "C", "D")

# graph: "none" (no neighbours), "small" (self-loops, duplicates), "random" (<= 12 random neighbours), "long" (up to 20 with
# duplicates, empty lists, clusters with num_members 0), "slic150" / "slic300" (graph_cases.npz's reference clusters and
# connectivity), "chain" (Slic on four frames, see make_golden_crf.chain_inputs)
CASES = [
    dict(name="k1_c2_t1", C=2, K=1, T=1, iters=[3], graph="none", umode=["unary"], init="initialize"),
    dict(name="k3_c3_t2", C=3, K=3, T=2, iters=[10], graph="small", umode=["mask", "proba"], init="initialize"),
    dict(name="k3_c2_t2_iter0", C=2, K=3, T=2, iters=[0], graph="small", umode=["unary"], init="initialize"),
    dict(name="k150_c21_t4", C=21, K=150, T=4, iters=[10], graph="random", umode=["proba"], init="initialize"),
    dict(name="k150_c3_t2_smooth", C=3, K=150, T=2, iters=[1], graph="random", umode=["unary"], init="initialize",
         params=[3.5, 7.25, 9.0, 17.0, 31.0, 2.5, 4.5], compat=[0.5, 1.75, 1.0]),
    dict(name="k1600_c2_t4_long", C=2, K=1600, T=4, iters=[3], graph="long", umode=["unary", "mask"], init="reset"),
    dict(name="k150_c3_t3_slide", C=3, K=150, T=3, iters=[3, 3], graph="random", umode=["mask", "unbiased", "unary"],
         init="initialize", slide=True),
    dict(name="slic150_c21_t2", C=21, K=150, T=2, iters=[10], graph="slic150", umode=["mask"], init="initialize"),
    dict(name="slic300_c3_t4", C=3, K=300, T=4, iters=[10], graph="slic300", umode=["unary"], init="initialize",
         compat=[1.0, 0.25, 2.0]),
    dict(name="chain_k100_c3_t4", C=3, K=CHAIN_K, T=4, iters=[10], graph="chain", umode=["mask"], init="initialize"),
]
CASE_NAMES = [c["name"] for c in CASES]
CASE_BY_NAME = {c["name"]: c for c in CASES}

# The edges of the sweep behind SimpleCRF.inference and superpixel_crf (tests/golden/crf_edge_cases.npz).  Its own: 127, 128 and 129
# classes around the cut at which the messages leave LDS (128: the largest LDS form, 16 wavefronts of 8 classes), 17 classes (two
# classes per wavefront, the last wavefront with one) on a last tile of 6 live lanes, one class, window sizes on the block edges of
# the sweep (64 nodes) and of the edge pass (256), the clamp of the class sum, neighbour rows of thousands of entries, and a window
# that grows, shrinks and slides between inferences.  And those of the kernels SimpleCRF ran before it, which cut at 256 classes:
# 255, 256, 257 and 300 classes.
# With the default params and make_inputs' random centres and colours every pairwise energy underflows against the unaries, so q
# would not depend on the q before it.  WIDE makes the messages count: a stale q or another summation order changes the result.
WIDE = [1.5, 2.0, 150.0, 120.0, 600.0, 0.5, 400.0]
# further graphs: "hub" ("random", but nodes 0 and K-1 list HUB_ENTRIES neighbours each, duplicates and self-loops among them)
HUB_ENTRIES = 3000
# "offsets": every node's unaries (uniform in [0, 4)) are raised by one of these, so that the class sum spans everything from O(1) to
# 0: below 1e-5 (clamped: the row no longer sums to 1), expf results that are denormal, rows of zeros.
CLAMP_OFFSETS = [0.0, 9.0, 12.5, 40.0, 95.0, 104.0, 110.0]
# "script": operations after the T initial frames are pushed and initialize()d (see replay); q of every live frame is recorded after
# each "infer".  This one: grow with q on the device (2 -> 3), a read, two pops in a row (-> 1), three pushes (-> 4), a reset of one
# frame, then a pop inside the capacity of 4 that shifts every frame.
WINDOW_SCRIPT = [("infer", 2), ("push", 2), ("infer", 2), ("read", 1), ("pop",), ("pop",), ("infer", 1), ("push", 3), ("push", 4),
                 ("push", 5), ("infer", 2), ("reset", 1), ("infer", 1), ("pop",), ("infer", 2)]


def _block_edge(name, K, T):
    return dict(name=name, C=2, K=K, T=T, iters=[2], graph="random", umode=["unary"], init="initialize", params=WIDE)


# "ugrid": the unaries (uniform in [0, 4)) are rounded down to multiples of 1 / ugrid.  They and q0 = expf(-unaries) then take 256
# values and compress to a third, which keeps the fixture file below 1 MiB.  A cell still differs from another one with probability
# 255 / 256, so a sweep that mixes up classes, lanes or frames shows; the energies keep full mantissas, so every message, every Potts
# sum and every q after the first sweep is rounded as with any other unaries.
UNARY_GRID = 64


def _class_edge(C, K, T):
    """The smallest shape at which one form of the sweep can go wrong; the compat values differ, so the order of the Potts sum shows."""
    return dict(name="c%d_k%d_t%d" % (C, K, T), C=C, K=K, T=T, iters=[2], graph="random", umode=["unary"], init="initialize",
                params=WIDE, compat=[0.25 + 0.125 * (c % 11) for c in range(C)], ugrid=UNARY_GRID)


EDGE_CASES = [
    dict(name="c257_k65_t2_long", C=257, K=65, T=2, iters=[3], graph="long", umode=["unary", "mask"], init="initialize",
         params=[0.375, 1.25, 150.0, 120.0, 600.0, 0.125, 400.0], compat=[0.25 + 0.125 * (c % 11) for c in range(257)]),
    dict(name="c256_k33_t1", C=256, K=33, T=1, iters=[2], graph="random", umode=["unary"], init="initialize", params=WIDE),
    dict(name="c255_k33_t1", C=255, K=33, T=1, iters=[2], graph="random", umode=["mask"], init="initialize", params=WIDE),
    dict(name="c300_k33_t3_slide", C=300, K=33, T=3, iters=[2, 2], graph="random", umode=["mask", "unbiased", "unary"],
         init="initialize", slide=True, params=WIDE),
    dict(name="c1_k70_t2", C=1, K=70, T=2, iters=[3], graph="random", umode=["unary", "proba", "unbiased"], init="initialize",
         params=WIDE),
    dict(name="clamp_c3_k130_t3", C=3, K=130, T=3, iters=[4], graph="random", umode=["unary"], init="initialize",
         offsets=CLAMP_OFFSETS),
    _block_edge("n63", 63, 1), _block_edge("n64", 64, 1), _block_edge("n65", 65, 1),
    _block_edge("n255", 85, 3), _block_edge("n256", 128, 2), _block_edge("n257", 257, 1),
    dict(name="hub_c5_k200_t2", C=5, K=200, T=2, iters=[3], graph="hub", umode=["unary", "mask"], init="initialize",
         params=[0.004, 0.05, 150.0, 120.0, 600.0, 0.002, 400.0]),
    dict(name="window_c3_k40", C=3, K=40, T=2, iters=[2], graph="random", umode=["unary", "mask", "proba"], init="initialize",
         params=WIDE, script=WINDOW_SCRIPT),
    _class_edge(127, 33, 1),                  # just below the cut
    _class_edge(128, 33, 2),                  # the largest LDS form (64 KB), with temporal links
    _class_edge(129, 33, 2),                  # the first plane form: messages in the workspace, exponentials in q_out
    _class_edge(17, 70, 3),                   # two classes per wavefront, the last wavefront with one; a tile of 6 live lanes
]
EDGE_CASE_NAMES = [c["name"] for c in EDGE_CASES]
EDGE_CASE_BY_NAME = {c["name"]: c for c in EDGE_CASES}


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(l) for l in lists])
    idx = np.array([v for l in lists for v in l], np.uint32)
    return off, idx


def make_inputs(case, rng, graph_npz=None, chain=None):
    """Deterministic inputs of a case: one dict per pushed frame (clusters, off, idx, umode, udata, conf)."""
    from fast_slic_amd._binding import CLUSTER_DTYPE
    C, K, T = case["C"], case["K"], case["T"]
    nframes = T + (1 if case.get("slide") else 0)
    for op in case.get("script") or []:
        if op[0] == "push":
            nframes = max(nframes, op[1] + 1)
    g = case["graph"]
    chain_frames = chain() if g == "chain" else None
    base = None
    if g in ("slic150", "slic300"):
        key = {"slic150": "slic_150x201_k150", "slic300": "slic_240x320_k300"}[g]
        base = np.ascontiguousarray(graph_npz[key + "/clusters"]).view(CLUSTER_DTYPE).reshape(-1)
        num, nb = graph_npz[key + "/conn_num"], graph_npz[key + "/conn_nb"]
        base_lists = [list(nb[i, :num[i]]) for i in range(K)]
    frames = []
    for j in range(nframes):
        if g == "chain":
            cl, num, nb = chain_frames[j]
            lists = [list(nb[i, :num[i]]) for i in range(K)]
        elif base is not None:
            cl = base.copy()
            if j:
                for ch in ("r", "g", "b"):            # the same superpixels with drifting colours
                    cl[ch] = cl[ch] + rng.integers(-6, 7, K).astype(np.float32)
            lists = base_lists
        else:
            cl = np.zeros(K, CLUSTER_DTYPE)
            cl["y"] = rng.integers(0, 720, K).astype(np.float32) + rng.integers(0, 4, K) * np.float32(0.25)
            cl["x"] = rng.integers(0, 1280, K).astype(np.float32) + rng.integers(0, 8, K) * np.float32(0.125)
            for ch in ("r", "g", "b"):
                cl[ch] = rng.integers(0, 256, K).astype(np.float32)
            cl["number"] = np.arange(K)
            cl["num_members"] = rng.integers(1, 900, K)
            if g == "long":
                cl["num_members"][rng.random(K) < 0.1] = 0
            if g == "none":
                lists = [[] for _ in range(K)]
            elif g == "small":
                lists = [[0, 1, 1], [1, 2, 0, 2], []] if K == 3 else [[i] for i in range(K)]
            elif g in ("random", "hub"):
                lists = [list(rng.choice(K, int(rng.integers(0, 13)), replace=False)) for _ in range(K)]
                if g == "hub":
                    for i in (0, K - 1):
                        l = list(rng.integers(0, K, HUB_ENTRIES))
                        l[1] = l[0]                   # a duplicate
                        l[-1] = i                     # a self-loop
                        lists[i] = l
            else:   # long
                lists = []
                for i in range(K):
                    n = int(rng.integers(0, 21)) if rng.random() > 0.1 else 0
                    l = list(rng.integers(0, K, n))
                    if n > 2:
                        l[1] = l[0]                   # a duplicate
                        l[-1] = i                     # a self-loop
                    lists.append(l)
        off, idx = _csr(lists)
        umode = case["umode"][j % len(case["umode"])]
        conf = 0.0
        if umode == "unary":
            udata = rng.uniform(0.0, 4.0, (C, K)).astype(np.float32)
            if case.get("ugrid"):
                udata = np.floor(udata * np.float32(case["ugrid"])) / np.float32(case["ugrid"])
            if case.get("offsets"):
                udata = udata + rng.choice(np.array(case["offsets"], np.float32), K)[None, :]
        elif umode == "proba":
            p = rng.uniform(0.01, 1.0, (C, K)).astype(np.float32)
            udata = (p / p.sum(0, keepdims=True)).astype(np.float32)
        elif umode == "mask":
            udata = rng.integers(0, C, K).astype(np.int32)
            conf = float(np.float32(rng.uniform(0.2, 0.9)))
        else:
            udata = np.zeros(0, np.float32)
        frames.append(dict(clusters=np.ascontiguousarray(cl), off=off, idx=idx, umode=umode, udata=udata, conf=conf))
    return frames


def _fill(crf, f, fr):
    crf.set_clusters(f, fr["clusters"])
    crf.set_connectivity(f, fr["off"], fr["idx"])
    crf.set_unary(f, fr["umode"], fr["udata"], fr["conf"])


def replay(crf, case, frames, host_only=False, only_step=None):
    """Run a case against `crf` (RefCRF of the maker or PkgCRF below); returns what the fixtures record.  host_only: stop before
    the first inference with max_iter > 0 (what needs no GPU; a case with a "script" stops before the script).  only_step: read q
    after that inference alone (the other entries of rec["steps"] are None) and stop there, so that q stays where the earlier
    inferences left it while the window moves; reading it, as recording every step does, brings it to the host."""
    C, K, T = case["C"], case["K"], case["T"]
    if case.get("params"):
        crf.set_params(case["params"])
    for cls, v in enumerate(case.get("compat") or []):
        crf.set_compat(cls, v)
    handles = []
    for j in range(T):
        f = crf.push()
        _fill(crf, f, frames[j])
        handles.append(f)
    rec = {"unaries": [crf.unaries(f) for f in handles]}
    f0 = handles[0]
    fr0 = frames[0]
    rec["spatial"] = np.array([crf.spatial(f0, int(fr0["idx"][k]), i) for i in range(K)
                               for k in range(fr0["off"][i], fr0["off"][i + 1])], np.float32)
    if T > 1:
        rec["temporal"] = np.array([[crf.temporal(handles[0], handles[1], i) for i in range(K)],
                                    [crf.temporal(handles[1], handles[0], i) for i in range(K)]], np.float32)
    if case["init"] == "initialize":
        crf.initialize()
    else:
        for f in handles[::2]:
            crf.reset_inferred(f)
    rec["q0"] = [crf.inferred(f) for f in handles]
    if host_only and case["iters"][0] > 0:
        return rec
    rec["steps"] = []
    if case.get("script"):
        _run_script(crf, case["script"], frames, handles, rec, only_step)
        return rec
    crf.inference(case["iters"][0])
    if _record(crf, handles, rec, only_step):
        return rec
    if case.get("slide"):
        crf.pop()
        handles.pop(0)
        f = crf.push()
        _fill(crf, f, frames[T])
        rec["unaries"].append(crf.unaries(f))
        handles.append(f)
        crf.inference(case["iters"][1])
        _record(crf, handles, rec, only_step)
    return rec


def _record(crf, handles, rec, only_step):
    """One step of rec["steps"]: q of every live frame, or None for a step that only_step leaves out.  -> only_step is reached."""
    s = len(rec["steps"])
    rec["steps"].append([crf.inferred(f) for f in handles] if only_step in (None, s) else None)
    return only_step == s


def _run_script(crf, script, frames, handles, rec, only_step=None):
    """The operations of a case's "script" on the live frames `handles` (oldest first): ("infer", n), ("push", j) (frame j of the
    inputs; the pushes name j = T, T + 1, ... in order, so rec["unaries"] stays indexed by input frame), ("pop",), ("reset", i)
    (reset_inferred of the i-th live frame), ("read", i) (get_inferred of it, discarded).  Every "infer" records one step."""
    for op in script:
        if op[0] == "infer":
            crf.inference(op[1])
            if _record(crf, handles, rec, only_step):
                return
        elif op[0] == "push":
            assert op[1] == len(rec["unaries"]), "pushes take the input frames in order"
            f = crf.push()
            _fill(crf, f, frames[op[1]])
            rec["unaries"].append(crf.unaries(f))
            handles.append(f)
        elif op[0] == "pop":
            crf.pop()
            handles.pop(0)
        elif op[0] == "reset":
            crf.reset_inferred(handles[op[1]])
        elif op[0] == "read":
            crf.inferred(handles[op[1]])
        else:
            raise ValueError("unknown script operation %r" % (op,))


def pack(case, frames, rec):
    out = {"meta": np.array(json.dumps({k: v for k, v in case.items()}))}
    for j, fr in enumerate(frames):
        out["f%d/clusters" % j] = fr["clusters"].view(np.uint8).reshape(-1, 32)
        out["f%d/off" % j] = fr["off"]
        out["f%d/idx" % j] = fr["idx"]
        out["f%d/udata" % j] = fr["udata"]
        out["f%d/conf" % j] = np.float32(fr["conf"])
        if fr["umode"] != "unary":
            out["f%d/unaries" % j] = rec["unaries"][j]
    out["spatial"] = rec["spatial"]
    if "temporal" in rec:
        out["temporal"] = rec["temporal"]
    for j, q in enumerate(rec["q0"]):
        out["q0/%d" % j] = q
    for s, qs in enumerate(rec["steps"]):
        for j, q in enumerate(qs):
            out["step%d/%d" % (s, j)] = q
    return out


def unpack_frames(npz, name):
    """The inputs of a case as make_inputs produced them (from the fixture; no reference needed)."""
    from fast_slic_amd._binding import CLUSTER_DTYPE
    case = json.loads(str(npz[name + "/meta"]))
    frames = []
    j = 0
    while (name + "/f%d/off" % j) in npz.files:
        frames.append(dict(clusters=np.ascontiguousarray(npz[name + "/f%d/clusters" % j]).view(CLUSTER_DTYPE).reshape(-1),
                           off=npz[name + "/f%d/off" % j], idx=npz[name + "/f%d/idx" % j],
                           umode=case["umode"][j % len(case["umode"])], udata=npz[name + "/f%d/udata" % j],
                           conf=float(npz[name + "/f%d/conf" % j])))
        j += 1
    return case, frames


class PkgCRF(object):
    """fast_slic_amd.crf.SimpleCRF with the interface replay() drives."""

    def __init__(self, C, K, device=0):
        from fast_slic_amd.crf import SimpleCRF
        self.crf = SimpleCRF(C, K, device=device)
        self.C, self.K = C, K

    def set_params(self, values):
        for n, v in zip(PARAM_NAMES, values):
            setattr(self.crf, n, v)

    def set_compat(self, cls, v):
        self.crf.set_compat(cls, v)

    def push(self):
        return self.crf.push_frame()

    def pop(self):
        return self.crf.pop_frame()

    def set_clusters(self, f, cl):
        f.set_clusters(cl)

    def set_connectivity(self, f, off, idx):
        f.set_connectivity([list(idx[off[i]:off[i + 1]]) for i in range(self.K)])

    def set_unary(self, f, mode, data, conf):
        if mode == "unary":
            f.unaries = np.asarray(data, np.float32)
        elif mode == "proba":
            f.set_proba(np.asarray(data, np.float32))
        elif mode == "mask":
            f.set_mask(np.asarray(data, np.int32), conf)
        else:
            f.set_unbiased()

    def unaries(self, f):
        return f.unaries

    def inferred(self, f):
        return f.get_inferred()

    def spatial(self, f, i, j):
        return np.float32(f.spatial_pairwise_energy(i, j))

    def temporal(self, f, other, i):
        return np.float32(f.temporal_pairwise_energy(i, other))

    def reset_inferred(self, f):
        f.reset_inferred()

    def initialize(self):
        self.crf.initialize()

    def inference(self, n):
        self.crf.inference(n)
