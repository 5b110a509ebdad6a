"""SimpleCRF inference on torch tensors on the MI355X (fast_slic_amd/crf_torch.py, csrc/crf_tensor.hip), bit for bit: against the
reference's recorded results (tests/golden/crf_cases.npz, and the edges of the sweep in crf_edge_cases.npz), against the package's
SimpleCRF (pinned to the same fixtures; it runs the same edge pass and sweep, so these compare the two uploads) at the seams of the
sweep's layout (64 nodes a block, one wavefront per class slice, the LDS cut at 128 classes), with neighbour entries out
of range, batch independence, streams, no host synchronisation, SuperpixelGraph.to_batch_csr, and the all-GPU chain
Slic -> pool -> graph -> CRF -> unpool.  Every comparison is np.array_equal on the float bits; there are no tolerances."""
import os

import numpy as np
import pytest
import torch

import crf_cases as CC
from fast_slic_amd import _binding as B
from fast_slic_amd.crf import SimpleCRF
from fast_slic_amd.crf_torch import superpixel_crf
from fast_slic_amd.pool import superpixel_pool, superpixel_unpool
from fast_slic_amd.rag import superpixel_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD = np.load(os.path.join(GOLDEN, "crf_cases.npz"))
EDGE_GOLD = np.load(os.path.join(GOLDEN, "crf_edge_cases.npz"))
# the edge cases that are one window and one inference: what a single superpixel_crf call can replay
EDGE_NAMES = [c["name"] for c in CC.EDGE_CASES if not c.get("script") and not c.get("slide")]
LDS_CUT = 128                     # kCrfTensorLdsClasses (csrc/crf_tensor.h)


def bits_equal(got, exp, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    exp = exp.cpu().numpy() if isinstance(exp, torch.Tensor) else np.asarray(exp)
    assert got.dtype == np.float32 and exp.dtype == np.float32 and got.shape == exp.shape, what
    bad = np.count_nonzero(got.view(np.uint32) != exp.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), "%s: differs at %d of %d entries" % (what, bad, got.size)


def cluster_tensors(clusters):
    """CLUSTER_DTYPE[N][K] -> yxrgb float32 [N, 5, K], members int32 [N, K] on the GPU."""
    yx = np.stack([np.stack([cl[n] for n in ("y", "x", "r", "g", "b")]) for cl in clusters]).astype(np.float32)
    mem = np.stack([cl["num_members"].view(np.int32) for cl in clusters])
    return torch.from_numpy(yx).to(DEV), torch.from_numpy(np.ascontiguousarray(mem)).to(DEV)


def csr_tensors(rows):
    """rows[N][K] lists -> one CSR over (frame, node) on the GPU."""
    flat = [r for frame in rows for r in frame]
    off = np.zeros(len(flat) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in flat])
    idx = np.array([v for r in flat for v in r], np.int64).astype(np.int32)
    return torch.from_numpy(off).to(DEV), torch.from_numpy(idx).to(DEV)


def on_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the reference's fixtures ----
def fixture(name):
    gold = GOLD if name in CC.CASE_BY_NAME else EDGE_GOLD
    case, frames = CC.unpack_frames(gold, name)
    T = case["T"]
    frames = frames[:T]
    unaries = [gold["%s/f%d/unaries" % (name, j)] if frames[j]["umode"] != "unary" else frames[j]["udata"] for j in range(T)]
    rows = [[list(map(int, f["idx"][f["off"][i]:f["off"][i + 1]])) for i in range(case["K"])] for f in frames]
    yx, mem = cluster_tensors([f["clusters"] for f in frames])
    params = dict(zip(CC.PARAM_NAMES, case["params"])) if case.get("params") else None
    q0 = np.stack([gold["%s/q0/%d" % (name, j)] for j in range(T)])
    step = np.stack([gold["%s/step0/%d" % (name, j)] for j in range(T)])
    return case, on_gpu(np.stack(unaries).astype(np.float32)), csr_tensors(rows), yx, mem, params, case.get("compat"), q0, step


@pytest.mark.parametrize("name", CC.CASE_NAMES + EDGE_NAMES)
def test_matches_the_reference_fixture(name):
    case, un, graph, yx, mem, params, compat, q0, step = fixture(name)
    q = superpixel_crf(un, graph, yx, mem, max_iter=case["iters"][0], params=params, compat=compat, temporal=True, q0=on_gpu(q0))
    assert q.shape == un.shape and q.dtype == torch.float32 and q.device == DEV
    bits_equal(q, step, name)


@pytest.mark.parametrize("name", [c["name"] for c in CC.CASES if c["init"] == "initialize"])
def test_q0_none_is_initialize(name):
    case, un, graph, yx, mem, params, compat, q0, _ = fixture(name)
    bits_equal(superpixel_crf(un, graph, yx, mem, max_iter=0, params=params, compat=compat, temporal=True), q0, name)


# ---- against the package's SimpleCRF ----
def random_case(seed, N, Cn, K, max_degree=12, hub=0):
    """Clusters, neighbour lists (duplicates, self-loops, empty rows; node 0 of every frame with `hub` entries) and unaries."""
    rng = np.random.default_rng(seed)
    clusters, rows = [], []
    for _ in range(N):
        cl = np.zeros(K, B.CLUSTER_DTYPE)
        cl["y"] = rng.integers(0, 720, K).astype(np.float32) + rng.integers(0, 4, K) * np.float32(0.25)
        cl["x"] = rng.integers(0, 1280, K).astype(np.float32) + rng.integers(0, 8, K) * np.float32(0.125)
        for ch in ("r", "g", "b"):
            cl[ch] = rng.integers(0, 256, K).astype(np.float32)
        cl["number"] = np.arange(K)
        cl["num_members"] = rng.integers(1, 900, K)
        cl["num_members"][rng.random(K) < 0.1] = 0
        clusters.append(cl)
        frame = []
        for i in range(K):
            r = [int(v) for v in rng.integers(0, K, int(rng.integers(0, max_degree + 1)))] if rng.random() > 0.1 else []
            if len(r) > 2:
                r[1] = r[0]
                r[-1] = i
            frame.append(r)
        if hub:
            frame[0] = [int(v) for v in rng.integers(0, K, hub)]
        rows.append(frame)
    unaries = rng.uniform(0.0, 4.0, (N, Cn, K)).astype(np.float32)
    return clusters, rows, unaries


def simple_crf(clusters, rows, unaries, iters, params=None, compat=None):
    """The frames as one window of the package's SimpleCRF: initialize(), inference(iters) -> q [T, C, K]."""
    T, Cn, K = unaries.shape
    crf = SimpleCRF(Cn, K)
    for n, v in (params or {}).items():
        setattr(crf, n, v)
    for cls, v in enumerate(compat or []):
        crf.set_compat(cls, v)
    frames = []
    for j in range(T):
        f = crf.push_frame()
        f.set_clusters(clusters[j])
        f.set_connectivity(rows[j])
        f.unaries = unaries[j]
        frames.append(f)
    crf.initialize()
    crf.inference(iters)
    return np.stack([f.get_inferred() for f in frames])


def tensor_crf(clusters, rows, unaries, iters, **kw):
    yx, mem = cluster_tensors(clusters)
    return superpixel_crf(on_gpu(unaries), csr_tensors(rows), yx, mem, max_iter=iters, **kw)


@pytest.mark.parametrize("N,Cn,K,hub", [
    (2, 3, 63, 0), (2, 3, 64, 0), (2, 3, 65, 0), (2, 21, 129, 0),          # the wavefront and block seams; 21 classes: 11 waves of 2
    (2, 1, 70, 0),                                                          # one class: the compatibility sum is empty
    (3, 17, 70, 0),                                                         # two class slices, the last wave idle in the second
    (1, LDS_CUT, 70, 0), (2, LDS_CUT + 1, 70, 0),                           # the last shape with messages in LDS, the first without
    (2, 3, 70, 300),                                                        # one hub row of 300 entries
])
def test_temporal_window_equals_simple_crf(N, Cn, K, hub):
    clusters, rows, unaries = random_case(N * 1000 + Cn * 10 + K, N, Cn, K, hub=hub)
    params = dict(spatial_w=3.5, temporal_w=7.25, spatial_smooth_w=2.5, spatial_sxy=200.0)
    compat = [0.5 + 0.25 * (c % 5) for c in range(Cn)]
    for iters in (1, 4):                                                    # both parities of the ping-pong
        got = tensor_crf(clusters, rows, unaries, iters, params=params, compat=compat, temporal=True)
        bits_equal(got, simple_crf(clusters, rows, unaries, iters, params, compat), "N=%d C=%d K=%d, %d sweeps" % (N, Cn, K, iters))


def test_independent_frames_equal_separate_simple_crfs():
    clusters, rows, unaries = random_case(11, 3, 5, 150)
    got = tensor_crf(clusters, rows, unaries, 5, temporal=False)
    exp = np.concatenate([simple_crf(clusters[n:n + 1], rows[n:n + 1], unaries[n:n + 1], 5) for n in range(3)])
    bits_equal(got, exp, "three independent frames")
    window = tensor_crf(clusters, rows, unaries, 5, temporal=True)
    assert not torch.equal(window, got)                                     # the temporal links do change the result
    # a single [C, K] frame is the batch of one
    yx, mem = cluster_tensors(clusters[:1])
    one = superpixel_crf(on_gpu(unaries[0]), csr_tensors(rows[:1]), yx[0], mem[0], max_iter=5)
    assert one.shape == (5, 150)
    bits_equal(one, exp[0], "unbatched")


def test_no_neighbours_at_all():
    clusters, rows, unaries = random_case(12, 2, 3, 70)
    rows = [[[] for _ in range(70)] for _ in range(2)]
    off, idx = csr_tensors(rows)
    assert idx.shape == (0,) and idx.dtype == torch.int32
    for temporal in (False, True):
        got = tensor_crf(clusters, rows, unaries, 3, temporal=temporal)
        exp = simple_crf(clusters, rows, unaries, 3) if temporal else \
            np.concatenate([simple_crf(clusters[n:n + 1], rows[n:n + 1], unaries[n:n + 1], 3) for n in range(2)])
        bits_equal(got, exp, "nnz = 0, temporal=%s" % temporal)


def test_non_contiguous_inputs_and_compat_tensor():
    clusters, rows, unaries = random_case(13, 2, 4, 70)
    yx, mem = cluster_tensors(clusters)
    compat = [1.0, 0.25, 2.0, 0.5]
    exp = simple_crf(clusters, rows, unaries, 2, compat=compat)
    un_t = on_gpu(unaries.transpose(0, 2, 1).copy()).transpose(1, 2)        # [N, C, K] view of [N, K, C] storage
    yx_t = yx.transpose(1, 2).contiguous().transpose(1, 2)
    assert not un_t.is_contiguous() and not yx_t.is_contiguous()
    wide = torch.zeros(8, device=DEV)
    wide[::2] = torch.tensor(compat, device=DEV)
    got = superpixel_crf(un_t, csr_tensors(rows), yx_t, mem, max_iter=2, compat=wide[::2], temporal=True)
    bits_equal(got, exp, "non-contiguous inputs")


# ---- neighbour entries out of range ----
def test_out_of_range_entries_contribute_nothing():
    K = 70
    clusters, rows, unaries = random_case(14, 2, 3, K)
    rng = np.random.default_rng(15)
    dirty = []
    for frame in rows:
        out = []
        for r in frame:
            r = list(r)
            for bad in (-1, K, (1 << 31) - 1):
                if rng.random() < 0.4:
                    r.insert(int(rng.integers(0, len(r) + 1)), bad)
            out.append(r)
        dirty.append(out)
    dirty[0][3] = [-1, K, (1 << 31) - 1]                                    # a row of nothing else
    rows[0][3] = []
    dirty[1][0] = [(1 << 31) - 1] + rows[1][0] + [-1]                       # at the ends of the first row of the second frame
    assert sum(len(r) for f in dirty for r in f) > sum(len(r) for f in rows for r in f) + 50
    for temporal in (False, True):
        bits_equal(tensor_crf(clusters, dirty, unaries, 3, temporal=temporal), tensor_crf(clusters, rows, unaries, 3, temporal=temporal),
                   "out-of-range entries, temporal=%s" % temporal)


# ---- batch independence, determinism ----
def test_batch_position_and_repeated_calls():
    clusters, rows, unaries = random_case(16, 4, 21, 129)
    alone = tensor_crf(clusters[:1], rows[:1], unaries[:1], 3)
    assert torch.equal(alone, tensor_crf(clusters[:1], rows[:1], unaries[:1], 3))
    for pos in range(4):
        order = [1, 2, 3]
        order.insert(pos, 0)
        batch = tensor_crf([clusters[n] for n in order], [rows[n] for n in order], unaries[order], 3, temporal=False)
        assert torch.equal(batch[pos], alone[0]), "position %d of 4" % pos
        assert torch.equal(batch, tensor_crf([clusters[n] for n in order], [rows[n] for n in order], unaries[order], 3, temporal=False))


# ---- streams, inputs untouched, no synchronisation ----
def test_non_default_stream_and_inputs_unchanged():
    clusters, rows, unaries = random_case(17, 2, 5, 129)
    yx, mem = cluster_tensors(clusters)
    graph = csr_tensors(rows)
    un = on_gpu(unaries)
    q0 = torch.softmax(-un, dim=1).contiguous()
    un_before, q0_before = un.clone(), q0.clone()
    exp = superpixel_crf(un, graph, yx, mem, max_iter=3, temporal=True, q0=q0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got = superpixel_crf(un, graph, yx, mem, max_iter=3, temporal=True, q0=q0)
    side.synchronize()
    assert torch.equal(got, exp)
    assert torch.equal(un, un_before) and torch.equal(q0, q0_before)
    assert not torch.equal(exp, superpixel_crf(un, graph, yx, mem, max_iter=3, temporal=True))      # q0 was used


_slic_cache = {}


def slic_batch(H, W, K, variants):
    """Label maps [N, H, W] (torch int16 on the GPU) and frames [N, H, W, 3] of Slic on synthetic frames."""
    key = (H, W, K, variants)
    if key not in _slic_cache:
        from fast_slic_amd import Slic
        from fast_slic_amd.synth import variant
        frames = [variant(v, H, W, seed=1) for v in variants]
        labels = [Slic(num_components=K).iterate(f) for f in frames]
        _slic_cache[key] = (torch.from_numpy(np.stack(labels)).to(DEV), np.stack(frames))
    return _slic_cache[key]


def pooled_inputs(lab, frames, K, Cn, seed):
    """What the chain pools on the GPU: unaries from class probabilities, yxrgb from coordinate and image means, members = counts."""
    N, H, W = lab.shape
    rng = np.random.default_rng(seed)
    proba = torch.softmax(on_gpu(rng.normal(0, 2, (N, Cn, H, W)).astype(np.float32)), dim=1)
    p, counts = superpixel_pool(proba, lab, K, return_counts=True)
    img = torch.from_numpy(frames).to(DEV).permute(0, 3, 1, 2).to(torch.float32)
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
    coords = torch.stack([yy, xx]).expand(N, 2, H, W)
    yxrgb = superpixel_pool(torch.cat([coords, img], dim=1), lab, K)
    return -torch.log(p.clamp_min(1e-6)), yxrgb, counts


def test_no_host_synchronisation():
    K = 40
    lab, frames = slic_batch(120, 160, K, ("A", "B"))
    graph = superpixel_graph(lab, K)                                        # (synchronises: the number of edges shapes its result)
    un, yxrgb, counts = pooled_inputs(lab, frames, K, 3, 18)
    exp = superpixel_crf(un, graph, yxrgb, counts, max_iter=3, compat=[1.0, 0.5, 2.0], params=dict(spatial_w=5.0))
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            got = superpixel_crf(un, graph, yxrgb, counts, max_iter=3, compat=[1.0, 0.5, 2.0], params=dict(spatial_w=5.0))
            plain = superpixel_crf(un, graph, yxrgb, counts, temporal=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error')")
    assert torch.equal(got, exp) and plain.shape == un.shape


# ---- SuperpixelGraph.to_batch_csr ----
def assert_batch_csr(g):
    off, idx = g.to_batch_csr()
    K, N = g.num_components, g.num_frames
    assert off.dtype == torch.int64 and idx.dtype == torch.int32 and off.shape == (N * K + 1,) and off.device == DEV and idx.device == DEV
    offs, idxs, shift = [torch.zeros(1, dtype=torch.int64, device=DEV)], [], 0
    for n in range(N):
        o, i = g.to_csr(n)
        offs.append(o[1:] + shift)
        idxs.append(i)
        shift += int(o[-1])
    assert torch.equal(off, torch.cat(offs)) and torch.equal(idx, torch.cat(idxs))
    assert idx.shape == (2 * g.edge_index.shape[1],)


def test_to_batch_csr_equals_the_frames_csr():
    K = 40
    lab, _ = slic_batch(120, 160, K, ("A", "B", "C"))
    assert_batch_csr(superpixel_graph(lab, K, connectivity=8))
    holed = lab.clone()
    holed[1] = -1                                                           # an empty frame in the middle
    g = superpixel_graph(holed, K)
    assert int(g.offsets[1]) == int(g.offsets[2]) > 0
    assert_batch_csr(g)


# ---- the chain ----
def test_all_gpu_chain_equals_simple_crf():
    H, W, K, Cn, iters = 240, 320, 150, 3, 5
    lab, frames = slic_batch(H, W, K, ("A",))
    lab, frame = lab[0], frames[:1]
    un, yxrgb, counts = pooled_inputs(lab[None], frame, K, Cn, 19)
    un, yxrgb, counts = un[0], yxrgb[0], counts[0]
    graph = superpixel_graph(lab, K)
    q = superpixel_crf(un, graph, yxrgb, counts, max_iter=iters)
    seg = superpixel_unpool(q, lab).argmax(0)
    assert q.shape == (Cn, K) and seg.shape == (H, W)
    # the same tensors through SimpleCRF
    cl = np.zeros(K, B.CLUSTER_DTYPE)
    for j, n in enumerate(("y", "x", "r", "g", "b")):
        cl[n] = yxrgb[j].cpu().numpy()
    cl["num_members"] = counts.cpu().numpy().view(np.uint32)
    off, idx = (t.tolist() for t in graph.to_csr())
    exp = simple_crf([cl], [[idx[off[k]:off[k + 1]] for k in range(K)]], un.cpu().numpy()[None], iters)[0]
    bits_equal(q, exp, "chain")
    assert torch.equal(seg, superpixel_unpool(on_gpu(exp), lab).argmax(0))
    assert len(torch.unique(seg)) > 1
