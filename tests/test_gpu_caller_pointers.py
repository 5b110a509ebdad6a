"""Every entry point that works on the caller's device memory in place, at the addresses a PyTorch-ROCm caller really passes (-m gpu).

Everywhere else in the suite a buffer is a tensor of its own, which the allocator aligns to 512 bytes.  A caller holds one stacked
[n, H, W, 3] uint8 tensor and one [n, H, W] int16 tensor and passes t[i].data_ptr(): with an odd H * W frame i of the RGB stack lies at
byte residue 3 i H W mod 4 (0, 3, 2, 1 over four frames) and frame i of the label stack at 2 i H W mod 8 (0, 2, 4, 6); a view at a
storage offset gives the torch-tensor operations the same kind of pointer.  Here every buffer is carved out of one flat allocation
filled with a guard byte, its residue is asserted through data_ptr(), and after every call every byte outside the outputs -- the guard
before, between and behind the frames, and the input frames themselves -- must be what it was.

The kernels that dereference such a pointer, and what each does about its alignment (found by reading csrc/ for FrameDev::rgb,
CcaDev::out and every pointer include/fslic_hip.h calls "host or device" or takes from a torch tensor):
  k_rgb_to_lab<CONVERT> (lab.hip)     reads FrameDev::rgb: three dwords per four pixels when the frame is 4-byte aligned, otherwise the
                                      whole frame byte by byte (`aligned4`, per frame: the frames of one launch may differ)
  k_cca_relabel (cca.hip)             writes CcaDev::out: 8-byte stores when W % 4 == 0 and the frame's map is 8-byte aligned
                                      (`aligned8`, added with this module: the pointer was not looked at), otherwise 2-byte stores
  no other kernel of the engine touches the caller's frames: the assign, cluster, LSC, float-distance, preemptive and the other
  connectivity kernels work on the engine's own planes (256-byte aligned by the arena's carve)
  k_mask_sums, k_density_to_mask, k_adjacent_pairs (graph.hip)   one element per access
  k_pool_tiles (pool.hip)             one element per access
  k_unpool (pool.hip)                 16-byte stores when H * W % 4 == 0 and `out` is 16-byte aligned (the launch decides), else 4-byte
  k_rag_* (rag.hip)                   a pixel of a C = 4 image as one dword when the image is 4-byte aligned (`word`), else bytes
  compare.hip, crf_tensor*.hip        one element per access (their vector types are parts of the call's own 16-byte-aligned workspace)
A d_labels at an odd address cannot hold uint16_t and is refused before any device work (fill_job, group.cpp): tested here and not in
tests/test_capi_cpu.py, because every entry point that takes d_labels takes an engine, and there is no engine without a GPU.

What would fail: with `aligned8` taken out of k_cca_relabel, the 40 x 68 frames whose maps lie at residues 2, 4 and 6 (mod 8) send
misaligned 8-byte stores (three of four single calls, six of the eight frames of the mixed group); with `aligned4` a constant 1 in
k_rgb_to_lab, every frame at residue 1, 2 or 3 (mod 4) loads misaligned dwords -- both CONVERT forms, single calls and frames inside a
mixed group are among the cases (test_layouts_cover_every_residue restates that arithmetic without a GPU).

Expected values: integer SLIC against the plain-C oracle, bit for bit; the float-distance variant and LSC against the same call on
tensors of their own (the aligned runs the other suites pin to the reference), byte for byte; the graph utilities against the committed
fixture; the torch operations against tests/pool_ref.py, tests/rag_ref.py, tests/compare_ref.py, and superpixel_crf against the same
call on fresh clones.  For the torch operations the pointers that reach the library are recorded (Spy) and must be the views' own: a
.contiguous() or .to(device) that copied would make the module test nothing."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import compare_ref
import pool_ref
import rag_ref
from oracle import oracle as orc
from fast_slic_amd import _binding as B
from fast_slic_amd import Engine, make_params
from fast_slic_amd.synth import variant
from util import describe_mismatch, cluster_fields_equal

pytestmark = pytest.mark.gpu

GUARD = 0xC3
MARGIN = 256              # guard bytes before the first and behind the last buffer of a region; a multiple of 16, so residues are the offsets'
BASE_ALIGN = 512          # what the allocator gives a tensor of its own (asserted on every carve)
_TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32,
          np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32}


# ---- buffers carved out of one guarded allocation ----------------------------------------------------------------------------------
class Carve(object):
    """One flat uint8 device allocation filled with GUARD.  put() places an input at a byte offset, hole() reserves an output there;
    both return a contiguous view whose data_ptr() is base + offset.  check() (after the call): every byte outside the holes is what it
    was -- guard bytes and inputs alike."""

    def __init__(self, nbytes):
        self.buf = torch.full((int(nbytes),), GUARD, dtype=torch.uint8, device="cuda")
        self.base = self.buf.data_ptr()
        assert self.base % BASE_ALIGN == 0, "the allocator's alignment is what the residues are counted from"
        self.host = np.full(int(nbytes), GUARD, np.uint8)
        self.used = np.zeros(int(nbytes), bool)
        self.holes = np.zeros(int(nbytes), bool)

    def _take(self, off, nbytes, dtype, shape):
        assert MARGIN <= off and off + nbytes + MARGIN <= self.host.size, "a buffer needs guard bytes on both sides"
        assert not self.used[off:off + nbytes].any(), "buffers overlap"
        self.used[off:off + nbytes] = True
        t = self.buf[off:off + nbytes].view(_TORCH[np.dtype(dtype)]).view(tuple(shape))
        assert t.is_contiguous() and t.data_ptr() == self.base + off and t.storage_offset() * t.element_size() == off
        return t

    def put(self, off, array):
        a = np.ascontiguousarray(array)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        raw = a.view(np.uint8).reshape(-1)
        t = self._take(off, raw.size, a.dtype, a.shape)
        self.host[off:off + raw.size] = raw
        self.buf[off:off + raw.size] = torch.from_numpy(raw.copy()).cuda()
        return t

    def hole(self, off, shape, dtype):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        t = self._take(off, nbytes, dtype, shape)
        self.holes[off:off + nbytes] = True
        return t

    def check(self, what):
        torch.cuda.synchronize()
        now = self.buf.cpu().numpy()
        bad = np.nonzero((now != self.host) & ~self.holes)[0]
        assert bad.size == 0, "%s: %d bytes outside the outputs changed, the first at offset %d (%s, 0x%02x -> 0x%02x)" % (
            what, bad.size, bad[0], "an input" if self.used[bad[0]] else "guard", self.host[bad[0]], now[bad[0]])


def engine_layout(H, W, n):
    """Byte offsets of n RGB frames and n label maps in one allocation, and its size: shape arithmetic only.
    RGB pitch: 3 H W, plus one byte when that is even -- an odd pitch takes four consecutive frames through every residue mod 4 (odd
    H * W: the frames of a stacked tensor, no byte between them).  Label pitch: 2 H W, plus two bytes when that is a multiple of 4 --
    a pitch of 2 mod 4 takes four consecutive maps through 0, 2, 4, 6 mod 8 (H * W odd: again the plain stack)."""
    HW = H * W
    rgb_pitch = 3 * HW + (1 if 3 * HW % 2 == 0 else 0)
    lab_pitch = 2 * HW + (2 if 2 * HW % 4 == 0 else 0)
    rgb = [MARGIN + i * rgb_pitch for i in range(n)]
    lab0 = -(-(rgb[-1] + 3 * HW + MARGIN) // BASE_ALIGN) * BASE_ALIGN + MARGIN
    lab = [lab0 + i * lab_pitch for i in range(n)]
    return rgb, lab, lab[-1] + 2 * HW + MARGIN


# (name, H, W, K, last_path).  37 x 53: 3 H W = 3 mod 4 and 2 H W = 2 mod 8, so the plain stacks walk through every residue; W % 4 = 1
# (relabel's scalar form whatever the address); 1961 pixels = 490 quads and a tail of one in the LAB kernel where the frame is aligned,
# all tail where it is not; 1 x 2 connectivity tiles of 64 x 32.  40 x 68: W % 4 == 0 (relabel's 8-byte form where the map's address
# allows it), 2 x 2 connectivity tiles, 680 quads and no tail.  K so that S >= 8 (the tiled assign kernels, last_path 0), and the
# 37 x 53 frame again at K = 60 (S = 5: the generic kernel, last_path 1).
SHAPES = [("odd_37x53_k12", 37, 53, 12, 0), ("w4_40x68_k16", 40, 68, 16, 0), ("generic_37x53_k60", 37, 53, 60, 1)]
OPTIONS = [(True, 0.25), (True, 0.0), (False, 0.25), (False, 0.0)]      # (convert_to_lab, min_size_factor)
GROUP = 8                                                              # frames of the mixed group: every residue twice


def test_layouts_cover_every_residue():
    """(No GPU work.)  The residues the cases claim, from the shape arithmetic alone."""
    for _, H, W, K, path in SHAPES:
        rgb, lab, total = engine_layout(H, W, GROUP)
        assert [o % 4 for o in rgb[:4]] == ([0, 3, 2, 1] if H * W % 2 else [0, 1, 2, 3]) and {o % 4 for o in rgb[4:]} == {0, 1, 2, 3}
        assert [o % 8 for o in lab[:4]] == [0, 2, 4, 6] and [o % 8 for o in lab[4:]] == [0, 2, 4, 6]
        assert all(b - a >= 3 * H * W for a, b in zip(rgb, rgb[1:])) and all(b - a >= 2 * H * W for a, b in zip(lab, lab[1:]))
        assert rgb[0] == MARGIN and rgb[-1] + 3 * H * W + MARGIN <= lab[0] - MARGIN and lab[-1] + 2 * H * W + MARGIN == total
        S = int(np.sqrt(H * W // K))
        assert (S >= 8) == (path == 0)
        assert (W + 63) // 64 * ((H + 31) // 32) >= 2               # more than one connectivity tile (40 x 68: 2 x 2)
    assert 37 * 53 % 4 == 1 and 37 * 53 // 4 >= 1                       # at least one full quad and a tail where the frame is aligned
    assert 3 * 37 * 53 % 4 == 3 and 2 * 37 * 53 % 8 == 2 and 53 % 4 == 1
    assert 68 % 4 == 0 and (2 * 40 * 68 + 2) % 8 == 2 and (68 + 63) // 64 == 2 and (40 + 31) // 32 == 2
    # which frames would take a misaligned wide access without the two alignment conditions
    _, lab, _ = engine_layout(40, 68, GROUP)
    assert [i for i, o in enumerate(lab) if o % 8] == [1, 2, 3, 5, 6, 7]
    for _, H, W, _, _ in SHAPES:
        assert sum(1 for o in engine_layout(H, W, GROUP)[0] if o % 4) == 6


@functools.lru_cache(maxsize=None)
def frame(H, W, i):
    f = np.ascontiguousarray(variant("ABCD"[i % 4], H, W, seed=i))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def oracle_result(H, W, K, convert, msf, i):
    f = frame(H, W, i)
    labels, cl = orc.slic_iterate(f, orc.initialize_clusters(f, K), min_size_factor=msf, convert_to_lab=convert)
    labels.setflags(write=False)
    return labels, cl.tobytes()


def carve_frames(H, W, positions, n=GROUP):
    """A fresh allocation with the frames of `positions` of the n-frame layout in place (frame i of the layout shows frame(H, W, i)):
    -> carve, {i: (rgb view, label view)}; residues asserted through data_ptr()."""
    rgb, lab, total = engine_layout(H, W, n)
    c = Carve(total)
    views = {}
    for i in positions:
        r, l = c.put(rgb[i], frame(H, W, i)), c.hole(lab[i], (H, W), np.int16)
        assert r.data_ptr() % 4 == rgb[i] % 4 and l.data_ptr() % 8 == lab[i] % 8 and l.data_ptr() % 2 == 0
        views[i] = (r, l)
    return c, views


def fresh_clusters(H, W, K, positions):
    return [orc.initialize_clusters(frame(H, W, i), K) for i in positions]


def assert_frames(what, c, views, cls, want):
    """want(i) -> (uint16 labels, Cluster bytes).  The guard check first: a stray store is the more telling failure."""
    c.check(what)
    for (i, (_, l)), cl in zip(sorted(views.items()), cls):
        labels, clbytes = want(i)
        got = l.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, labels), describe_mismatch("%s frame %d (rgb residue %d, label residue %d)" % (
            what, i, views[i][0].data_ptr() % 4, l.data_ptr() % 8), got, labels)
        assert cl.tobytes() == clbytes, "%s frame %d: %s" % (what, i, "; ".join(cluster_fields_equal(cl, np.frombuffer(clbytes, cl.dtype))))


@pytest.fixture(scope="module")
def one_slot():
    """One slot: the frames of an iterate_batch call share every launch, and last_path(0) speaks of the call just made."""
    e = Engine(0, 1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pipe():
    """The submit / drain pipeline on one slot of its own."""
    e = Engine(0, 1)
    yield e
    e.close()


def run_every_entry_point(engine, one_slot, pipe, H, W, K, p, path, want, tag):
    ptrs = lambda views, j: [views[i][j].data_ptr() for i in sorted(views)]
    # iterate_device, once per residue: frame i alone in its allocation, guard on both sides of it
    for i in range(4):
        c, views = carve_frames(H, W, [i])
        cls = fresh_clusters(H, W, K, [i])
        engine.iterate_device(views[i][0].data_ptr(), views[i][1].data_ptr(), H, W, cls[0], p, slot=i % engine.n_slots)
        assert engine.last_path(i % engine.n_slots) == path
        assert_frames("%s iterate_device" % tag, c, views, cls, want)
    # iterate_batch over device pointers: eight frames of mixed residues in ONE launch group
    idx = list(range(GROUP))
    c, views = carve_frames(H, W, idx)
    assert {v[0].data_ptr() % 4 for v in views.values()} == {0, 1, 2, 3} and {v[1].data_ptr() % 8 for v in views.values()} == {0, 2, 4, 6}
    cls = fresh_clusters(H, W, K, idx)
    one_slot.iterate_batch(ptrs(views, 0), cls, ptrs(views, 1), H, W, p, device_ptrs=True)
    assert one_slot.last_group_frames(0) == GROUP and one_slot.last_path(0) == path
    assert_frames("%s iterate_batch" % tag, c, views, cls, want)
    # submit_group / wait_group: frames 1, 2, 3 and 4 (RGB residues 3/1, 2, 1/3, 0; label residues 2, 4, 6, 0)
    idx = [1, 2, 3, 4]
    for eng, name in ((one_slot, "submit_group"), (pipe, "pipeline_submit")):
        c, views = carve_frames(H, W, idx)
        cls = fresh_clusters(H, W, K, idx)
        arrs = (eng.pointer_array(ptrs(views, 0)), eng.pointer_array([cl.ctypes.data for cl in cls]), eng.pointer_array(ptrs(views, 1)))
        if name == "submit_group":
            eng.submit_group(0, arrs[0], arrs[1], arrs[2], len(idx), H, W, K, p)
            eng.wait_group(0)
        else:
            eng.pipeline_submit(arrs[0], arrs[1], arrs[2], len(idx), H, W, K, p)
            assert eng.pipeline_drain()["frames"] == len(idx)
        assert eng.last_group_frames(0) == len(idx) and eng.last_path(0) == path
        assert_frames("%s %s" % (tag, name), c, views, cls, want)


@pytest.mark.parametrize("convert,msf", OPTIONS, ids=lambda v: str(v))
@pytest.mark.parametrize("name,H,W,K,path", SHAPES, ids=[s[0] for s in SHAPES])
def test_integer_slic_at_stacked_and_unaligned_frames(engine, one_slot, pipe, name, H, W, K, path, convert, msf):
    p = make_params(10, 10.0, msf, 3, convert)
    assert (orc.S_of(H, W, K) >= 8) == (path == 0)
    run_every_entry_point(engine, one_slot, pipe, H, W, K, p, path, lambda i: oracle_result(H, W, K, convert, msf, i),
                          "%s convert=%d min_size_factor=%g" % (name, convert, msf))


@pytest.mark.parametrize("kind", [B.VARIANT_REALDIST, B.VARIANT_LSC], ids=["realdist", "lsc"])
@pytest.mark.parametrize("name,H,W,K,path", SHAPES[:2], ids=[s[0] for s in SHAPES[:2]])
def test_float_variants_equal_their_aligned_runs(engine, one_slot, pipe, name, H, W, K, path, kind):
    p = make_params(10, 10.0, 0.25, 3, True, variant=kind)
    aligned = {}
    for i in range(GROUP):                                  # the same call on tensors of their own
        d_rgb = torch.from_numpy(np.array(frame(H, W, i))).cuda()
        d_lab = torch.full((H, W), -7, dtype=torch.int16, device="cuda")
        assert d_rgb.data_ptr() % BASE_ALIGN == 0 and d_lab.data_ptr() % BASE_ALIGN == 0
        cl = orc.initialize_clusters(frame(H, W, i), K)
        engine.iterate_device(d_rgb.data_ptr(), d_lab.data_ptr(), H, W, cl, p)
        torch.cuda.synchronize()
        aligned[i] = (d_lab.cpu().numpy().view(np.uint16), cl.tobytes())
    run_every_entry_point(engine, one_slot, pipe, H, W, K, p, 0, lambda i: aligned[i], "%s variant %d" % (name, kind))


def test_odd_label_pointer_is_refused_before_any_device_work(engine, one_slot, pipe):
    H, W, K = 37, 53, 12
    p = make_params(10, 10.0, 0.25, 3)
    c, views = carve_frames(H, W, [0, 1])
    c.holes[:] = False                                   # nothing may be written at all
    cls = fresh_clusters(H, W, K, [0, 1])
    before = [cl.tobytes() for cl in cls]
    rgb = [views[i][0].data_ptr() for i in (0, 1)]
    lab = [views[0][1].data_ptr(), views[1][1].data_ptr() + 1]
    assert lab[0] % 2 == 0 and lab[1] % 2 == 1
    with pytest.raises(ValueError, match=r"d_labels\[0\] is not 2-byte aligned"):
        engine.iterate_device(rgb[1], lab[1], H, W, cls[1], p)
    with pytest.raises(ValueError, match=r"d_labels\[1\] is not 2-byte aligned"):
        one_slot.iterate_batch(rgb, cls, lab, H, W, p, device_ptrs=True)
    arrs = (one_slot.pointer_array(rgb), one_slot.pointer_array([cl.ctypes.data for cl in cls]), one_slot.pointer_array(lab))
    with pytest.raises(ValueError, match=r"d_labels\[1\] is not 2-byte aligned"):
        one_slot.submit_group(0, arrs[0], arrs[1], arrs[2], 2, H, W, K, p)
    one_slot.wait_group(0)                               # the slot holds nothing
    with pytest.raises(ValueError, match=r"d_labels\[1\] is not 2-byte aligned"):
        pipe.pipeline_submit(arrs[0], arrs[1], arrs[2], 2, H, W, K, p)
    assert pipe.pipeline_drain()["frames"] == 0
    c.check("refused calls")
    assert [cl.tobytes() for cl in cls] == before
    # an odd d_rgb is a frame like any other (iterate_device at residues 1 and 3 above); and the engines still serve
    c, views = carve_frames(H, W, [1])
    cls = fresh_clusters(H, W, K, [1])
    one_slot.iterate_batch([views[1][0].data_ptr()], cls, [views[1][1].data_ptr()], H, W, p, device_ptrs=True)
    assert_frames("after the refusals", c, views, cls, lambda i: oracle_result(H, W, K, True, 0.25, i))


# ---- graph utilities on device planes ----------------------------------------------------------------------------------------------
def test_graph_utilities_on_unaligned_device_planes(engine):
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_cases.npz"))
    case = "slic_96x128_k40"
    labels, mask = gold[case + "/labels"], gold[case + "/mask"]
    cl = np.ascontiguousarray(gold[case + "/clusters"]).view(B.CLUSTER_DTYPE).reshape(-1)
    H, W = labels.shape
    K = cl.shape[0]
    N = H * W
    lab_off, mask_off, out_off = MARGIN + 2, 2 * MARGIN + 2 + 2 * N + 1, 4 * MARGIN + 3 * N + 7      # 2 mod 4; odd; odd
    total = out_off + N + MARGIN

    def planes(with_mask=False, with_out=False):
        c = Carve(total)
        d_lab = c.put(lab_off, labels)
        assert d_lab.data_ptr() % 4 == 2
        d_mask = c.put(mask_off, mask) if with_mask else None
        d_out = c.hole(out_off, (H, W), np.uint8) if with_out else None
        assert all(t is None or t.data_ptr() % 2 == 1 for t in (d_mask, d_out))
        torch.cuda.synchronize()
        return c, d_lab, d_mask, d_out

    c, d_lab, _, _ = planes()
    num, nb = engine.get_connectivity(d_lab.data_ptr(), H, W, K)
    c.check("get_connectivity")
    np.testing.assert_array_equal(num, gold[case + "/conn_num"])
    np.testing.assert_array_equal(nb, gold[case + "/conn_nb"])
    c, d_lab, d_mask, _ = planes(with_mask=True)
    dens = engine.get_mask_density(cl, d_lab.data_ptr(), d_mask.data_ptr(), H, W)
    c.check("get_mask_density")
    np.testing.assert_array_equal(dens, gold[case + "/density"])
    c, d_lab, _, d_out = planes(with_out=True)
    engine.cluster_density_to_mask(d_lab.data_ptr(), dens, H, W, out=d_out.data_ptr())
    c.check("cluster_density_to_mask")
    np.testing.assert_array_equal(d_out.cpu().numpy(), gold[case + "/broadcast"])


# ---- torch-tensor operations on views at a storage offset --------------------------------------------------------------------------
class Spy(object):
    """Records the arguments of the named C-ABI functions (monkeypatched on the loaded library for the length of the test)."""

    def __init__(self, monkeypatch, *names):
        lib = B.load_library()
        self.calls = {n: [] for n in names}
        for n in names:
            monkeypatch.setattr(lib, n, self._wrap(n, getattr(lib, n)))

    def _wrap(self, name, real):
        def call(*args):
            self.calls[name].append([a.value if isinstance(a, C.c_void_p) else a for a in args])
            return real(*args)
        return call

    def assert_reached(self, name, *tensors):
        assert self.calls[name], "%s was not called" % name
        for t in tensors:
            assert any(t.data_ptr() in [a for a in call if isinstance(a, int)] for call in self.calls[name]), \
                "%s did not receive the view's own pointer: the wrapper copied it" % name
        self.calls[name] = []


def view_at(c, off, array, residue=None, mod=16):
    t = c.put(off, array)
    assert t.storage_offset() > 0 and t.is_contiguous()
    if residue is not None:
        assert t.data_ptr() % mod == residue
    return t


def block_labels(H, W, K, seed, dtype=np.int16, cell=7):
    """A map of cell x cell blocks numbered modulo K with noise and a few pixels without a label."""
    rng = np.random.default_rng(seed)
    lab = ((np.arange(H)[:, None] // cell) * ((W + cell - 1) // cell) + np.arange(W)[None, :] // cell) % K
    m = rng.random((H, W)) < 0.08
    lab[m] = rng.integers(0, K, int(m.sum()))
    lab[rng.random((H, W)) < 0.02] = -1
    return np.ascontiguousarray(lab.astype(dtype))


def quarter_features(shape, seed):
    """Multiples of 1/4 in [-16, 16]: every sum of a frame's worth of them is exact in f32 and in f64, whatever the order."""
    return (np.random.default_rng(seed).integers(-64, 65, shape) / 4.0).astype(np.float32)


@pytest.mark.parametrize("H,W", [(20, 70), (37, 53)], ids=["20x70", "37x53"])      # 2 x 2 tiles of 16 x 64 with H * W % 4 == 0; ragged, H * W odd
@pytest.mark.parametrize("foff", [1, 2, 3])
def test_pool_and_unpool_on_offset_views(monkeypatch, H, W, foff):
    from fast_slic_amd.pool import superpixel_pool, superpixel_unpool
    N, Cc, K = 2, 3, 12
    x = quarter_features((N, Cc, H, W), seed=foff)
    lab = np.stack([block_labels(H, W, K, seed=10 + n) for n in range(N)])
    ref = pool_ref.pool(x, lab, K)
    x_off = MARGIN + 4 * foff
    lab_off = -(-(x_off + x.nbytes + MARGIN) // BASE_ALIGN) * BASE_ALIGN + MARGIN + 2
    val_off = -(-(lab_off + lab.nbytes + MARGIN) // BASE_ALIGN) * BASE_ALIGN + MARGIN + 4 * foff
    total = val_off + 4 * N * Cc * K + MARGIN
    spy = Spy(monkeypatch, "fslic_hip_pool", "fslic_hip_unpool")
    for reduce in ("sum", "mean", "max"):
        c = Carve(total)
        xt, lt = view_at(c, x_off, x, 4 * foff), view_at(c, lab_off, lab, 2, 4)
        v, cnt = superpixel_pool(xt, lt, K, reduce=reduce, return_counts=True)
        c.check("superpixel_pool %s" % reduce)
        spy.assert_reached("fslic_hip_pool", xt, lt)
        v, cnt = v.cpu().numpy(), cnt.cpu().numpy()
        assert np.array_equal(cnt, ref["counts"])
        if reduce == "sum":
            assert np.array_equal(v.astype(np.float64), ref["sum"]), "sum"
        elif reduce == "mean":
            cc = ref["counts"][:, None, :]
            want = np.where(cc > 0, ref["sum"].astype(np.float32) / np.maximum(cc, 1).astype(np.float32), np.float32(0)).astype(np.float32)
            assert np.array_equal(v.view(np.uint32), want.view(np.uint32)), "mean"
        else:
            assert np.array_equal(v.view(np.uint32), ref["max"].view(np.uint32)), "max"
    # unpool: the same label view, the values at a float offset as well
    vals = quarter_features((N, Cc, K), seed=40 + foff)
    c = Carve(total)
    lt, vt = view_at(c, lab_off, lab, 2, 4), view_at(c, val_off, vals, 4 * foff)
    out = superpixel_unpool(vt, lt, fill=-7.25)
    c.check("superpixel_unpool")
    spy.assert_reached("fslic_hip_unpool", vt, lt)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), pool_ref.unpool(vals, lab, -7.25).view(np.uint32))


@pytest.mark.parametrize("residue", [4, 8, 12])
def test_raw_unpool_into_an_output_that_is_not_16_byte_aligned(residue):
    """fslic_hip_unpool through the C ABI: H * W % 4 == 0, so only the output's address keeps the launch from the 16-byte stores."""
    from fast_slic_amd.pool import superpixel_unpool
    N, Cc, H, W, K = 2, 3, 20, 70, 12
    assert H * W % 4 == 0
    vals = torch.from_numpy(quarter_features((N, Cc, K), seed=residue)).cuda()
    lab = torch.from_numpy(np.stack([block_labels(H, W, K, seed=20 + n) for n in range(N)])).cuda()
    want = superpixel_unpool(vals.clone(), lab.clone(), fill=1.5)
    assert want.data_ptr() % 16 == 0
    out_off = MARGIN + residue
    c = Carve(out_off + 4 * N * Cc * H * W + MARGIN)
    out = c.hole(out_off, (N, Cc, H, W), np.float32)
    assert out.data_ptr() % 16 == residue
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    B._check(B.load_library().fslic_hip_unpool(0, st, N, Cc, H, W, K, vals.data_ptr(), lab.data_ptr(), 0, None, C.c_float(1.5), out.data_ptr()))
    c.check("fslic_hip_unpool, output at %d mod 16" % residue)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("Cc,lead", [(4, 0), (4, 1), (4, 2), (4, 3), (3, 1), (3, 0)], ids=lambda v: str(v))
def test_graph_of_an_image_at_every_byte_lead(monkeypatch, Cc, lead):
    """superpixel_graph with contrast: a C = 4 image at lead 0 takes a pixel as one dword (`word`), at leads 1..3 and with C = 3 as bytes."""
    from fast_slic_amd.rag import superpixel_graph
    N, H, W, K = 2, 37, 53, 40
    lab = np.stack([block_labels(H, W, K, seed=30 + n) for n in range(N)])
    img = np.random.default_rng(lead + 8 * Cc).integers(0, 256, (N, H, W, Cc)).astype(np.uint8)
    ref = rag_ref.graph(lab, K, 8, img)
    lab_off = MARGIN + 2
    img_off = -(-(lab_off + lab.nbytes + MARGIN) // BASE_ALIGN) * BASE_ALIGN + MARGIN + lead
    c = Carve(img_off + img.nbytes + MARGIN)
    lt, it = view_at(c, lab_off, lab, 2, 4), view_at(c, img_off, img, lead, 4)
    spy = Spy(monkeypatch, "fslic_hip_rag_accumulate")
    g = superpixel_graph(lt, K, connectivity=8, image=it)
    c.check("superpixel_graph")
    spy.assert_reached("fslic_hip_rag_accumulate", lt, it)
    assert np.array_equal(g.edge_index.cpu().numpy(), ref["edge_index"])
    assert np.array_equal(g.boundary.cpu().numpy(), ref["boundary"])
    assert np.array_equal(g.contrast.cpu().numpy(), ref["contrast"])
    assert np.array_equal(g.offsets.cpu().numpy(), ref["offsets"])


@pytest.mark.parametrize("other_dtype", [np.int16, np.int32], ids=["int16", "int32"])
def test_compare_on_offset_views(monkeypatch, other_dtype):
    from fast_slic_amd.compare import label_overlap, boundary_match
    N, H, W, K, M = 2, 37, 53, 40, 24
    lab = np.stack([block_labels(H, W, K, seed=50 + n) for n in range(N)])
    oth = np.stack([block_labels(H, W, M, seed=60 + n, dtype=other_dtype, cell=9) for n in range(N)])
    lab_off = MARGIN + 2
    oth_off = -(-(lab_off + lab.nbytes + MARGIN) // BASE_ALIGN) * BASE_ALIGN + MARGIN + oth.itemsize
    total = oth_off + oth.nbytes + MARGIN
    spy = Spy(monkeypatch, "fslic_hip_overlap_accumulate", "fslic_hip_boundary_match")
    c = Carve(total)
    lt, ot = view_at(c, lab_off, lab, 2, 4), view_at(c, oth_off, oth, oth.itemsize, 2 * oth.itemsize)
    t = label_overlap(lt, ot, K, M)
    c.check("label_overlap")
    spy.assert_reached("fslic_hip_overlap_accumulate", lt, ot)
    ref = compare_ref.overlap(lab.view(np.uint16), oth if other_dtype != np.int16 else oth.view(np.uint16), K, M)
    assert np.array_equal(t.pairs.cpu().numpy(), ref["pairs"]) and np.array_equal(t.count.cpu().numpy(), ref["count"])
    assert np.array_equal(t.offsets.cpu().numpy(), ref["offsets"])
    for tol in (0, 2):
        c = Carve(total)
        lt, ot = view_at(c, lab_off, lab, 2, 4), view_at(c, oth_off, oth, oth.itemsize, 2 * oth.itemsize)
        m = boundary_match(lt, ot, tolerance=tol)
        c.check("boundary_match")
        spy.assert_reached("fslic_hip_boundary_match", lt, ot)
        assert np.array_equal(m.cpu().numpy(), compare_ref.boundary_match(lab, oth, tol))


def test_crf_forward_and_backward_on_offset_views(monkeypatch):
    """superpixel_crf with every tensor a view at a storage offset -- forward without gradients, forward with gradients and one backward
    whose incoming gradient is such a view too -- against the same calls on fresh clones, byte for byte."""
    from fast_slic_amd.crf_torch import superpixel_crf
    N, Cn, K = 2, 5, 37
    rng = np.random.default_rng(77)
    yx = np.stack([np.stack([rng.uniform(0, 37, K), rng.uniform(0, 53, K), rng.integers(0, 256, K), rng.integers(0, 256, K),
                             rng.integers(0, 256, K)]) for _ in range(N)]).astype(np.float32)
    mem = rng.integers(0, 90, (N, K)).astype(np.int32)
    rows = [[int(v) for v in rng.integers(0, K, int(rng.integers(0, 9)))] for _ in range(N * K)]
    off = np.zeros(N * K + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    idx = np.array([v for r in rows for v in r], np.int32)
    un = rng.uniform(0.0, 4.0, (N, Cn, K)).astype(np.float32)
    q0 = rng.uniform(0.05, 1.0, (N, Cn, K))
    q0 = (q0 / q0.sum(1, keepdims=True)).astype(np.float32)
    comp = np.array([0.5 + 0.25 * (c % 5) for c in range(Cn)], np.float32)
    grad = rng.normal(0.0, 1.0, (N, Cn, K)).astype(np.float32)
    params = dict(spatial_w=0.05, temporal_w=0.05, spatial_srgb=300.0, temporal_srgb=300.0, spatial_sxy=2000.0, spatial_smooth_w=0.02,
                  spatial_smooth_sxy=1000.0)
    arrays = dict(un=un, q0=q0, comp=comp, grad=grad, yx=yx, mem=mem, off=off, idx=idx)
    lead = dict(un=4, q0=8, comp=12, grad=4, yx=8, mem=12, off=8, idx=4)          # bytes past a 512-byte boundary

    def carve():
        offs, at = {}, 0
        for k, a in arrays.items():
            offs[k] = at + MARGIN + lead[k]
            at = -(-(offs[k] + a.nbytes + MARGIN) // BASE_ALIGN) * BASE_ALIGN
        c = Carve(at)
        return c, {k: view_at(c, offs[k], a, lead[k]) for k, a in arrays.items()}

    def clones():
        return {k: torch.from_numpy(a.copy()).cuda() for k, a in arrays.items()}

    def forward(t, grads):
        for k in ("un", "q0", "comp"):
            t[k].requires_grad_(grads)
        return superpixel_crf(t["un"], (t["off"], t["idx"]), t["yx"], t["mem"], max_iter=3, params=params, compat=t["comp"],
                              temporal=True, q0=t["q0"])

    spy = Spy(monkeypatch, "fslic_hip_crf_tensor_inference", "fslic_hip_crf_tensor_inference_saved", "fslic_hip_crf_tensor_backward")
    inputs = ("un", "q0", "comp", "yx", "mem", "off", "idx")
    want = forward(clones(), False)
    c, t = carve()
    got = forward(t, False)
    c.check("superpixel_crf forward")
    spy.assert_reached("fslic_hip_crf_tensor_inference", *[t[k] for k in inputs])
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # with gradients
    tc = clones()
    qc = forward(tc, True)
    qc.backward(tc["grad"])
    c, t = carve()
    q = forward(t, True)
    spy.assert_reached("fslic_hip_crf_tensor_inference_saved", *[t[k] for k in inputs])
    q.backward(t["grad"])
    c.check("superpixel_crf forward and backward")
    spy.assert_reached("fslic_hip_crf_tensor_backward", t["grad"], t["comp"], t["mem"], t["off"], t["idx"])
    assert torch.equal(q.detach().view(torch.int32), want.view(torch.int32)) and torch.equal(qc.detach().view(torch.int32), want.view(torch.int32))
    for k in ("un", "q0", "comp"):
        assert t[k].grad is not None and torch.equal(t[k].grad.view(torch.int32), tc[k].grad.view(torch.int32)), "gradient of %s" % k
