"""Slic on torch tensors on the MI355X (fast_slic_amd/frames.py, csrc/ingest.hip), with exact equality throughout: k_pack_rgb against the
numpy model of tests/frames_ref.py for every dtype and layout at shapes whose planes are and are not 16-byte aligned and end in tails of
1 - 3 pixels; its footprint; slic_tensor against per-frame Slic.iterate on numpy for the five variants, batches of several groups with a
ragged last one, the warm start, the ordering against torch's streams and the chain into the graph and the tensor CRF."""
import functools

import numpy as np
import pytest
import torch

import frames_ref as R
import fast_slic_amd
from fast_slic_amd import frames as F
from fast_slic_amd.crf_torch import superpixel_crf
from fast_slic_amd.frames import pack_rgb, slic_tensor
from fast_slic_amd.pool import superpixel_pool
from fast_slic_amd.rag import superpixel_graph
from fast_slic_amd.synth import variant

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# H * W = 1, 6, 91, 1024, 1139, 4290: odd and even plane sizes (every other plane of an odd one is off the 16-byte grid), tails of 1, 2
# and 3 pixels behind the last whole quad, one block (1024 pixels) exactly, just above, and several
SHAPES = [(1, 1), (2, 3), (7, 13), (16, 64), (17, 67), (33, 130)]
DTYPES = [torch.uint8, torch.float16, torch.bfloat16, torch.float32]
KINDS = ["nchw", "nhwc", "channels_last", "crop", "offset", "gray"]
SCALES = [255.0, 1.0, 127.5]
GUARD = 64


def values(shape, dtype, scale, seed):
    """A CPU tensor of `shape`: bytes for uint8; for floats values whose product with `scale` covers [-20, 275], with ties (k + 0.5),
    both clamps, NaN and the infinities sprinkled in."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if dtype == torch.uint8:
        return torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8).reshape(shape))
    v = rng.uniform(-20.0, 275.0, n)
    ties = rng.random(n) < 0.3
    v[ties] = np.floor(v[ties]) + 0.5
    v = (v / scale).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 0.5 / scale, 1.5 / scale, 2.5 / scale, 254.5 / scale, 255.5 / scale,
                        -0.4 / scale], np.float32)
    at = rng.integers(0, n, min(n, 2 * len(special)))
    v[at] = special[np.arange(len(at)) % len(special)]
    return torch.from_numpy(v.reshape(shape)).to(dtype)


def source(kind, dtype, N, H, W, scale, seed):
    """(base, src, channels_first): base the tensor that owns the memory on the GPU, src the view of it that is packed."""
    if kind == "nchw":
        base = values((N, 3, H, W), dtype, scale, seed).to(DEV)
        return base, base, True
    if kind == "nhwc":
        base = values((N, H, W, 3), dtype, scale, seed).to(DEV)
        return base, base, False
    if kind == "channels_last":
        base = values((N, 3, H, W), dtype, scale, seed).to(DEV).contiguous(memory_format=torch.channels_last)
        return base, base, True
    if kind == "crop":
        base = values((N, 3, H + 2, W + 5), dtype, scale, seed).to(DEV)
        return base, base[:, :, 1:-1, 2:-3], True
    if kind == "offset":
        base = values((N * 3 * H * W + 1,), dtype, scale, seed).to(DEV)
        return base, base[1:].view(N, 3, H, W), True
    base = values((N, 1, H, W), dtype, scale, seed).to(DEV)
    return base, base.expand(N, 3, H, W), True


def model_input(src, channels_first):
    """The [N, 3, H, W] numpy array the model reads: bfloat16 widened exactly to float32."""
    x = src.cpu() if channels_first else src.cpu().permute(0, 3, 1, 2)
    return (x.to(torch.float32) if x.dtype == torch.bfloat16 else x).numpy()


def bits(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().copy()


def guarded(N, pitch):
    big = torch.full((GUARD + N * pitch + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    return big, big[GUARD:GUARD + N * pitch].view(N, pitch)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_pack_equals_the_model_inside_its_footprint(H, W, N):
    pitch = F.frame_pitch(H, W)
    assert pitch == R.frame_pitch(H, W) and pitch % 16 == 0 and 0 <= pitch - 3 * H * W < 16
    seed = 0
    for dtype in DTYPES:
        for kind in KINDS:
            for scale in (SCALES if dtype != torch.uint8 else [255.0]):
                seed += 1
                what = (str(dtype), kind, scale)
                base, src, cf = source(kind, dtype, N, H, W, scale, seed)
                before = bits(base)
                big, out = guarded(N, pitch)
                got, gh, gw = pack_rgb(src, scale=scale, channels_first=cf, out=out)
                assert got is out and (gh, gw) == (H, W), what
                want = R.pack(model_input(src, cf), scale)
                host = big.cpu().numpy()
                assert np.array_equal(host[GUARD:-GUARD].reshape(N, pitch), want), what
                assert (host[:GUARD] == 0xAB).all() and (host[-GUARD:] == 0xAB).all(), what
                assert not host[GUARD:-GUARD].reshape(N, pitch)[:, 3 * H * W:].any(), what
                assert np.array_equal(bits(base), before), what                       # the source is bit-identical afterwards
                # repeated calls, a fresh buffer of the call's own, and a frame alone give the same bytes
                again, _, _ = pack_rgb(src, scale=scale, channels_first=cf)
                assert tuple(again.shape) == (N, pitch) and again.dtype == torch.uint8 and again.device == DEV, what
                assert np.array_equal(again.cpu().numpy(), want), what
                alone, _, _ = pack_rgb(src[N - 1], scale=scale, channels_first=cf)
                assert np.array_equal(alone.cpu().numpy(), want[N - 1:]), what


def test_pack_with_a_wider_pitch_and_the_default_arguments():
    H, W, N = 17, 67, 2
    base, src, _ = source("nchw", torch.float32, N, H, W, 255.0, 5)
    pitch = F.frame_pitch(H, W) + 48
    big, out = guarded(N, pitch)
    pack_rgb(src, out=out)                                       # floats: channel-first, scale 255
    host = big.cpu().numpy()
    assert np.array_equal(host[GUARD:-GUARD].reshape(N, pitch), R.pack(model_input(src, True), 255.0, pitch))
    assert (host[:GUARD] == 0xAB).all() and (host[-GUARD:] == 0xAB).all()
    u8 = values((H, W, 3), torch.uint8, 1.0, 6).to(DEV)          # uint8: channel-last, unbatched
    got, _, _ = pack_rgb(u8)
    assert np.array_equal(got.cpu().numpy()[0, :3 * H * W], u8.cpu().numpy().reshape(-1))


# ---- slic_tensor against the numpy route ----
VARIANTS = ["Slic", "LSC", "SlicRealDist", "SlicRealDistL2", "SlicRealDistNoQ"]
CASES = [(61, 83, 20), (120, 160, 40), (96, 128, 300)]
MAXN = 17


@functools.lru_cache(maxsize=None)
def frames_u8(H, W):
    """uint8 [MAXN, H, W, 3]: synthetic frames, all different."""
    a = np.stack([variant("A" if i % 3 else "B", H, W, seed=i) for i in range(MAXN)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def numpy_route(vname, H, W, K):
    """Per frame: (labels int16 [H, W], the model's Cluster[K] bytes) of a fresh `vname`(K).iterate(frame)."""
    out = []
    for img in frames_u8(H, W):
        s = getattr(fast_slic_amd, vname)(num_components=K)
        lab = s.iterate(np.ascontiguousarray(img))
        out.append((lab.copy(), s.slic_model.cluster_array.tobytes()))
    return out


def check(r, want, what):
    lab = r.labels.cpu().numpy()
    assert r.labels.dtype == torch.int16 and r.labels.device == DEV and r.clusters.dtype == fast_slic_amd.CLUSTER_DTYPE, what
    assert lab.shape == (len(want),) + want[0][0].shape and r.clusters.shape[0] == len(want), what
    for n, (wl, wc) in enumerate(want):
        assert np.array_equal(lab[n], wl), what + (n,)
        assert r.clusters[n].tobytes() == wc, what + (n,)


@pytest.mark.parametrize("H,W,K", CASES)
@pytest.mark.parametrize("vname", VARIANTS)
def test_slic_tensor_equals_the_numpy_route(vname, H, W, K, monkeypatch):
    want = numpy_route(vname, H, W, K)
    u8 = torch.from_numpy(frames_u8(H, W).copy()).to(DEV)
    # float32 NCHW made as uint8 / 255 (tests/test_frames_cpu.py: it rounds back to the same bytes for all 256 values)
    f32 = torch.from_numpy(frames_u8(H, W).astype(np.float32) / np.float32(255)).to(DEV).permute(0, 3, 1, 2).contiguous()
    slic = getattr(fast_slic_amd, vname)(num_components=K)
    for N in (1, 2, 9, 17):
        check(slic_tensor(f32[:N], slic), want[:N], (vname, "f32 nchw", N))
        with monkeypatch.context() as m:      # a contiguous uint8 NHWC batch is used in place: no pack launch
            m.setattr(F, "_pack", None)
            check(slic_tensor(u8[:N], slic), want[:N], (vname, "u8 nhwc", N))
    r = slic_tensor(u8[3], slic)              # unbatched [H, W, 3]
    assert tuple(r.labels.shape) == (H, W) and r.clusters.shape == (1, K) and r.num_components == K
    assert np.array_equal(r.labels.cpu().numpy(), want[3][0]) and r.clusters[0].tobytes() == want[3][1]
    # the slic object only supplied the options
    m = slic.slic_model
    assert not m.initialized and slic.last_assignment is None and not m.cluster_array.view(np.uint8).any()


def test_lsc_replays_of_a_one_frame_device_group_equal_the_single_run():
    """What the LSC cases above met first: a slot that serves the same one-frame LSC group over device pointers again and again enqueues
    it directly, records its graph, then replays it -- and every replay gives the single run's result (the clear of the LSC accumulators
    is a kernel node of that graph; as a memset node of one row it left the third replay with the sums of the second)."""
    H, W, K = 61, 83, 20
    img = np.ascontiguousarray(frames_u8(H, W)[0])
    p = fast_slic_amd.LSC(num_components=K).slic_model.iterate_params(10, 10, 0.25, 3)
    lib = fast_slic_amd._binding.load_library()

    def seeds():
        cl = np.zeros(K, fast_slic_amd.CLUSTER_DTYPE)
        assert lib.fslic_hip_initialize_clusters(H, W, K, img.ctypes.data, cl.ctypes.data) == 0
        return cl

    e = fast_slic_amd.Engine(0, 1)
    try:
        cl0 = seeds()
        want = e.iterate(img, cl0, p).view(np.int16).copy()
        frame = torch.from_numpy(img.copy()).to(DEV)
        modes = []
        for rep in range(8):
            cl = seeds()
            lab = torch.full((H, W), -2, dtype=torch.int16, device=DEV)
            torch.cuda.synchronize(DEV)
            e.iterate_batch([frame.data_ptr()], [cl], [lab.data_ptr()], H, W, p, device_ptrs=True)
            modes.append(e.last_launch_mode(0))
            assert np.array_equal(lab.cpu().numpy(), want) and cl.tobytes() == cl0.tobytes(), (rep, modes)
        assert modes[-1] == 2, modes          # the last ones were replays
    finally:
        e.close()


def test_slic_tensor_packs_other_layouts_to_the_same_frames():
    H, W, K = 61, 83, 20
    want = numpy_route("Slic", H, W, K)[:3]
    slic = fast_slic_amd.Slic(num_components=K)
    u8 = torch.from_numpy(frames_u8(H, W)[:3].copy()).to(DEV)
    chw = u8.permute(0, 3, 1, 2)
    check(slic_tensor(chw, slic, channels_first=True), want, ("u8 nchw view",))
    check(slic_tensor(chw.to(torch.float16), slic, scale=1.0), want, ("f16 integer-valued",))
    check(slic_tensor(chw.to(torch.bfloat16).contiguous(memory_format=torch.channels_last), slic, scale=1.0), want, ("bf16 channels_last",))
    big = torch.zeros((3, H + 3, W + 4, 3), dtype=torch.uint8, device=DEV)
    big[:, 1:-2, 3:-1] = u8
    check(slic_tensor(big[:, 1:-2, 3:-1], slic), want, ("u8 nhwc crop",))


def test_warm_start_equals_consecutive_iterate_calls():
    H, W, K = 120, 160, 40
    f = frames_u8(H, W)
    ref = fast_slic_amd.Slic(num_components=K)
    a1 = ref.iterate(np.ascontiguousarray(f[0])).copy()
    c1 = ref.slic_model.cluster_array.tobytes()
    forks = [fast_slic_amd.Slic(slic_model=ref.slic_model) for _ in range(2)]      # two copies of the model after frame 0
    a2 = ref.iterate(np.ascontiguousarray(f[1])).copy()
    c2 = ref.slic_model.cluster_array.tobytes()
    slic = fast_slic_amd.Slic(num_components=K)
    t = torch.from_numpy(f[:3].copy()).to(DEV)
    r1 = slic_tensor(t[0:1], slic)
    assert np.array_equal(r1.labels.cpu().numpy()[0], a1) and r1.clusters[0].tobytes() == c1
    kept = r1.clusters.tobytes()
    r2 = slic_tensor(t[1:2], slic, clusters=r1.clusters)
    assert np.array_equal(r2.labels.cpu().numpy()[0], a2) and r2.clusters[0].tobytes() == c2
    assert r1.clusters.tobytes() == kept and r2.clusters is not r1.clusters       # the caller's array is not written
    # a [K] block starts every frame of a batch
    r3 = slic_tensor(t[1:3], slic, clusters=r1.clusters[0])
    for n, fork in enumerate(forks):
        lab = fork.iterate(np.ascontiguousarray(f[1 + n]))
        assert np.array_equal(r3.labels.cpu().numpy()[n], lab) and r3.clusters[n].tobytes() == fork.slic_model.cluster_array.tobytes()
    assert r1.clusters.tobytes() == kept
    m = slic.slic_model
    assert not m.initialized and slic.last_assignment is None and not m.cluster_array.view(np.uint8).any()


def test_ordering_against_torch_streams():
    H, W, K, N = 120, 160, 40, 4
    want = numpy_route("Slic", H, W, K)[:N]
    slic = fast_slic_amd.Slic(num_components=K)
    host = torch.from_numpy(frames_u8(H, W)[:N].copy()).to(DEV)
    feat = torch.from_numpy(np.random.default_rng(3).standard_normal((N, 5, H, W)).astype(np.float32)).to(DEV)
    plain = slic_tensor(host, slic)
    check(plain, want, ("plain",))
    pooled = superpixel_pool(feat, plain.labels, K)
    frames = torch.zeros_like(host)                      # zeros until the side stream's copy lands
    big = torch.ones(1 << 26, device=DEV)
    torch.cuda.synchronize(DEV)
    s, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        for _ in range(24):                              # 256 MB read and written per op: the copy below waits behind all of them
            big = big * 1.0001
        frames.copy_(host)
        r = slic_tensor(frames, slic)
    with torch.cuda.stream(s2):                          # the results are valid on every stream when the call returns
        got = superpixel_pool(feat, r.labels, K)
    s2.synchronize()
    check(r, want, ("side stream",))
    assert torch.equal(got, pooled)
    with torch.cuda.stream(s):                           # and through the pack kernel, which runs on the current stream
        for _ in range(24):
            big = big * 1.0001
        f32 = (frames.permute(0, 3, 1, 2).to(torch.float32) * 1.0).contiguous()
        r = slic_tensor(f32, slic, scale=1.0)
    check(r, want, ("side stream, packed",))
    torch.cuda.synchronize(DEV)


def test_chain_into_the_graph_and_the_tensor_crf():
    H, W, K, N, Cn = 96, 128, 300, 3, 4
    f = frames_u8(H, W)[:N]
    slic = fast_slic_amd.Slic(num_components=K)
    r = slic_tensor(torch.from_numpy(f.copy()).to(DEV), slic)
    labs, yxm = [], []
    for img in f:
        s = fast_slic_amd.Slic(num_components=K)
        labs.append(s.iterate(np.ascontiguousarray(img)).copy())
        yxm.append(s.slic_model.to_yxmrgb())
    yxm = np.stack(yxm)                                                     # [N, K, 6]: y, x, members, r, g, b
    yxrgb = torch.from_numpy(np.ascontiguousarray(yxm[:, :, [0, 1, 3, 4, 5]].transpose(0, 2, 1)).astype(np.float32)).to(DEV)
    members = torch.from_numpy(yxm[:, :, 2].astype(np.int32)).to(DEV)
    assert r.yxrgb.dtype == torch.float32 and tuple(r.yxrgb.shape) == (N, 5, K) and r.yxrgb.is_contiguous()
    assert r.members.dtype == torch.int32 and tuple(r.members.shape) == (N, K) and r.members.is_contiguous()
    assert torch.equal(r.yxrgb, yxrgb) and torch.equal(r.members, members) and r.yxrgb is r.yxrgb
    g1 = superpixel_graph(r.labels, K)
    g2 = superpixel_graph(np.stack(labs), K)
    for name in ("edge_index", "boundary", "offsets"):
        assert torch.equal(getattr(g1, name), getattr(g2, name)), name
    un = torch.from_numpy(np.random.default_rng(4).random((N, Cn, K)).astype(np.float32) * 3).to(DEV)
    q1 = superpixel_crf(un, g1, r.yxrgb, r.members)
    q2 = superpixel_crf(un, g2, yxrgb, members)
    assert torch.equal(q1, q2) and bool(torch.isfinite(q1).all())


def test_another_device_leaves_the_current_one_alone():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    H, W, K = 61, 83, 20
    want = numpy_route("Slic", H, W, K)[:2]
    other = torch.device("cuda", 1)
    assert torch.cuda.current_device() == 0
    r = slic_tensor(torch.from_numpy(frames_u8(H, W)[:2].copy()).to(other), fast_slic_amd.Slic(num_components=K))
    assert torch.cuda.current_device() == 0 and r.labels.device == other and r.yxrgb.device == other
    for n, (wl, wc) in enumerate(want):
        assert np.array_equal(r.labels[n].cpu().numpy(), wl) and r.clusters[n].tobytes() == wc
