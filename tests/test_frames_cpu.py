"""CPU tests of Slic on torch tensors (fast_slic_amd/frames.py, fslic_hip_pack_rgb, fslic_hip_seed_positions): the numpy model of the pack
rule (tests/frames_ref.py) on hand-written values, the seed positions against fslic_hip_initialize_clusters, every argument error refused
before any device work -- ValueError in Python, FSLIC_E_INVALID from the C ABI before its first HIP call -- and the agreement of the
header, EXPORTS and the library on the two new names.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from fast_slic_amd import _binding as B
from fast_slic_amd import frames as F
from fast_slic_amd.base_slic import BaseSlic
from fast_slic_amd.synth import variant
from oracle import oracle as orc
import frames_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fslic_hip_pack_rgb", "fslic_hip_seed_positions"]
CAPI_CASES = [(480, 640, 200), (2160, 3840, 6000), (37, 53, 7), (10, 10, 100), (5, 300, 17)]      # tests/test_capi_cpu.py


def lib():
    return B.load_library()


# ---- the model of the pack rule on hand-written values ----
def test_model_ties_go_to_even():
    x = np.array([0.5, 1.5, 2.5, 254.5, 3.5, 0.49999997, 0.50000006], np.float32)
    assert R.to_bytes(x, 1.0).tolist() == [0, 2, 2, 254, 4, 0, 1]


def test_model_clamps_nan_and_infinities():
    x = np.array([255.5, 256.0, 1e30, -0.4, -0.0, -1e30, np.nan, np.inf, -np.inf], np.float32)
    assert R.to_bytes(x, 1.0).tolist() == [255, 255, 255, 0, 0, 0, 0, 255, 0]
    assert R.to_bytes(np.array([np.inf, -np.inf, np.nan], np.float32), 0.0).tolist() == [0, 0, 0]      # inf * 0 is NaN
    assert R.to_bytes(np.array([1.0, -1.0], np.float32), -255.0).tolist() == [0, 255]


def test_model_product_is_one_float32_rounding():
    """The vectorised model against the same rule written out in scalar float32 arithmetic."""
    for s in (255.0, 127.5, 1.0):
        v = np.linspace(-0.5, 2.5, 4001, dtype=np.float32)
        exp = [int(np.rint(min(max(np.float32(a) * np.float32(s), np.float32(0)), np.float32(255)))) for a in v]
        assert R.to_bytes(v, s).tolist() == exp


def test_model_uint8_round_trip_through_unit_floats():
    """What the GPU tests rely on: float32(k) / 255 * 255 rounds back to k for every byte, so `uint8 / 255` frames pack to their bytes."""
    k = np.arange(256, dtype=np.float32)
    assert np.array_equal(np.rint(k / np.float32(255) * np.float32(255)), k)
    assert R.to_bytes(k / np.float32(255), 255.0).tolist() == list(range(256))
    assert R.to_bytes(np.arange(256, dtype=np.uint8), 123.0).tolist() == list(range(256))      # uint8 is copied, scale ignored


def test_model_half_and_bfloat16_widen_exactly():
    h = np.array([0.5, 1.5, 2.5, 254.5, 300.0, -2.0, np.nan, np.inf, 0.1], np.float16)
    assert R.to_bytes(h, 1.0).tolist() == [0, 2, 2, 254, 255, 0, 0, 255, 0]
    assert R.to_bytes(np.array([0.1], np.float16), 255.0).tolist() == [int(np.rint(np.float32(np.float16(0.1)) * np.float32(255)))]
    t = torch.tensor([0.5, 1.5, 2.5, 254.0, 300.0, -2.0, float("nan"), float("inf"), 0.1], dtype=torch.bfloat16)
    wide = R.bf16_bits_to_f32(t.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(wide.view(np.uint32), t.to(torch.float32).numpy().view(np.uint32))
    assert R.to_bytes(wide, 1.0).tolist() == [0, 2, 2, 254, 255, 0, 0, 255, 0]
    assert R.to_bytes(wide[-1:], 255.0).tolist() == [int(np.rint(np.float32(0.10009765625) * np.float32(255)))]


def test_model_layout_and_padding():
    x = np.arange(2 * 3 * 2 * 3, dtype=np.uint8).reshape(2, 3, 2, 3)
    out = R.pack(x, 1.0)
    assert out.shape == (2, 32) and R.frame_pitch(2, 3) == 32 and F.frame_pitch(2, 3) == 32
    assert out[0, :18].tolist() == [0, 6, 12, 1, 7, 13, 2, 8, 14, 3, 9, 15, 4, 10, 16, 5, 11, 17] and not out[:, 18:].any()
    assert [F.frame_pitch(h, w) for h, w in ((1, 1), (7, 13), (16, 64), (720, 1280))] == [16, 288, 3072, 2764800]


# ---- seed positions ----
@pytest.mark.parametrize("H,W,K", CAPI_CASES)
def test_seed_positions_equal_initialize_clusters_on_a_zero_image(H, W, K):
    seed = np.zeros(K, B.CLUSTER_DTYPE)
    assert lib().fslic_hip_seed_positions(H, W, K, seed.ctypes.data) == 0
    full = np.zeros(K, B.CLUSTER_DTYPE)
    zero = np.zeros((H, W, 3), np.uint8)
    assert lib().fslic_hip_initialize_clusters(H, W, K, zero.ctypes.data, full.ctypes.data) == 0
    assert seed.tobytes() == full.tobytes()
    # and with an image: the oracle's clusters, whose positions, numbers and flags are the seed's
    img = variant("A", H, W)
    assert lib().fslic_hip_initialize_clusters(H, W, K, img.ctypes.data, full.ctypes.data) == 0
    assert full.tobytes() == orc.initialize_clusters(img, K).tobytes()
    for name in ("y", "x", "a", "number", "is_active", "is_updatable", "num_members"):
        assert np.array_equal(full[name], seed[name]), name
    y, x = seed["y"].astype(np.int64), seed["x"].astype(np.int64)
    for c, name in enumerate("rgb"):          # the gather index frames.py uses: byte 3 (W y + x) + c of the frame
        assert np.array_equal(full[name], img.reshape(-1)[3 * (W * y + x) + c].astype(np.float32)), name


def test_seed_positions_sets_the_colours_to_zero_and_refuses_null():
    cl = np.zeros(7, B.CLUSTER_DTYPE)
    cl["r"], cl["g"], cl["b"], cl["a"] = 5, 6, 7, 8
    assert lib().fslic_hip_seed_positions(37, 53, 7, cl.ctypes.data) == 0
    assert not cl["r"].any() and not cl["g"].any() and not cl["b"].any() and (cl["a"] == 8).all()
    assert lib().fslic_hip_seed_positions(37, 53, 7, None) == B.FSLIC_E_INVALID
    assert b"NULL" in lib().fslic_hip_last_error()
    before = cl.tobytes()
    for H, W, K in ((0, 53, 7), (37, 0, 7), (37, 53, 0), (-1, 53, 7)):      # like initialize_clusters: a silent return
        assert lib().fslic_hip_seed_positions(H, W, K, cl.ctypes.data) == 0
    assert cl.tobytes() == before


# ---- fslic_hip_pack_rgb refuses every bad argument before its first HIP call ----
def pack_args(**kw):
    a = dict(device=0, stream=None, N=2, H=7, W=13, src=C.c_void_p(0x1000), src_type=3, strides=(C.c_longlong * 4)(273, 91, 13, 1),
             scale=C.c_float(255.0), out=C.c_void_p(0x2000), pitch=C.c_size_t(288))
    a.update(kw)
    return [a[k] for k in ("device", "stream", "N", "H", "W", "src", "src_type", "strides", "scale", "out", "pitch")]


@pytest.mark.parametrize("kw,word", [
    (dict(device=-1), b"device"), (dict(src=None), b"NULL"), (dict(out=None), b"NULL"), (dict(strides=None), b"NULL"),
    (dict(N=0), b"positive"), (dict(N=-3), b"positive"), (dict(H=0), b"positive"), (dict(W=-1), b"positive"),
    (dict(H=1 << 16, W=1 << 15, pitch=C.c_size_t(3 << 31)), b"2^31"),
    (dict(src_type=4), b"source type"), (dict(src_type=-1), b"source type"),
    (dict(pitch=C.c_size_t(272)), b"pitch"), (dict(pitch=C.c_size_t(280)), b"pitch"), (dict(pitch=C.c_size_t(0)), b"pitch"),
    (dict(pitch=C.c_size_t((1 << 33) + 16)), b"pitch"),
    (dict(scale=C.c_float(float("nan"))), b"scale"), (dict(scale=C.c_float(float("inf"))), b"scale"), (dict(scale=C.c_float(float("-inf"))), b"scale"),
    (dict(out=C.c_void_p(0x2002)), b"aligned"), (dict(src=C.c_void_p(0x1002)), b"aligned"), (dict(src=C.c_void_p(0x1001), src_type=1), b"aligned"),
    (dict(N=1 << 30, pitch=C.c_size_t(6160)), b"too many frames"),
])
def test_pack_rgb_entry_refuses_bad_arguments(kw, word):
    assert lib().fslic_hip_pack_rgb(*pack_args(**kw)) == B.FSLIC_E_INVALID
    assert word in lib().fslic_hip_last_error(), lib().fslic_hip_last_error()


# ---- the Python calls refuse every bad argument before any device work (the images here are CPU tensors: refused last) ----
class StubSlic(BaseSlic):
    """A BaseSlic whose model needs no engine (constructing a SlicModel needs a GPU)."""

    def make_slic_model(self, num_components):
        m = object.__new__(B.SlicModel)
        m.num_components, m.real_dist, m.real_dist_type, m.initialized = num_components, False, "standard", False
        m._clusters = np.zeros(min(num_components, 8), B.CLUSTER_DTYPE)
        return m


GOOD = torch.zeros(2, 3, 7, 13)


@pytest.mark.parametrize("call", [F.pack_rgb, lambda *a, **k: F.slic_tensor(a[0], StubSlic(20), **k)])
@pytest.mark.parametrize("images,kw,word", [
    (np.zeros((2, 3, 7, 13), np.float32), {}, "torch tensor"),
    (torch.zeros(2, 3, 7, 13, dtype=torch.float64), {}, "uint8, float16"),
    (torch.zeros(2, 3, 7, 13, dtype=torch.int16), {}, "uint8, float16"),
    (torch.zeros(7, 13), {}, "shape"), (torch.zeros(1, 2, 3, 7, 13), {}, "shape"),
    (torch.zeros(2, 4, 7, 13), {}, "3 channels"), (torch.zeros(2, 7, 13, 3), {}, "3 channels"),
    (torch.zeros(2, 3, 7, 13, dtype=torch.uint8), {}, "3 channels"), (torch.zeros(7, 13, 3), dict(channels_first=True), "3 channels"),
    (torch.zeros(2, 3, 0, 13), {}, "empty"), (torch.zeros(0, 3, 7, 13), {}, "empty"),
    (GOOD, dict(channels_first=1), "channels_first"),
    (GOOD, dict(scale=float("nan")), "scale"), (GOOD, dict(scale=float("inf")), "scale"), (GOOD, dict(scale="255"), "scale"),
    (GOOD, dict(scale=True), "scale"),
    (GOOD, {}, "ROCm GPU"), (torch.zeros(7, 13, 3, dtype=torch.uint8), {}, "ROCm GPU"), (torch.zeros(2, 7, 13, 3), dict(channels_first=False), "ROCm GPU"),
])
def test_python_calls_refuse_bad_images(call, images, kw, word):
    with pytest.raises(ValueError, match=word):
        call(images, **kw)


@pytest.mark.parametrize("out,word", [
    (torch.zeros(2, 288), "uint8"), (torch.zeros(2 * 288, dtype=torch.uint8), "uint8"), (torch.zeros(3, 288, dtype=torch.uint8), "uint8"),
    (torch.zeros(2, 576, dtype=torch.uint8)[:, :288], "contiguous"), (torch.zeros(2, 272, dtype=torch.uint8), "pitch"),
    (torch.zeros(2, 280, dtype=torch.uint8), "pitch"), (np.zeros((2, 288), np.uint8), "uint8"),
    (torch.zeros(2 * 288 + 1, dtype=torch.uint8)[1:].view(2, 288), "aligned"),
])
def test_pack_rgb_refuses_a_bad_out(out, word):
    with pytest.raises(ValueError, match=word):
        F.pack_rgb(GOOD, out=out)


def test_slic_tensor_refuses_bad_arguments():
    ok = np.zeros((2, 20), B.CLUSTER_DTYPE)
    for kw, word in [(dict(clusters=np.zeros((2, 20), np.float32)), "CLUSTER_DTYPE"), (dict(clusters=[ok[0], ok[1]]), "CLUSTER_DTYPE"),
                     (dict(clusters=np.zeros((3, 20), B.CLUSTER_DTYPE)), "clusters must be"),
                     (dict(clusters=np.zeros((1, 2, 20), B.CLUSTER_DTYPE)), "clusters must be"),
                     (dict(clusters=np.zeros((2, 0), B.CLUSTER_DTYPE)), "number of clusters"),
                     (dict(clusters=np.zeros(65534, B.CLUSTER_DTYPE)), "number of clusters"),
                     (dict(max_iter=-1), "max_iter"), (dict(max_iter=2.5), "max_iter"), (dict(max_iter=True), "max_iter"),
                     (dict(clusters=ok), "ROCm GPU"), (dict(clusters=ok[0]), "ROCm GPU")]:
        with pytest.raises(ValueError, match=word):
            F.slic_tensor(GOOD, StubSlic(20), **kw)
    with pytest.raises(ValueError, match="number of clusters"):
        F.slic_tensor(GOOD, StubSlic(65534))
    with pytest.raises(ValueError, match="debug_mode"):
        F.slic_tensor(GOOD, StubSlic(20, debug_mode=True))
    for slic in (None, 20, B.SlicModel, StubSlic):
        with pytest.raises(ValueError, match="slic must be"):
            F.slic_tensor(GOOD, slic)


def test_iterate_params_is_what_iterate_builds():
    """SlicModel.iterate_params: the options and the variant of the model, field by field."""
    s = StubSlic(20, compactness=7, min_size_factor=0.5, subsample_stride=2, convert_to_lab=False, preemptive=True, preemptive_thres=0.1,
                 manhattan_spatial_dist=False, num_threads=3)
    p = s.slic_model.iterate_params(4, s.compactness, s.min_size_factor, s.subsample_stride)
    got = {n: getattr(p, n) for n, _ in B.Params._fields_ if n != "reserved"}
    assert got == dict(max_iter=4, compactness=7.0, min_size_factor=0.5, subsample_stride=2, convert_to_lab=0, manhattan_spatial_dist=0,
                       preemptive=1, preemptive_thres=pytest.approx(0.1), num_threads=3, debug_mode=0, abi=B.PARAMS_ABI, variant=B.VARIANT_SLIC)
    m = s.slic_model
    m.real_dist = True
    for name, v in (("standard", B.VARIANT_REALDIST), ("l2", B.VARIANT_REALDIST_L2), ("noq", B.VARIANT_REALDIST_NOQ), ("lsc", B.VARIANT_LSC)):
        m.real_dist_type = name
        assert m.iterate_params(1, 10, 0.25, 3).variant == v
    m.real_dist_type = "nope"
    with pytest.raises(RuntimeError):
        m.iterate_params(1, 10, 0.25, 3)


# ---- the header, EXPORTS and the library agree on the new names ----
def test_header_exports_and_library_agree():
    src = open(os.path.join(ROOT, "include", "fslic_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        assert len(re.findall(r"\bint\s+%s\s*\(" % n, src)) == 1, n
        assert B.EXPORTS.count(n) == 1, n
        f = getattr(lib(), n)
        assert f.restype is C.c_int
    assert len(lib().fslic_hip_pack_rgb.argtypes) == 11 and len(lib().fslic_hip_seed_positions.argtypes) == 4
    assert re.search(r"FSLIC_PACK_U8 = 0, FSLIC_PACK_F16 = 1, FSLIC_PACK_BF16 = 2, FSLIC_PACK_F32 = 3", src)
    assert F._SRC_TYPE == {torch.uint8: 0, torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}


def test_the_package_does_not_import_torch():
    import subprocess
    import sys
    code = "import sys, fast_slic_amd; assert 'torch' not in sys.modules; import fast_slic_amd.frames; assert 'torch' in sys.modules"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)
