"""The numpy model of the frame ingest (fast_slic_amd/csrc/ingest.h): every operation is one float32 operation, so the bytes are the
kernel's bytes.  Float16 arrays widen exactly with astype; bfloat16 comes as its 16 bits (uint16) through bf16_bits_to_f32."""
import numpy as np


def bf16_bits_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def to_bytes(x, scale):
    """uint8 array of x's shape: a uint8 x is copied; a float x becomes rint(clamp(float32(x) * float32(scale), 0, 255)), NaN -> 0."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x.copy()
    assert x.dtype in (np.float16, np.float32), x.dtype
    with np.errstate(all="ignore"):
        v = x.astype(np.float32) * np.float32(scale)                  # one rounding
        v = np.where(np.isnan(v), np.float32(0), v)
        v = np.minimum(np.maximum(v, np.float32(0)), np.float32(255))
        v = np.rint(v)                                                # to nearest, ties to even
    assert v.dtype == np.float32
    return v.astype(np.uint8)


def frame_pitch(H, W):
    return (3 * H * W + 15) & ~15


def pack(x, scale, pitch=None):
    """x: [N, 3, H, W] (uint8, float16, float32) -> uint8 [N, pitch]: frame n as [H][W][3] interleaved, then zeros."""
    N, ch, H, W = x.shape
    assert ch == 3
    pitch = frame_pitch(H, W) if pitch is None else pitch
    out = np.zeros((N, pitch), np.uint8)
    out[:, :3 * H * W] = to_bytes(x, scale).transpose(0, 2, 3, 1).reshape(N, 3 * H * W)
    return out
