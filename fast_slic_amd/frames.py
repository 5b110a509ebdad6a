"""Slic on torch tensors: frames and label maps that stay in HBM (csrc/ingest.hip for the frames, the engine's batch entry for the run).

    r = slic_tensor(images, Slic(num_components=1600), max_iter=10)     # images: [N, 3, H, W] float in [0, 1], or uint8 [N, H, W, 3]
    r.labels            # int16 [N, H, W] on the images' GPU, -1 for no label: what Slic.iterate returns, frame by frame
    r.clusters          # CLUSTER_DTYPE [N, K] on the host: the Cluster[K] block of every frame after the run
    r.yxrgb, r.members  # float32 [N, 5, K], int32 [N, K] on the GPU: the clusters as superpixel_crf takes them
    r2 = slic_tensor(next_images, slic, clusters=r.clusters)            # the warm start of a video

    packed, H, W = pack_rgb(images)     # the frames alone: uint8 [N, pitch], frame n = packed[n, :3 H W] read as [H, W, 3]

`images` is [3, H, W] / [N, 3, H, W] (channel-first) or [H, W, 3] / [N, H, W, 3] (channel-last) on a ROCm GPU, uint8, float16, bfloat16 or
float32, of any strides: contiguous, `channels_last`, a crop, a view with a storage offset, a gray plane `expand`ed to three channels.
`channels_first=None` means channel-last for uint8 (the form Slic.iterate takes) and channel-first for floats.  A float element x becomes
the byte rint(clamp(x * scale, 0, 255)) in float32 -- one rounding in the product, ties to even, NaN -> 0; float16 and bfloat16 widen
exactly first -- and a uint8 element is copied (`scale` is ignored).  pitch is 3 H W rounded up to a multiple of 16 and the padding
bytes are 0.  The results are those of Slic.iterate on the same bytes, bit for bit, whatever the batch size.  This module imports torch;
the package itself does not import it.
"""
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import _binding as B, _tensors as T
from .base_slic import BaseSlic

__all__ = ["slic_tensor", "pack_rgb", "SlicFrames"]

_SRC_TYPE = {torch.uint8: 0, torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}      # FSLIC_PACK_*
MAX_COMPONENTS = 65533                                                                    # (SlicModel: num_components < 65534)
_ENTRY = ("fslic_hip_pack_rgb", "frame ingest entry points")


def frame_pitch(H, W):
    """Bytes from one packed frame to the next: 3 H W rounded up to a multiple of 16."""
    return (3 * H * W + 15) & ~15


# ---- argument checks: all of them run before any device work ----
def _check_images(images, channels_first):
    """-> (the images as a [N, 3, H, W] view, batched, channel-first?)."""
    if not isinstance(images, torch.Tensor):
        raise ValueError("images must be a torch tensor")
    if images.dtype not in _SRC_TYPE:
        raise ValueError("images must be uint8, float16, bfloat16 or float32, got %s" % images.dtype)
    if images.dim() not in (3, 4):
        raise ValueError("images must be [3, H, W], [N, 3, H, W], [H, W, 3] or [N, H, W, 3], got shape %s" % (tuple(images.shape),))
    if channels_first is None:
        channels_first = images.dtype != torch.uint8
    elif not isinstance(channels_first, bool):
        raise ValueError("channels_first must be None, True or False")
    batched = images.dim() == 4
    x = images if batched else images.unsqueeze(0)
    if not channels_first:
        x = x.permute(0, 3, 1, 2)
    if x.shape[1] != 3:
        raise ValueError("images must have 3 channels (%s), got shape %s" % ("channel-first" if channels_first else "channel-last", tuple(images.shape)))
    if x.numel() == 0:
        raise ValueError("images must not be empty, got shape %s" % (tuple(images.shape),))
    if x.shape[2] * x.shape[3] >= 1 << 31:
        raise ValueError("H * W must be below 2^31")
    return x, batched, channels_first


def _check_scale(scale):
    if isinstance(scale, bool) or not isinstance(scale, numbers.Real) or not math.isfinite(scale):
        raise ValueError("scale must be a finite real number, got %r" % (scale,))
    return float(scale)


def _check_out(out, N, need):
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != N or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor [N, pitch]")
    if out.shape[1] < need or out.shape[1] % 16:
        raise ValueError("out must be [N, pitch] with pitch >= 3 H W = %d and a multiple of 16, got pitch %d" % (need, out.shape[1]))
    if out.data_ptr() % 4:
        raise ValueError("out must be 4-byte aligned")


def _pack(x, scale, out):
    """x: the [N, 3, H, W] view.  One launch on torch's current stream of x's device."""
    N, _, H, W = x.shape
    strides = (C.c_longlong * 4)(*x.stride())
    B._check(T.library(*_ENTRY).fslic_hip_pack_rgb(x.device.index, T.stream(x.device), N, H, W, x.data_ptr(), _SRC_TYPE[x.dtype], strides,
                                                   C.c_float(scale), out.data_ptr(), out.shape[1]))
    return out


def pack_rgb(images, scale=255.0, channels_first=None, out=None):
    """The frames in the engine's form: (packed, H, W), packed a uint8 tensor [N, pitch] on the images' GPU whose row n holds frame n as
    [H, W, 3] interleaved, then zeros (N = 1 for an unbatched input).  One kernel on torch's current stream, whatever the layout of
    `images`; no host synchronisation, and no allocation but the result's, which `out` ([N, pitch'], contiguous, pitch' >= 3 H W and a
    multiple of 16) replaces."""
    x, _, _ = _check_images(images, channels_first)
    scale = _check_scale(scale)
    N, _, H, W = (int(v) for v in x.shape)
    if out is not None:
        _check_out(out, N, 3 * H * W)
    T.check_device(images, "images")      # (a CPU tensor is the last thing refused)
    if out is not None and out.device != images.device:
        raise ValueError("out must be on the images' device %s, got %s" % (images.device, out.device))
    if out is None:
        out = torch.empty((N, frame_pitch(H, W)), dtype=torch.uint8, device=x.device)
    return _pack(x, scale, out), H, W


def _check_clusters(clusters, N):
    if not isinstance(clusters, np.ndarray) or clusters.dtype != B.CLUSTER_DTYPE:
        raise ValueError("clusters must be a numpy array of CLUSTER_DTYPE")
    if clusters.ndim not in (1, 2) or (clusters.ndim == 2 and clusters.shape[0] != N):
        raise ValueError("clusters must be [K] or [N, K] with N = %d, got shape %s" % (N, clusters.shape))
    return _check_num_components(clusters.shape[-1])


def _check_num_components(K):
    if not 1 <= K <= MAX_COMPONENTS:
        raise ValueError("the number of clusters must be in [1, %d], got %d" % (MAX_COMPONENTS, K))
    return int(K)


class SlicFrames(object):
    """What slic_tensor returns: labels (int16 [N, H, W], or [H, W] for an unbatched input; -1 for no label; on the images' GPU),
    clusters (CLUSTER_DTYPE [N, K], host), num_components, and -- built from the clusters with numpy at the first use, one upload --
    yxrgb (float32 [N, 5, K]) and members (int32 [N, K]) on the GPU: the values SimpleCRF.push_slic_frame reads from the model, in
    the form superpixel_crf takes."""

    def __init__(self, labels, clusters, device):
        self.labels, self.clusters, self.num_components = labels, clusters, int(clusters.shape[1])
        self._device, self._tensors = device, None

    def _cluster_tensors(self):
        if self._tensors is None:
            cl = self.clusters
            N, K = cl.shape
            words = np.empty(N * 6 * K, np.int32)
            words[:N * 5 * K].view(np.float32).reshape(N, 5, K)[...] = np.stack([cl[f] for f in ("y", "x", "r", "g", "b")], axis=1)
            words[N * 5 * K:].view(np.uint32).reshape(N, K)[...] = cl["num_members"]
            dev = torch.from_numpy(words).to(self._device)
            self._tensors = dev[:N * 5 * K].view(torch.float32).view(N, 5, K), dev[N * 5 * K:].view(N, K)
        return self._tensors

    @property
    def yxrgb(self):
        return self._cluster_tensors()[0]

    @property
    def members(self):
        return self._cluster_tensors()[1]


def _seed_clusters(frames, N, H, W, K):
    """The clusters Slic.iterate starts a fresh model with, for every frame: the seed grid once, then the K seed pixels of all frames
    by one gather on the device and one copy of N K 3 bytes to the host.  frames: uint8 [N, >= 3 H W]."""
    seed = np.zeros(K, B.CLUSTER_DTYPE)
    B._check(T.library(*_ENTRY).fslic_hip_seed_positions(H, W, K, seed.ctypes.data))
    base = 3 * (W * seed["y"].astype(np.int64) + seed["x"].astype(np.int64))
    index = torch.from_numpy((base[:, None] + np.arange(3)).reshape(-1)).to(frames.device)
    rgb = frames.index_select(1, index).cpu().numpy().reshape(N, K, 3)
    cl = np.repeat(seed[None], N, axis=0)
    for c, name in enumerate("rgb"):
        cl[name] = rgb[:, :, c]
    return cl


def slic_tensor(images, slic, max_iter=10, clusters=None, scale=255.0, channels_first=None):
    """Slic on `images` (the module docstring has the layouts) -> a SlicFrames; labels and clusters are those of a per-frame
    `slic.iterate` on the same bytes, for every variant.

    slic: a BaseSlic instance (Slic, LSC, SlicRealDist, SlicRealDistL2, SlicRealDistNoQ).  It supplies the options and the variant and is
    not modified: its model's clusters, `initialized` and `last_assignment` stay as they are.  debug_mode is refused (the batch entry
    cannot record).
    clusters: None seeds every frame the way a fresh model is initialised; the K seed pixels are read from the frames on the device, no
    frame goes to the host.  Otherwise a CLUSTER_DTYPE array [K] or [N, K] to start from -- the previous call's `clusters` for the
    frames of a video, like a model kept across iterate calls.  The array is copied, never written.
    Frames: a contiguous uint8 [N, H, W, 3] tensor is used in place (no kernel, no copy); everything else goes through pack_rgb.

    Ordering.  The engine runs on its own streams, so the call synchronises torch's current stream of the images' device once before
    the engine starts: that covers whatever produced `images` on that stream and the pack kernel (work on other streams is the
    caller's to order, as for any torch operation).  Seeding reads the seed pixels back before that.  When the call returns the
    engine has finished: labels and clusters are complete and valid on every stream."""
    x, batched, channels_first = _check_images(images, channels_first)
    scale = _check_scale(scale)
    N, _, H, W = (int(v) for v in x.shape)
    if not isinstance(slic, BaseSlic):
        raise ValueError("slic must be a Slic, LSC, SlicRealDist, SlicRealDistL2 or SlicRealDistNoQ instance")
    model = slic.slic_model
    if model.debug_mode:
        raise ValueError("debug_mode is not supported by slic_tensor: the batch entry cannot record")
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or max_iter < 0:
        raise ValueError("max_iter must be a non-negative integer")
    K = _check_num_components(slic.num_components) if clusters is None else _check_clusters(clusters, N)
    params = model.iterate_params(int(max_iter), slic.compactness, slic.min_size_factor, slic.subsample_stride)
    T.check_device(images, "images")      # (a CPU tensor is the last thing refused)

    dev = x.device
    if x.dtype == torch.uint8 and not channels_first and x.permute(0, 2, 3, 1).is_contiguous():
        frames = x.permute(0, 2, 3, 1).reshape(N, 3 * H * W)      # a view: the caller's bytes, in place
    else:
        frames = _pack(x, scale, torch.empty((N, frame_pitch(H, W)), dtype=torch.uint8, device=dev))
    if clusters is None:
        cl = _seed_clusters(frames, N, H, W, K)
    else:
        cl = np.array(np.broadcast_to(clusters, (N, K)), dtype=B.CLUSTER_DTYPE, order="C", copy=True)
    labels = torch.empty((N, H, W), dtype=torch.int16, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    engine = B.default_engine(dev.index)
    with torch.cuda.device(dev):      # the entry calls hipSetDevice
        engine.iterate_batch([frames.data_ptr() + n * frames.shape[1] for n in range(N)], [cl[n] for n in range(N)],
                             [labels.data_ptr() + n * 2 * H * W for n in range(N)], H, W, params, device_ptrs=True)
    return SlicFrames(labels if batched else labels[0], cl, dev)
