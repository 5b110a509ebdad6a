"""Superpixel pooling and unpooling of float feature maps over a label map, on torch tensors in HBM (csrc/pool.hip).

    v = superpixel_pool(features, labels, num_components, reduce="mean")                 # [C, K] or [N, C, K], float32
    v, counts = superpixel_pool(features, labels, K, reduce="sum", return_counts=True)   # counts: [K] / [N, K] int32
    x = superpixel_unpool(values, labels, fill=0.0)                                      # [C, K] -> [C, H, W]; [N, C, K] -> [N, C, H, W]

`features` is a float32 tensor on a ROCm GPU, channel-first.  `labels` is the int16 map Slic.iterate returns (numpy or torch; -1 means
"no label") or an int32 / int64 torch tensor; labels outside [0, K) are ignored.  The work runs on torch's current stream of the
features' device, without host synchronisation; scratch memory comes from torch's caching allocator.  Results are bitwise reproducible
(no float atomics) and differentiable (sum, mean, max, unpool).  The sum: one f32 partial per tile of 16 x 64 pixels and label; every
partial is truncated towards zero to a multiple of 2^-96 (partials and inputs below 2^-96 vanish; from 2^-73 on nothing is lost), the
truncated partials are added exactly in fixed point and the total is rounded once to f32, ties to even.  A zero total is +0.0; a total
of magnitude 2^128 - 2^103 or more is +-inf; an in-tile partial that overflows f32 leaves its segment's entry unspecified, like an Inf
input.
[C, K] is SimpleCRFFrame's [num_classes, num_nodes]: `v.cpu().numpy()` goes straight into set_proba.  This module imports torch; the
package itself does not import it.
"""
import ctypes as C
import numbers

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _binding as B

__all__ = ["superpixel_pool", "superpixel_unpool"]

_REDUCE = {"sum": 0, "mean": 1, "max": 2}                                  # FSLIC_POOL_*
_LABEL_TYPE = {torch.int16: 0, torch.int32: 1, torch.int64: 2}             # FSLIC_LABEL_*: int16 is read as uint16 (-1 = 0xFFFF)
_NUMPY_LABELS = (np.int16, np.uint16, np.int32, np.int64)
MAX_COMPONENTS = 65534


def _lib():
    lib = B.load_library()
    if not hasattr(lib, "fslic_hip_pool"):
        raise RuntimeError("fast_slic_amd: the loaded library has no pooling entry points; rebuild it")
    return lib


# ---- argument checks: all of them run before any device work ----
def _check_float_map(t, ranks, what, shape_text):
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a torch tensor" % what)
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (what, t.dtype))
    if t.dim() not in ranks:
        raise ValueError("%s must be %s, got shape %s" % (what, shape_text, tuple(t.shape)))
    if t.numel() == 0:
        raise ValueError("%s must not be empty, got shape %s" % (what, tuple(t.shape)))


def _check_labels(labels, shape):
    if isinstance(labels, np.ndarray):
        if labels.dtype.type not in _NUMPY_LABELS:
            raise ValueError("labels must be int16 (Slic.iterate's map), int32 or int64, got %s" % labels.dtype)
    elif isinstance(labels, torch.Tensor):
        if labels.dtype not in _LABEL_TYPE:
            raise ValueError("labels must be int16 (Slic.iterate's map), int32 or int64, got %s" % labels.dtype)
    else:
        raise ValueError("labels must be a numpy array or a torch tensor")
    if tuple(labels.shape) != tuple(shape):
        raise ValueError("labels must have shape %s to match the features, got %s" % (tuple(shape), tuple(labels.shape)))
    H, W = shape[-2:]
    if H * W >= 1 << 31:
        raise ValueError("H * W must be below 2^31")


def _check_num_components(K):
    if isinstance(K, bool) or not isinstance(K, numbers.Integral):
        raise ValueError("num_components must be an integer")
    K = int(K)
    if not 1 <= K <= MAX_COMPONENTS:
        raise ValueError("num_components must be in [1, %d], got %d" % (MAX_COMPONENTS, K))
    return K


def _check_device(t, what):
    if t.device.type != "cuda":
        raise ValueError("%s must be on a ROCm GPU, got device %s (there is no CPU fallback)" % (what, t.device))


def _labels_on(labels, device):
    """Contiguous device tensor of the labels and its FSLIC_LABEL_* code."""
    if isinstance(labels, np.ndarray):
        a = np.ascontiguousarray(labels)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        labels = torch.from_numpy(a)
    lab = labels.to(device=device).contiguous()
    return lab, _LABEL_TYPE[lab.dtype]


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---- the raw calls: [N, C, H, W] / [N, H, W] / [N, C, K], contiguous, on one device ----
def _pool_raw(feat, lab, ltype, K, reduce):
    lib = _lib()
    N, Cc, H, W = feat.shape
    dev = feat.device
    r = _REDUCE[reduce]
    nbytes = C.c_size_t()
    B._check(lib.fslic_hip_pool_workspace_size(N, Cc, K, r, C.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    values = torch.empty((N, Cc, K), dtype=torch.float32, device=dev)
    counts = torch.empty((N, K), dtype=torch.int32, device=dev)
    argmax = torch.empty((N, Cc, K), dtype=torch.int32, device=dev) if reduce == "max" else None
    st = _stream(dev)
    B._check(lib.fslic_hip_pool(dev.index, st, N, Cc, H, W, K, r, feat.data_ptr(), lab.data_ptr(), ltype, ws.data_ptr(), nbytes.value))
    B._check(lib.fslic_hip_pool_finalize(dev.index, st, N, Cc, K, r, ws.data_ptr(), nbytes.value, values.data_ptr(), counts.data_ptr(),
                                         argmax.data_ptr() if argmax is not None else None))
    return values, counts, argmax


def _unpool_raw(values, lab, ltype, H, W, fill, argmax=None):
    lib = _lib()
    N, Cc, K = values.shape
    dev = values.device
    out = torch.empty((N, Cc, H, W), dtype=torch.float32, device=dev)
    B._check(lib.fslic_hip_unpool(dev.index, _stream(dev), N, Cc, H, W, K, values.data_ptr(), lab.data_ptr(), ltype,
                                  argmax.data_ptr() if argmax is not None else None, C.c_float(fill), out.data_ptr()))
    return out


class _Pool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, lab, ltype, K, reduce):
        values, counts, argmax = _pool_raw(feat, lab, ltype, K, reduce)
        ctx.ltype, ctx.reduce, ctx.hw = ltype, reduce, tuple(feat.shape[-2:])
        ctx.save_for_backward(lab, counts, argmax)
        ctx.mark_non_differentiable(counts)
        return values, counts

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_counts):
        lab, counts, argmax = ctx.saved_tensors
        g = g.contiguous()
        H, W = ctx.hw
        if ctx.reduce == "mean":               # unpool(g / count); an empty segment reaches no pixel
            g = g / counts.clamp_min(1).to(torch.float32).unsqueeze(1)
        gin = _unpool_raw(g, lab, ctx.ltype, H, W, 0.0, argmax if ctx.reduce == "max" else None)
        return gin, None, None, None, None


class _Unpool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, lab, ltype, H, W, fill):
        ctx.ltype, ctx.K = ltype, values.shape[-1]
        ctx.save_for_backward(lab)
        return _unpool_raw(values, lab, ltype, H, W, fill)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lab, = ctx.saved_tensors
        gv, _, _ = _pool_raw(g.contiguous(), lab, ctx.ltype, ctx.K, "sum")
        return gv, None, None, None, None, None


def superpixel_pool(features, labels, num_components, reduce="mean", return_counts=False):
    """Pool `features` ([C, H, W] or [N, C, H, W], float32 on a ROCm GPU) over `labels` ([H, W] / [N, H, W]) into [C, K] / [N, C, K].

    reduce: "sum"; "mean" (the sum divided by the count in f32, 0 for an empty segment); "max" (exact, -0.0 below +0.0, 0 for an
    empty segment; the gradient goes to the lowest flat index h * W + w holding the maximum).  With return_counts also the pixels
    per segment, int32 [K] / [N, K].  NaN or Inf in a segment leave that segment's entries unspecified and no other."""
    _check_float_map(features, (3, 4), "features", "[C, H, W] or [N, C, H, W]")
    batched = features.dim() == 4
    H, W = features.shape[-2:]
    _check_labels(labels, (features.shape[0], H, W) if batched else (H, W))
    K = _check_num_components(num_components)
    if reduce not in _REDUCE:
        raise ValueError("reduce must be one of %s, got %r" % (sorted(_REDUCE), reduce))
    _check_device(features, "features")
    lab, ltype = _labels_on(labels, features.device)
    feat = (features if batched else features.unsqueeze(0)).contiguous()
    values, counts = _Pool.apply(feat, lab if batched else lab.unsqueeze(0), ltype, K, reduce)
    if not batched:
        values, counts = values.squeeze(0), counts.squeeze(0)
    return (values, counts) if return_counts else values


def superpixel_unpool(values, labels, fill=0.0):
    """Broadcast per-segment values ([C, K] / [N, C, K], float32 on a ROCm GPU) to the pixels of `labels` ([H, W] / [N, H, W]):
    out[..., c, h, w] = values[..., c, labels[..., h, w]], `fill` where the label is not in [0, K).  Exact; differentiable (the
    gradient is the sum-pool of the incoming gradient)."""
    _check_float_map(values, (2, 3), "values", "[C, K] or [N, C, K]")
    batched = values.dim() == 3
    if not isinstance(labels, (np.ndarray, torch.Tensor)) or labels.ndim != values.dim():
        raise ValueError("labels must be [H, W] for [C, K] values and [N, H, W] for [N, C, K] values")
    H, W = labels.shape[-2:]
    _check_labels(labels, (values.shape[0], H, W) if batched else (H, W))
    if H == 0 or W == 0:
        raise ValueError("labels must not be empty")
    _check_num_components(values.shape[-1])
    if isinstance(fill, bool) or not isinstance(fill, numbers.Real):
        raise ValueError("fill must be a real number")
    _check_device(values, "values")
    lab, ltype = _labels_on(labels, values.device)
    vals = (values if batched else values.unsqueeze(0)).contiguous()
    out = _Unpool.apply(vals, lab if batched else lab.unsqueeze(0), ltype, int(H), int(W), float(fill))
    return out if batched else out.squeeze(0)
