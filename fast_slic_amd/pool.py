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

from . import _binding as B, _tensors as T
from ._tensors import MAX_COMPONENTS      # (public here: the largest num_components)

__all__ = ["superpixel_pool", "superpixel_unpool"]

_REDUCE = {"sum": 0, "mean": 1, "max": 2}                                  # FSLIC_POOL_*
_ENTRY = ("fslic_hip_pool", "pooling entry points")


# ---- argument checks: all of them run before any device work ----
def _check_labels(labels, shape):
    if isinstance(labels, np.ndarray):
        if labels.dtype.type not in T.NUMPY_LABELS:
            raise ValueError("labels must be int16 (Slic.iterate's map), int32 or int64, got %s" % labels.dtype)
    elif isinstance(labels, torch.Tensor):
        if labels.dtype not in T.LABEL_TYPE:
            raise ValueError("labels must be int16 (Slic.iterate's map), int32 or int64, got %s" % labels.dtype)
    else:
        raise ValueError("labels must be a numpy array or a torch tensor")
    if tuple(labels.shape) != tuple(shape):
        raise ValueError("labels must have shape %s to match the features, got %s" % (tuple(shape), tuple(labels.shape)))
    H, W = shape[-2:]
    if H * W >= 1 << 31:
        raise ValueError("H * W must be below 2^31")


# ---- the raw calls: [N, C, H, W] / [N, H, W] / [N, C, K], contiguous, on one device ----
def _pool_raw(feat, lab, ltype, K, reduce):
    lib = T.library(*_ENTRY)
    N, Cc, H, W = feat.shape
    dev = feat.device
    r = _REDUCE[reduce]
    ws, nbytes = T.scratch(dev, lib.fslic_hip_pool_workspace_size, N, Cc, K, r)
    values = torch.empty((N, Cc, K), dtype=torch.float32, device=dev)
    counts = torch.empty((N, K), dtype=torch.int32, device=dev)
    argmax = torch.empty((N, Cc, K), dtype=torch.int32, device=dev) if reduce == "max" else None
    st = T.stream(dev)
    B._check(lib.fslic_hip_pool(dev.index, st, N, Cc, H, W, K, r, feat.data_ptr(), lab.data_ptr(), ltype, ws.data_ptr(), nbytes))
    B._check(lib.fslic_hip_pool_finalize(dev.index, st, N, Cc, K, r, ws.data_ptr(), nbytes, values.data_ptr(), counts.data_ptr(),
                                         T.ptr(argmax)))
    return values, counts, argmax


def _unpool_raw(values, lab, ltype, H, W, fill, argmax=None):
    lib = T.library(*_ENTRY)
    N, Cc, K = values.shape
    dev = values.device
    out = torch.empty((N, Cc, H, W), dtype=torch.float32, device=dev)
    B._check(lib.fslic_hip_unpool(dev.index, T.stream(dev), N, Cc, H, W, K, values.data_ptr(), lab.data_ptr(), ltype, T.ptr(argmax),
                                  C.c_float(fill), out.data_ptr()))
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
    T.check_float_map(features, (3, 4), "features", "[C, H, W] or [N, C, H, W]")
    batched = features.dim() == 4
    H, W = features.shape[-2:]
    _check_labels(labels, (features.shape[0], H, W) if batched else (H, W))
    K = T.check_count(num_components, "num_components")
    if reduce not in _REDUCE:
        raise ValueError("reduce must be one of %s, got %r" % (sorted(_REDUCE), reduce))
    T.check_device(features, "features")
    lab, ltype = T.labels_on(labels, features.device, batched)
    values, counts = _Pool.apply(T.batch_of(features, batched), lab, ltype, K, reduce)
    if not batched:
        values, counts = values.squeeze(0), counts.squeeze(0)
    return (values, counts) if return_counts else values


def superpixel_unpool(values, labels, fill=0.0):
    """Broadcast per-segment values ([C, K] / [N, C, K], float32 on a ROCm GPU) to the pixels of `labels` ([H, W] / [N, H, W]):
    out[..., c, h, w] = values[..., c, labels[..., h, w]], `fill` where the label is not in [0, K).  Exact; differentiable (the
    gradient is the sum-pool of the incoming gradient)."""
    T.check_float_map(values, (2, 3), "values", "[C, K] or [N, C, K]")
    batched = values.dim() == 3
    if not isinstance(labels, (np.ndarray, torch.Tensor)) or labels.ndim != values.dim():
        raise ValueError("labels must be [H, W] for [C, K] values and [N, H, W] for [N, C, K] values")
    H, W = labels.shape[-2:]
    _check_labels(labels, (values.shape[0], H, W) if batched else (H, W))
    if H == 0 or W == 0:
        raise ValueError("labels must not be empty")
    T.check_count(values.shape[-1], "num_components")
    if isinstance(fill, bool) or not isinstance(fill, numbers.Real):
        raise ValueError("fill must be a real number")
    T.check_device(values, "values")
    lab, ltype = T.labels_on(labels, values.device, batched)
    out = _Unpool.apply(T.batch_of(values, batched), lab, ltype, int(H), int(W), float(fill))
    return out if batched else out.squeeze(0)
