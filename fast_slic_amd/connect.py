"""Connectivity on label tensors in HBM: the connected components of a label map, and the merge of the components below a minimum
area that makes a label map a superpixel map (csrc/connect.hip).

    comp, n = connected_components(labels)            # int32 [N, H, W] (or [H, W]), n: int32 [N] (or 0-dim)
    out,  n = enforce_connectivity(labels, min_size)  # int32 [N, H, W] with labels 0 .. n-1, n: int32 [N]

`labels` is [H, W] or [N, H, W], int16, int32 or int64, a torch tensor on a ROCm GPU or a numpy array, which is uploaded (to `device`,
or torch's current GPU, when nothing else names one).  Label values are compared for equality only, at their own width: any value is
allowed, and a region of -1 is a label like any other (as 0xFFFF is in the reference).  N * H * W must be below 2^31.  `min_size` is a
non-negative Python integer.  The rules are the reference's ConnectivityEnforcer::execute (src/cca.cpp:178-265) with its cut at K
labels never binding:

1. Components.  Components are the 4-connected sets of equal labels.  A component's *leader* is its first pixel in raster order.
   Components are numbered 0, 1, 2, ... in ascending leader order.  connected_components returns this number per pixel, and the
   number of components per frame.
2. Kept components.  A component is *kept* if its area is >= min_size.  Kept components receive the labels 0, 1, 2, ... in ascending
   leader order.
3. Component 0.  If component 0 (the one holding pixel (0, 0)) is not kept, it takes label 0.
4. Other unkept components.  Every other component that is not kept takes the final label of a neighbouring component: the component
   of the pixel left of its leader, or, for a leader in column 0, of the pixel above.  That component may itself not be kept; the rule
   then applies again.  Leaders strictly decrease along this chain, so it ends at a kept component or at component 0.
5. Count.  n is the number of kept components, or 1 when there are none.  The labels 0 .. n-1 all occur.  For min_size >= 1,
   n <= H * W // min_size: the bound a caller passes on as `num_components` (superpixel_pool, superpixel_graph, ...) without reading
   n back.

There is no `max_components` cap: the engine's uint16 host entry (fast_slic_amd.enforce_connectivity) keeps that and its tie rule.
There is no 8-connectivity, and nothing here is differentiable.

The work runs on torch's current stream of the map's device, without host synchronisation, without a copy to the host and without a
host path for any input; scratch memory (8 bytes per pixel) comes from torch's caching allocator.  The input is not modified.  All of
it is integer arithmetic: results are exact and identical from run to run.  Unbatched input drops the leading N of every result.
This module imports torch; the package itself does not import it.
"""
import numbers

import torch

from . import _binding as B, _tensors as T

__all__ = ["connected_components", "enforce_connectivity"]


# ---- argument checks: all of them run before any device work ----
def _check_map(labels):
    T.check_label_map(labels, "labels")
    total = 1
    for v in labels.shape:
        total *= int(v)
    if total >= 1 << 31:
        raise ValueError("N * H * W must be below 2^31, got shape %s" % (tuple(labels.shape),))


def _check_min_size(min_size):
    if isinstance(min_size, bool) or not isinstance(min_size, numbers.Integral):
        raise ValueError("min_size must be an integer, got %r" % (min_size,))
    if int(min_size) < 0:
        raise ValueError("min_size must be >= 0, got %d" % int(min_size))
    return min(int(min_size), 1 << 31)               # (above H * W nothing is kept, whatever the value)


def _run(labels, device, min_size):
    """min_size None: the components."""
    _check_map(labels)
    if min_size is not None:
        min_size = _check_min_size(min_size)
    dev = T.one_device(((labels, "labels"),), device)

    lib = T.library("fslic_hip_connect_enforce", "connectivity entry points for label tensors")
    batched = labels.ndim == 3
    lab, ltype = T.labels_on(labels, dev, batched)
    N, H, W = (int(v) for v in lab.shape)
    with torch.cuda.device(dev):
        ws, nbytes = T.scratch(dev, lib.fslic_hip_connect_workspace_size, N, H, W)
        out = torch.empty((N, H, W), dtype=torch.int32, device=dev)
        n = torch.empty((N,), dtype=torch.int32, device=dev)
        head = (dev.index, T.stream(dev), N, H, W, lab.data_ptr(), ltype)
        if min_size is None:
            B._check(lib.fslic_hip_connected_components(*head, out.data_ptr(), n.data_ptr(), ws.data_ptr(), nbytes))
        else:
            B._check(lib.fslic_hip_connect_enforce(*head, min_size, out.data_ptr(), n.data_ptr(), ws.data_ptr(), nbytes))
    return (out, n) if batched else (out[0], n[0])


def connected_components(labels, *, device=None):
    """(comp, n): comp int32, of the shape of `labels`, the number of every pixel's component (rule 1 of the module's text); n int32
    [N] (0-dim for an [H, W] map) the components of every frame: comp's maximum + 1."""
    return _run(labels, device, None)


def enforce_connectivity(labels, min_size, *, device=None):
    """(out, n): out int32, of the shape of `labels`, the labels after the merge of every component below `min_size` pixels (rules 2 to
    4 of the module's text); n int32 [N] (0-dim for an [H, W] map) the labels of every frame: 0 .. n-1 all occur, and n <= H * W //
    min_size for min_size >= 1."""
    if min_size is None:
        raise ValueError("min_size must be an integer, got None")
    return _run(labels, device, min_size)
