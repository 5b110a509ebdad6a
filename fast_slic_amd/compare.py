"""Two label maps of one shape against each other, on torch tensors in HBM (csrc/compare.hip).

    t = label_overlap(labels, other, num_components, num_other)
    t.pairs      # int64 [2, P]: every (a, b) = (labels[p], other[p]) that shares a pixel, once; sorted by (frame, a, b)
    t.count      # int32 [P]: the pixels of that pair
    t.offsets    # int64 [N + 1]: the pairs of frame n are [offsets[n], offsets[n + 1]); N = 1 for an [H, W] map
    t.areas()                     # (int64 [N, K], int64 [N, M]): the valid pixels of every a and of every b
    t.majority()                  # int64 [N, K]: the b that covers most of a (the smallest such b), -1 for an a without a pixel
    t.best_overlap()              # float64 [N]: sum_a max_b n_ab / n; the achievable segmentation accuracy when other is ground truth
    t.undersegmentation_error()   # float64 [N]: (1 / n) sum_b sum_{a: n_ab > 0} min(n_ab, |a| - n_ab) (Neubert and Protzel)
    m = boundary_match(labels, other, tolerance=0)      # int64 [N, 3]: hits, boundary pixels of other, boundary pixels of labels

`labels` and `other` are int16 maps as Slic.iterate returns them (numpy or torch; -1 means "no label") or int32 / int64 maps, [H, W]
or [N, H, W], of one shape; their types may differ.  In the overlap table a pixel takes part when 0 <= labels[p] < K and
0 <= other[p] < M.  A boundary pixel is one whose value differs from its right or its lower neighbour's (values as stored, no K);
`hits` counts the boundary pixels of `other` with a boundary pixel of `labels` within Chebyshev distance `tolerance`: hits /
other's boundary pixels is the boundary recall, the swapped call gives the precision, and at tolerance 0 hits / (both - hits) is
the boundary IoU.  All of it is integer arithmetic: results are exact and bitwise reproducible.  Unbatched input drops the leading N
of every result.  This module imports torch; the package itself does not import it.
"""
import numbers

import torch

from . import _binding as B, _pairtable as PT, _tensors as T

__all__ = ["label_overlap", "boundary_match", "OverlapTable"]

MAX_TOLERANCE = 15


_ENTRY = ("fslic_hip_overlap_accumulate", "label map comparison entry points")


def first_capacity(K, M):
    """Slots per frame of the first pair table: a segment of one Slic-like map meets a handful of the other's, and the table stays
    under half load."""
    return max(1024, PT.pow2_at_least(16 * max(K, M)))


def capacity_limit(K, M, H, W):
    """Slots per frame that hold any two maps of this shape at half load: no more distinct pairs than label pairs or pixels."""
    return min(PT.MAX_CAPACITY, max(first_capacity(K, M), PT.pow2_at_least(2 * min(K * M, H * W))))


class OverlapTable(object):
    """What label_overlap returns: pairs, count, offsets (torch tensors on the labels' GPU), num_components, num_other, and capacity,
    the slots per frame of the pair table that held the result (it has no influence on the result).  The methods are torch integer
    operations on the table (scatter_reduce with amax, index_add_): independent of the order, hence exact; they launch no kernel of
    this library and do not synchronise the host."""

    def __init__(self, pairs, count, offsets, num_components, num_other, capacity, batched=True):
        self.pairs, self.count, self.offsets = pairs, count, offsets
        self.num_components, self.num_other, self.capacity = num_components, num_other, capacity
        self._batched = batched

    @property
    def num_frames(self):
        return self.offsets.shape[0] - 1

    def _rows(self):
        """(frame * K + a, frame * M + b, frame, count as int64) of every pair."""
        P, dev = self.pairs.shape[1], self.pairs.device
        # the frame of pair i: how many frames end at or before i
        frame = torch.searchsorted(self.offsets[1:].contiguous(), torch.arange(P, dtype=torch.int64, device=dev), right=True)
        return frame * self.num_components + self.pairs[0], frame * self.num_other + self.pairs[1], frame, self.count.to(torch.int64)

    def _out(self, t):
        return t if self._batched else t.squeeze(0)

    def _zeros(self, *shape):
        return torch.zeros(shape, dtype=torch.int64, device=self.pairs.device)

    def areas(self):
        """(int64 [N, K], int64 [N, M]): the pixels of every label of `labels` and of `other` among the pixels that take part."""
        N, K, M = self.num_frames, self.num_components, self.num_other
        ra, rb, _, cnt = self._rows()
        return (self._out(self._zeros(N * K).index_add_(0, ra, cnt).view(N, K)),
                self._out(self._zeros(N * M).index_add_(0, rb, cnt).view(N, M)))

    def majority(self):
        """int64 [N, K]: for every label a the label b of `other` that covers most of its pixels, the smallest such b on a tie; -1
        for an a without a pixel that takes part."""
        N, K = self.num_frames, self.num_components
        ra, _, _, cnt = self._rows()
        best = torch.full((N * K,), -1, dtype=torch.int64, device=self.pairs.device)
        best.scatter_reduce_(0, ra, cnt * 65536 + (65535 - self.pairs[1]), "amax", include_self=True)     # count first, then the smaller b
        return self._out(torch.where(best < 0, best, 65535 - (best & 65535)).view(N, K))

    def _totals(self, frame, cnt):
        return self._zeros(self.num_frames).index_add_(0, frame, cnt)

    def best_overlap(self):
        """float64 [N]: the fraction of the pixels whose segment of `labels` lies in the segment of `other` that it overlaps most,
        sum_a max_b n_ab / sum n_ab: one float64 division of two integers.  NaN for a frame without a pixel that takes part."""
        N, K = self.num_frames, self.num_components
        ra, _, frame, cnt = self._rows()
        best = self._zeros(N * K).scatter_reduce_(0, ra, cnt, "amax", include_self=True).view(N, K).sum(1)
        return self._out(best.to(torch.float64) / self._totals(frame, cnt).to(torch.float64))

    def undersegmentation_error(self):
        """float64 [N]: (1 / n) sum_b sum_{a: n_ab > 0} min(n_ab, |a| - n_ab) with |a| = sum_b n_ab and n = sum n_ab (Neubert and
        Protzel): what of every segment a leaks out of the segments b it touches, or, where that is less, what lies inside.  One
        float64 division of two integers; NaN for a frame without a pixel that takes part."""
        N, K = self.num_frames, self.num_components
        ra, _, frame, cnt = self._rows()
        area = self._zeros(N * K).index_add_(0, ra, cnt)
        leak = self._zeros(N).index_add_(0, frame, torch.minimum(cnt, area[ra] - cnt))
        return self._out(leak.to(torch.float64) / self._totals(frame, cnt).to(torch.float64))


# ---- argument checks: all of them run before any device work ----
def _check_maps(labels, other):
    T.check_label_map(labels, "labels")
    T.check_label_map(other, "other")
    if tuple(other.shape) != tuple(labels.shape):
        raise ValueError("other must have shape %s to match the labels, got %s" % (tuple(labels.shape), tuple(other.shape)))
    H, W = (int(v) for v in labels.shape[-2:])
    if H * W >= 1 << 31:
        raise ValueError("H * W must be below 2^31")
    return H, W


def label_overlap(labels, other, num_components, num_other, *, device=None, _start_capacity=None):
    """The overlap table of `labels` and `other` ([H, W] or [N, H, W] of one shape; int16, int32 or int64, not necessarily the same;
    numpy or torch) as an OverlapTable: every pair (a, b) with 0 <= a < num_components and 0 <= b < num_other that shares a pixel,
    and its pixels.  A label outside its range, decided on the value at its own width, takes its pixel out of the table.

    Torch tensors must be on one ROCm GPU, which is where the result lives; numpy arrays are uploaded to it (to `device`, or torch's
    current GPU, when nothing else names one).  The work runs on torch's current stream of that device and scratch memory comes from
    torch's caching allocator.  The number of pairs decides the shape of the result, so a call synchronises the host once; it
    synchronises again only when the pair table has to grow: the first table has a power of two >= 16 max(K, M) slots per frame (at
    least 1024); two maps with more distinct pairs than half of that (noise) double it and start over, up to a table that holds
    min(K M, H W) pairs.  The result does not depend on the table's size.  `_start_capacity` (testing) sets the first table's slots
    per frame."""
    H, W = _check_maps(labels, other)
    K = T.check_count(num_components, "num_components")
    M = T.check_count(num_other, "num_other")
    capacity, limit = PT.start_capacity(first_capacity(K, M), capacity_limit(K, M, H, W), _start_capacity)
    dev = T.one_device(((labels, "labels"), (other, "other")), device)

    lib = T.library(*_ENTRY)
    batched = labels.ndim == 3
    (lab, ltype), (oth, otype) = T.labels_on(labels, dev, batched), T.labels_on(other, dev, batched)
    N = lab.shape[0]

    def accumulate(capacity):
        ws, nbytes = T.scratch(dev, lib.fslic_hip_overlap_workspace_size, N, capacity)
        B._check(lib.fslic_hip_overlap_accumulate(dev.index, T.stream(dev), N, H, W, K, M, lab.data_ptr(), ltype, oth.data_ptr(), otype,
                                                  capacity, ws.data_ptr(), nbytes))
        return ws, nbytes

    def compact(ws, nbytes, capacity, P, keys, count):
        B._check(lib.fslic_hip_overlap_compact(dev.index, T.stream(dev), N, capacity, ws.data_ptr(), nbytes, keys.data_ptr(),
                                               count.data_ptr(), P))

    with torch.cuda.device(dev):
        pairs, count, _, offsets, capacity = PT.run(accumulate, compact, N, capacity, limit, dev)
    return OverlapTable(pairs, count, offsets, K, M, capacity, batched)


def boundary_match(labels, other, tolerance=0, *, device=None):
    """int64 [N, 3] ([3] for [H, W] maps) on the maps' GPU: (hits, boundary pixels of other, boundary pixels of labels), where hits
    counts the boundary pixels of `other` that have a boundary pixel of `labels` within Chebyshev distance `tolerance` (an integer in
    [0, 15]).  No host synchronisation; the work runs on torch's current stream of the device."""
    H, W = _check_maps(labels, other)
    if isinstance(tolerance, bool) or not isinstance(tolerance, numbers.Integral) or not 0 <= int(tolerance) <= MAX_TOLERANCE:
        raise ValueError("tolerance must be an integer in [0, %d], got %r" % (MAX_TOLERANCE, tolerance))
    dev = T.one_device(((labels, "labels"), (other, "other")), device)

    lib = T.library(*_ENTRY)
    batched = labels.ndim == 3
    (lab, ltype), (oth, otype) = T.labels_on(labels, dev, batched), T.labels_on(other, dev, batched)
    N = lab.shape[0]
    with torch.cuda.device(dev):
        out = torch.empty((N, 3), dtype=torch.int64, device=dev)
        B._check(lib.fslic_hip_boundary_match(dev.index, T.stream(dev), N, H, W, lab.data_ptr(), ltype, oth.data_ptr(), otype,
                                              int(tolerance), out.data_ptr()))
    return out if batched else out[0]
