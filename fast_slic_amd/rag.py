"""The region adjacency graph of a label map, on torch tensors in HBM (csrc/rag.hip).

    g = superpixel_graph(labels, num_components, connectivity=4, image=None)
    g.edge_index   # int64 [2, E]: every pair of labels that touch, once; row 0 < row 1; sorted by (frame, row 0, row 1)
    g.boundary     # int32 [E]: the number of neighbouring pixel pairs {p, q} whose labels are {a, b}
    g.contrast     # int64 [E, C]: the sum over those pixel pairs of |image[p, c] - image[q, c]|; None without an image
    g.offsets      # int64 [N + 1]: the edges of frame n are [offsets[n], offsets[n + 1]); N = 1 for an [H, W] map
    g.to_csr(frame=0)   # (offsets int64 [K + 1], indices int32): symmetric neighbour lists, every row ascending

`labels` is the int16 map Slic.iterate returns (numpy or torch; -1 means "no label") or an int32 / int64 map, [H, W] or [N, H, W];
a pixel whose label is outside [0, K) takes part in no pair.  connectivity 4 looks at every pixel's right and down neighbour, 8 also
at down-right and down-left: every unordered pixel pair of the whole plane exactly once, the last row and column included (unlike
SlicModel.get_connectivity, which reproduces the reference's scan and its cap of 12 neighbours).  All of it is integer arithmetic:
results are exact and bitwise reproducible.  This module imports torch; the package itself does not import it.
"""
import ctypes as C

import numpy as np
import torch

from . import _binding as B
from .pool import _check_device, _check_labels, _check_num_components, _labels_on, _stream

__all__ = ["superpixel_graph", "SuperpixelGraph"]

MAX_CHANNELS = 4
_HEADER_FIXED = 16          # bytes of the workspace header before the per-frame pair counts (csrc/rag.h)
_MIN_CAPACITY, _MAX_CAPACITY = 64, 1 << 31


def _lib():
    lib = B.load_library()
    if not hasattr(lib, "fslic_hip_rag_accumulate"):
        raise RuntimeError("fast_slic_amd: the loaded library has no region adjacency graph entry points; rebuild it")
    return lib


def _pow2_at_least(v):
    return 1 << max(0, int(v) - 1).bit_length()


def first_capacity(K):
    """Slots per frame of the first pair table: sized for a planar map (a Slic map has about 2.9 K edges), under half load."""
    return max(1024, _pow2_at_least(8 * K))


def capacity_limit(K, H, W, connectivity):
    """Slots per frame that hold any map of this shape at half load: no more distinct pairs than label pairs or pixel pairs."""
    pairs = min(K * (K - 1) // 2, (connectivity // 2) * H * W)
    return min(_MAX_CAPACITY, max(first_capacity(K), _pow2_at_least(2 * pairs)))


class SuperpixelGraph(object):
    """What superpixel_graph returns: edge_index, boundary, contrast, offsets (torch tensors on the labels' GPU), num_components,
    and capacity, the slots per frame of the pair table that held the result (it has no influence on the result)."""

    def __init__(self, edge_index, boundary, contrast, offsets, num_components, capacity):
        self.edge_index, self.boundary, self.contrast, self.offsets = edge_index, boundary, contrast, offsets
        self.num_components, self.capacity = num_components, capacity

    @property
    def num_frames(self):
        return self.offsets.shape[0] - 1

    def to_csr(self, frame=0):
        """The neighbour lists of one frame: (offsets int64 [K + 1], indices int32); node k's neighbours are
        indices[offsets[k]:offsets[k + 1]], ascending, and b is in a's list exactly when a is in b's."""
        if isinstance(frame, bool) or not isinstance(frame, int) or not 0 <= frame < self.num_frames:
            raise ValueError("frame must be an integer in [0, %d)" % self.num_frames)
        K = self.num_components
        e = self.edge_index[:, self.offsets[frame]:self.offsets[frame + 1]]
        flat = torch.cat([e[0] * K + e[1], e[1] * K + e[0]]).sort().values      # unique keys: any sort gives this order
        rows = torch.div(flat, K, rounding_mode="floor")
        offsets = torch.zeros(K + 1, dtype=torch.int64, device=flat.device)
        offsets[1:] = torch.bincount(rows, minlength=K).cumsum(0)
        return offsets, (flat - rows * K).to(torch.int32)

    def to_batch_csr(self):
        """The neighbour lists of every frame as one CSR over (frame, node): (offsets int64 [N * K + 1], indices int32 [2 E]); the
        neighbours of node k of frame n are indices[offsets[n * K + k]:offsets[n * K + k + 1]], node numbers inside the frame,
        ascending and symmetric: the concatenation of to_csr(n) over the frames with the offsets shifted.  Unlike to_csr, which
        slices by offsets[frame], it does not synchronise the host."""
        K, N, E = self.num_components, self.num_frames, self.edge_index.shape[1]
        dev = self.edge_index.device
        # the frame of edge e: how many frames end at or before e
        frame = torch.searchsorted(self.offsets[1:].contiguous(), torch.arange(E, dtype=torch.int64, device=dev), right=True)
        a, b = self.edge_index[0], self.edge_index[1]
        # key = (row over (frame, node)) * K + neighbour; unique, so any sort gives this order
        flat = torch.cat([(frame * K + a) * K + b, (frame * K + b) * K + a]).sort().values
        rows = torch.div(flat, K, rounding_mode="floor")
        # offsets[r] = the entries of the rows before r (bincount would read its size back from the device)
        offsets = torch.searchsorted(rows, torch.arange(N * K + 1, dtype=torch.int64, device=dev))
        return offsets, (flat - rows * K).to(torch.int32)


# ---- argument checks: all of them run before any device work ----
def _check_image(image, shape):
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise ValueError("image must be uint8, got %s" % image.dtype)
    elif isinstance(image, torch.Tensor):
        if image.dtype != torch.uint8:
            raise ValueError("image must be uint8, got %s" % image.dtype)
    else:
        raise ValueError("image must be a numpy array or a torch tensor")
    if image.ndim != len(shape) + 1 or tuple(image.shape[:-1]) != tuple(shape):
        raise ValueError("image must have shape %s + (C,), channel-last, to match the labels, got %s" % (tuple(shape), tuple(image.shape)))
    if not 1 <= image.shape[-1] <= MAX_CHANNELS:
        raise ValueError("image must have 1 to %d channels, got C = %d" % (MAX_CHANNELS, image.shape[-1]))


def _pick_device(labels, image, device):
    """The GPU of the result.  Torch tensors must already be there (and on the same one); numpy arrays are uploaded."""
    given = [(t, what) for t, what in ((labels, "labels"), (image, "image")) if isinstance(t, torch.Tensor)]
    for t, what in given:
        _check_device(t, what)
    devs = {t.device for t, _ in given}
    if device is not None:
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("device must be a ROCm GPU, got %s (there is no CPU fallback)" % device)
        if device.index is not None:
            devs.add(device)
    if len(devs) > 1:
        raise ValueError("labels, image and device must name one GPU, got %s" % sorted(str(d) for d in devs))
    if devs:
        return devs.pop()
    return torch.device("cuda", torch.cuda.current_device())


def _accumulate(lib, lab, ltype, img, K, connectivity, capacity):
    """One pass at the given capacity -> (workspace, its bytes, the header on the host).  Synchronises the host."""
    N, H, W = lab.shape
    Cc = img.shape[-1] if img is not None else 0
    dev = lab.device
    nbytes = C.c_size_t()
    B._check(lib.fslic_hip_rag_workspace_size(N, K, Cc, capacity, C.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    B._check(lib.fslic_hip_rag_accumulate(dev.index, _stream(dev), N, H, W, K, connectivity, lab.data_ptr(), ltype,
                                          img.data_ptr() if img is not None else None, Cc, capacity, ws.data_ptr(), nbytes.value))
    header = ws[:_HEADER_FIXED + 4 * N].cpu().numpy().view(np.uint32)
    return ws, nbytes.value, header


def superpixel_graph(labels, num_components, connectivity=4, image=None, *, device=None, _start_capacity=None):
    """The region adjacency graph of `labels` ([H, W] or [N, H, W]; int16, int32 or int64; numpy or torch) as a SuperpixelGraph.

    image: optional uint8 [H, W, C] / [N, H, W, C], channel-last as Slic.iterate takes it, C in 1 .. 4 (numpy or torch): adds
    `contrast`.  Torch tensors must be on one ROCm GPU, which is where the result lives; numpy arrays are uploaded to it (to `device`,
    or torch's current GPU, when nothing else names one).

    The work runs on torch's current stream of that device and scratch memory comes from torch's caching allocator.  The number of
    edges decides the shape of the result, so a call synchronises the host once; it synchronises again only when the pair table has to
    grow: the first table has a power of two >= 8 K slots per frame (at least 1024), which holds any planar map; a map with more
    distinct pairs (a noise map) doubles it and starts over, up to a table that holds every possible pair.  The result does not
    depend on the table's size.  `_start_capacity` (testing) sets the first table's slots per frame."""
    if not isinstance(labels, (np.ndarray, torch.Tensor)):
        raise ValueError("labels must be a numpy array or a torch tensor")
    if labels.ndim not in (2, 3):
        raise ValueError("labels must be [H, W] or [N, H, W], got shape %s" % (tuple(labels.shape),))
    if 0 in labels.shape:
        raise ValueError("labels must not be empty, got shape %s" % (tuple(labels.shape),))
    _check_labels(labels, labels.shape)
    H, W = (int(v) for v in labels.shape[-2:])
    if H * W >= 1 << 29:
        raise ValueError("H * W must be below 2^29")
    K = _check_num_components(num_components)
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))
    connectivity = int(connectivity)
    if image is not None:
        _check_image(image, labels.shape)
    limit = capacity_limit(K, H, W, connectivity)
    capacity = first_capacity(K)
    if _start_capacity is not None:
        capacity = _start_capacity
        if isinstance(capacity, bool) or not isinstance(capacity, int) or not _MIN_CAPACITY <= capacity <= _MAX_CAPACITY \
                or capacity & (capacity - 1):
            raise ValueError("_start_capacity must be a power of two in [%d, 2^31]" % _MIN_CAPACITY)
        limit = max(limit, capacity)
    dev = _pick_device(labels, image, device)

    lib = _lib()
    batched = labels.ndim == 3
    lab, ltype = _labels_on(labels, dev)
    if not batched:
        lab = lab.unsqueeze(0)
    img = None
    if image is not None:
        img = (torch.from_numpy(np.ascontiguousarray(image)) if isinstance(image, np.ndarray) else image).to(device=dev).contiguous()
        if not batched:
            img = img.unsqueeze(0)
    N = lab.shape[0]
    Cc = img.shape[-1] if img is not None else 0
    with torch.cuda.device(dev):
        while True:
            ws, nbytes, header = _accumulate(lib, lab, ltype, img, K, connectivity, capacity)
            if header[0] == 0:
                break
            del ws
            if capacity >= limit:
                raise RuntimeError("fast_slic_amd: the pair table overflowed at its largest size (%d slots per frame)" % capacity)
            capacity *= 2
        E = int(header[_HEADER_FIXED // 4:].sum(dtype=np.int64))
        offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        offsets[1:] = ws[_HEADER_FIXED:_HEADER_FIXED + 4 * N].view(torch.int32).to(torch.int64).cumsum(0)
        keys = torch.empty(E, dtype=torch.int64, device=dev)
        boundary = torch.empty(E, dtype=torch.int32, device=dev)
        contrast = torch.empty((E, Cc), dtype=torch.int64, device=dev) if img is not None else None
        if E:
            B._check(lib.fslic_hip_rag_compact(dev.index, _stream(dev), N, Cc, capacity, ws.data_ptr(), nbytes, keys.data_ptr(),
                                               boundary.data_ptr(), contrast.data_ptr() if contrast is not None else None, E))
            keys, order = torch.sort(keys)                              # unique keys (frame << 32 | a << 16 | b): one possible order
            boundary = boundary[order]
            if contrast is not None:
                contrast = contrast[order]
        edge_index = torch.stack([(keys >> 16) & 0xFFFF, keys & 0xFFFF])
    return SuperpixelGraph(edge_index, boundary, contrast, offsets, K, capacity)
