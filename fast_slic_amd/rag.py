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
import numpy as np
import torch

from . import _binding as B, _pairtable as PT, _tensors as T

__all__ = ["superpixel_graph", "SuperpixelGraph"]

MAX_CHANNELS = 4


def first_capacity(K):
    """Slots per frame of the first pair table: sized for a planar map (a Slic map has about 2.9 K edges), under half load."""
    return max(1024, PT.pow2_at_least(8 * K))


def capacity_limit(K, H, W, connectivity):
    """Slots per frame that hold any map of this shape at half load: no more distinct pairs than label pairs or pixel pairs."""
    pairs = min(K * (K - 1) // 2, (connectivity // 2) * H * W)
    return min(PT.MAX_CAPACITY, max(first_capacity(K), PT.pow2_at_least(2 * pairs)))


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


# ---- a SuperpixelGraph as an argument (merge.py, regions.py): its checks run before any device work ----
def check_graph(graph):
    """-> (N, K, E, C) of a SuperpixelGraph whose fields have the types and shapes superpixel_graph gives them."""
    if not isinstance(graph, SuperpixelGraph):
        raise ValueError("graph must be a SuperpixelGraph")
    K = T.check_count(graph.num_components, "num_components")
    T.check_tensor(graph.edge_index, "graph.edge_index", (torch.int64,), "[2, E]", lambda s: len(s) == 2 and s[0] == 2)
    E = int(graph.edge_index.shape[1])
    T.check_tensor(graph.offsets, "graph.offsets", (torch.int64,), "[N + 1]", lambda s: len(s) == 1 and s[0] >= 2)
    N = int(graph.offsets.shape[0]) - 1
    if E >= 1 << 31:
        raise ValueError("the graph must have fewer than 2^31 edges")
    if N * K >= 1 << 31:
        raise ValueError("N * num_components must be below 2^31")
    T.check_tensor(graph.boundary, "graph.boundary", (torch.int32,), "[E]", lambda s: s == (E,))
    Cc = 0
    if graph.contrast is not None:
        T.check_tensor(graph.contrast, "graph.contrast", (torch.int64,), "[E, C] with C in 1 .. %d" % MAX_CHANNELS,
                       lambda s: len(s) == 2 and s[0] == E and 1 <= s[1] <= MAX_CHANNELS)
        Cc = int(graph.contrast.shape[1])
    return N, K, E, Cc


def graph_device(graph, others):
    """The GPU of the graph; others: ((tensor or None, name), ...) must be there too.  A CPU tensor is the last thing refused."""
    return T.one_device([(graph.edge_index, "graph.edge_index"), (graph.offsets, "graph.offsets"), (graph.boundary, "graph.boundary"),
                         (graph.contrast, "graph.contrast")] + list(others))


def graph_edges(graph):
    """-> (edge_index, offsets), contiguous: what every entry that takes a graph is given."""
    return graph.edge_index.contiguous(), graph.offsets.contiguous()


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
    T.check_label_map(labels, "labels")
    H, W = (int(v) for v in labels.shape[-2:])
    if H * W >= 1 << 29:
        raise ValueError("H * W must be below 2^29")
    K = T.check_count(num_components, "num_components")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))
    connectivity = int(connectivity)
    if image is not None:
        _check_image(image, labels.shape)
    capacity, limit = PT.start_capacity(first_capacity(K), capacity_limit(K, H, W, connectivity), _start_capacity)
    dev = T.one_device(((labels, "labels"), (image, "image")), device)

    lib = T.library("fslic_hip_rag_accumulate", "region adjacency graph entry points")
    batched = labels.ndim == 3
    lab, ltype = T.labels_on(labels, dev, batched)
    img = None
    if image is not None:
        img = (torch.from_numpy(np.ascontiguousarray(image)) if isinstance(image, np.ndarray) else image).to(device=dev)
        img = T.batch_of(img, batched)
    N, Cc = lab.shape[0], img.shape[-1] if img is not None else 0

    def accumulate(capacity):
        ws, nbytes = T.scratch(dev, lib.fslic_hip_rag_workspace_size, N, K, Cc, capacity)
        B._check(lib.fslic_hip_rag_accumulate(dev.index, T.stream(dev), N, H, W, K, connectivity, lab.data_ptr(), ltype, T.ptr(img), Cc,
                                              capacity, ws.data_ptr(), nbytes))
        return ws, nbytes

    def compact(ws, nbytes, capacity, E, keys, boundary, contrast=None):
        B._check(lib.fslic_hip_rag_compact(dev.index, T.stream(dev), N, Cc, capacity, ws.data_ptr(), nbytes, keys.data_ptr(),
                                           boundary.data_ptr(), T.ptr(contrast), E))

    with torch.cuda.device(dev):
        edge_index, boundary, extra, offsets, capacity = PT.run(accumulate, compact, N, capacity, limit, dev,
                                                                [((Cc,), torch.int64)] if img is not None else [])
    contrast = extra[0] if extra else None
    return SuperpixelGraph(edge_index, boundary, contrast, offsets, K, capacity)
