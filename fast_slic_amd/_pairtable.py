"""What superpixel_graph (rag.py) and label_overlap (compare.py) share: the checks of a label map, the choice of the GPU, and the
driver of the per-frame label pair table (csrc/pairtable.h) -- grow until it holds the map, read the header, compact, sort.  This
module imports torch; the package itself does not import it."""
import numpy as np
import torch

from .pool import _LABEL_TYPE, _NUMPY_LABELS, _check_device

_HEADER_FIXED = 16          # bytes of the workspace header before the per-frame pair counts (csrc/pairtable.h)
_MIN_CAPACITY, _MAX_CAPACITY = 64, 1 << 31


def _pow2_at_least(v):
    return 1 << max(0, int(v) - 1).bit_length()


def check_label_map(t, what):
    if not isinstance(t, (np.ndarray, torch.Tensor)):
        raise ValueError("%s must be a numpy array or a torch tensor" % what)
    if t.ndim not in (2, 3):
        raise ValueError("%s must be [H, W] or [N, H, W], got shape %s" % (what, tuple(t.shape)))
    if 0 in t.shape:
        raise ValueError("%s must not be empty, got shape %s" % (what, tuple(t.shape)))
    ok = t.dtype.type in _NUMPY_LABELS if isinstance(t, np.ndarray) else t.dtype in _LABEL_TYPE
    if not ok:
        raise ValueError("%s must be int16 (Slic.iterate's map), int32 or int64, got %s" % (what, t.dtype))


def pick_device(tensors, device):
    """The GPU of the result; tensors: ((labels, "labels"), (image or None, "image")).  Torch tensors must already be there (and on
    the same one); numpy arrays are uploaded."""
    given = [(t, what) for t, what in tensors if isinstance(t, torch.Tensor)]
    devs = {t.device for t, _ in given if t.device.type == "cuda"}
    if device is not None:
        device = torch.device(device)
        if device.type == "cuda" and device.index is not None:
            devs.add(device)
    if len(devs) > 1:
        raise ValueError("%s and device must name one GPU, got %s" % (", ".join(what for _, what in tensors), sorted(str(d) for d in devs)))
    for t, what in given:                          # (a CPU tensor is the last thing refused)
        _check_device(t, what)
    if device is not None and device.type != "cuda":
        raise ValueError("device must be a ROCm GPU, got %s (there is no CPU fallback)" % device)
    if devs:
        return devs.pop()
    return torch.device("cuda", torch.cuda.current_device())


def start_capacity(first, limit, _start_capacity):
    """(first capacity, limit) of a call; `_start_capacity` (testing) replaces the first and may raise the limit."""
    if _start_capacity is None:
        return first, limit
    capacity = _start_capacity
    if isinstance(capacity, bool) or not isinstance(capacity, int) or not _MIN_CAPACITY <= capacity <= _MAX_CAPACITY \
            or capacity & (capacity - 1):
        raise ValueError("_start_capacity must be a power of two in [%d, 2^31]" % _MIN_CAPACITY)
    return capacity, max(limit, capacity)


def run(accumulate, compact, N, capacity, limit, dev, columns=()):
    """Fills the pair table and reads it out as sorted rows -> (pairs int64 [2, R], count int32 [R], the extra columns, offsets int64
    [N + 1], capacity).  accumulate(capacity) -> (workspace uint8 tensor, its bytes) enqueues one pass into a fresh workspace;
    compact(workspace, bytes, capacity, R, keys, count, *extra) enqueues the compact pass.  columns: per extra column of the rows
    (trailing shape, dtype).  Synchronises the host once per pass: the table doubles and starts over until no frame overflowed."""
    while True:
        ws, nbytes = accumulate(capacity)
        header = ws[:_HEADER_FIXED + 4 * N].cpu().numpy().view(np.uint32)
        if header[0] == 0:
            break
        del ws
        if capacity >= limit:
            raise RuntimeError("fast_slic_amd: the pair table overflowed at its largest size (%d slots per frame)" % capacity)
        capacity *= 2
    R = int(header[_HEADER_FIXED // 4:].sum(dtype=np.int64))
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    offsets[1:] = ws[_HEADER_FIXED:_HEADER_FIXED + 4 * N].view(torch.int32).to(torch.int64).cumsum(0)
    keys = torch.empty(R, dtype=torch.int64, device=dev)
    count = torch.empty(R, dtype=torch.int32, device=dev)
    extra = [torch.empty((R,) + tuple(shape), dtype=dtype, device=dev) for shape, dtype in columns]
    if R:
        compact(ws, nbytes, capacity, R, keys, count, *extra)
        keys, order = torch.sort(keys)                              # unique keys (frame << 32 | a << 16 | b): one possible order
        count = count[order]
        extra = [e[order] for e in extra]
    pairs = torch.stack([(keys >> 16) & 0xFFFF, keys & 0xFFFF])
    return pairs, count, extra, offsets, capacity
