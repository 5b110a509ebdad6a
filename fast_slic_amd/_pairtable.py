"""The driver of the per-frame label pair table (csrc/pairtable.h) that superpixel_graph (rag.py), label_overlap (compare.py) and
contract_graph (merge.py) share -- grow until it holds the map, read the header, compact, sort -- and the limits of its capacity.
This module imports torch; the package itself does not import it."""
import numpy as np
import torch

_HEADER_FIXED = 16          # bytes of the workspace header before the per-frame pair counts (csrc/pairtable.h)
MIN_CAPACITY, MAX_CAPACITY = 64, 1 << 31


def pow2_at_least(v):
    return 1 << max(0, int(v) - 1).bit_length()


def start_capacity(first, limit, _start_capacity):
    """(first capacity, limit) of a call; `_start_capacity` (testing) replaces the first and may raise the limit."""
    if _start_capacity is None:
        return first, limit
    capacity = _start_capacity
    if isinstance(capacity, bool) or not isinstance(capacity, int) or not MIN_CAPACITY <= capacity <= MAX_CAPACITY \
            or capacity & (capacity - 1):
        raise ValueError("_start_capacity must be a power of two in [%d, 2^31]" % MIN_CAPACITY)
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
