"""Float64 numpy reference of superpixel pooling (fast_slic_amd/pool.py): sum, |x| sum, counts, max with its lowest-index argmax,
and unpool.  Per channel np.bincount / one sort per frame, so that 3840x2160 frames take seconds."""
import numpy as np


def valid_labels(labels, K):
    """int64 labels of [.., H, W] and the mask of those in [0, K) (the int16 map's -1 is 0xFFFF, as the library reads it)."""
    lab = np.asarray(labels)
    if lab.dtype == np.int16:
        lab = lab.view(np.uint16)
    lab = lab.astype(np.int64)
    return lab, (lab >= 0) & (lab < K)


def ordered_key(x):
    """uint32 whose order is the float order (-0.0 below +0.0), as the kernel's."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def from_key(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def pool_frame(x, labels, K):
    """x [C, H, W] float32, labels [H, W] -> dict of sum / abs (float64 [C, K]), counts (int64 [K]), max (float32 [C, K], 0 where
    empty) and argmax (int64 [C, K], -1 where empty)."""
    Cc, H, W = x.shape
    lab, ok = valid_labels(labels, K)
    idx = lab.reshape(-1)[ok.reshape(-1)]
    pos = np.nonzero(ok.reshape(-1))[0]
    counts = np.bincount(idx, minlength=K).astype(np.int64)
    out = dict(sum=np.zeros((Cc, K)), abs=np.zeros((Cc, K)), counts=counts,
               max=np.zeros((Cc, K), np.float32), argmax=np.full((Cc, K), -1, np.int64))
    order = np.argsort(idx, kind="stable")               # by label, then by flat index
    pos_s = pos[order]
    nonempty = np.nonzero(counts)[0]
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])[nonempty]
    for c in range(Cc):
        v = x[c].reshape(-1)[pos].astype(np.float64)
        out["sum"][c] = np.bincount(idx, weights=v, minlength=K)
        out["abs"][c] = np.bincount(idx, weights=np.abs(v), minlength=K)
        if idx.size == 0:
            continue
        key = ordered_key(x[c].reshape(-1)[pos_s]).astype(np.int64)
        kmax = np.maximum.reduceat(key, starts)
        at_max = key == np.repeat(kmax, counts[nonempty])
        first = np.minimum.reduceat(np.where(at_max, pos_s, np.iinfo(np.int64).max), starts)
        out["max"][c, nonempty] = from_key(kmax.astype(np.uint32))
        out["argmax"][c, nonempty] = first
    return out


def pool(x, labels, K):
    """[N, C, H, W] / [N, H, W] -> the dict of pool_frame with a leading N axis."""
    frames = [pool_frame(x[n], labels[n], K) for n in range(x.shape[0])]
    return {k: np.stack([f[k] for f in frames]) for k in frames[0]}


def unpool(values, labels, fill):
    """values [C, K] / [N, C, K], labels [H, W] / [N, H, W] -> [C, H, W] / [N, C, H, W]: a gather, `fill` where the label is not in
    [0, K)."""
    values = np.asarray(values, dtype=np.float32)
    batched = values.ndim == 3
    V, L = (values, labels) if batched else (values[None], np.asarray(labels)[None])
    lab, ok = valid_labels(L, V.shape[-1])
    out = np.empty(V.shape[:2] + L.shape[-2:], np.float32)
    for n in range(V.shape[0]):
        out[n] = np.where(ok[n][None], V[n][:, np.where(ok[n], lab[n], 0)], np.float32(fill))
    return out if batched else out[0]
