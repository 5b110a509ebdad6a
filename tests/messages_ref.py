"""The numpy model of fast_slic_amd/messages.py's rules 1 to 4, float32 operation by operation: np.float32 scalars and arrays (every
numpy float32 operation rounds each element once), explicit loops over the entries p in ascending order, the features of an entry
side by side.  The validity of an entry, its row and the transposed bookkeeping are attention_ref.Entries'.  No torch, no GPU.

Lists: offsets int64 [N * K + 1] (offsets[0] == 0), indices int32 [nnz]; x and g float32 [N, C, K]; per-entry arrays float32 [F, nnz].

The bound of the comparisons with float64 (u = 2^-24, aggregate_ref.gamma): a sum of d terms is d - 1 roundings, the mean one more,
    |fold - exact| <= gamma(d) * sum |terms|          (gamma(d) = (d + 1) u / (1 - (d + 1) u) covers d + 1 roundings)
and a gather, a maximum, a minimum and the masked gradient of one are copies or selections: equality."""
import numpy as np

from attention_ref import Entries      # noqa: F401  (the tests build their lists through this module)

F32 = np.float32
REDUCES = ("sum", "mean", "max", "min")


def node_of(ent, end):
    """The flat (frame, node) each entry reads at `end`; 0 for an entry that is not valid."""
    return ent.f * ent.K + (ent.i if end == "target" else ent.jj)


def lists_of(ent, to):
    """node over (frame, node) -> its entries p in ascending order: the valid entries of the row (to="target"), or the valid entries
    whose index names the node (to="source": the transposed list)."""
    out = [[] for _ in range(ent.N * ent.K)]
    node = node_of(ent, to)
    for p in range(ent.nnz):
        if ent.valid[p]:
            out[int(node[p])].append(p)
    return out


def gather(x, ent, end, degree=None, argmax=None):
    """Rule 1 -> float32 [C, nnz]; with `degree` (per node, [N * K]) x / float32(degree) is gathered, with `argmax` ([N, C, K]) only
    the entry that the node's argmax names keeps its value: the backward of a reduce."""
    x = np.asarray(x, F32)
    N, C, K = x.shape
    flat = x.transpose(1, 0, 2).reshape(C, N * K)
    node = node_of(ent, end)
    arg = None if argmax is None else np.asarray(argmax).transpose(1, 0, 2).reshape(C, N * K)
    out = np.zeros((C, ent.nnz), F32)
    for p in range(ent.nnz):
        if not ent.valid[p]:
            continue
        v = flat[:, node[p]]
        if degree is not None:
            v = v / F32(degree[node[p]])
        if arg is not None:
            v = np.where(arg[:, node[p]] == p, v, F32(0))
        out[:, p] = v
    return out


def reduce(m, ent, how="sum", to="target"):
    """Rules 2 and 3 -> (y float32 [N, F, K], argmax int32 [N, F, K] (max, min; else None), degree int64 [N * K])."""
    m = np.asarray(m, F32)
    Fc, R = m.shape[0], ent.N * ent.K
    y, arg, deg = np.zeros((Fc, R), F32), np.full((Fc, R), -1, np.int32), np.zeros(R, np.int64)
    for node, entries in enumerate(lists_of(ent, to)):
        acc, best = np.zeros(Fc, F32), np.full(Fc, -1, np.int32)
        for p in entries:
            v = m[:, p]
            if how in ("sum", "mean"):
                acc = acc + v
            else:
                take = (best < 0) | (v > acc if how == "max" else v < acc)
                acc, best = np.where(take, v, acc), np.where(take, np.int32(p), best)
        if how == "mean" and entries:
            acc = acc / F32(len(entries))
        y[:, node], arg[:, node], deg[node] = acc, best, len(entries)
    shape = lambda a: np.ascontiguousarray(a.reshape(Fc, ent.N, ent.K).transpose(1, 0, 2))
    return shape(y), (shape(arg) if how in ("max", "min") else None), deg


def gather_backward(g, ent, end):
    """Rule 4: grad_x of entry_gather from g float32 [C, nnz] -> float32 [N, C, K]."""
    return reduce(g, ent, "sum", end)[0]


def reduce_backward(g, ent, how, to, argmax=None, degree=None):
    """Rule 4: grad_m of entry_reduce from g float32 [N, F, K]; argmax and degree as reduce() gave them."""
    return gather(g, ent, to, degree if how == "mean" else None, argmax if how in ("max", "min") else None)
