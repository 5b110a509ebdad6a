"""The numpy model of fast_slic_amd/attention.py's rules 1 to 5, float32 operation by operation (every numpy float32 array operation
rounds each element once; the folds run over the k-th entry of every row at once, which keeps the order inside each row), and a
float64 restatement in torch: dense masked attention per frame and head, through which autograd gives the gradients.  The
exponential is the library's own host entry fslic_hip_crf_expf_host(.., use_libm=0).  No GPU.

Lists: offsets int64 [N * K + 1] (offsets[0] == 0), indices int32 [nnz]; a, b, x, g float32 [N, C, K]; per-entry arrays float32
[Hd, nnz].

The bounds of the comparisons with float64, u = 2^-24, gamma(n) = (n + 1) u / (1 - (n + 1) u) (aggregate_ref.gamma: a product and
n - 1 additions, or n - 1 additions and a division, with one rounding to spare for the float64 side and second-order terms):

  dot, rule A and its transposed form: |fold - exact| <= gamma(n) * sum |terms|, n the terms of the fold.
  alpha of a row of d valid entries, from the same scores, Delta = max |s_p - m| over the row:
      the rounded difference s_p - m has the absolute error Delta u at most, which is a relative error of e_p;
      crf_expf is within one ulp of exp, a relative error below 2 u (no e_p is subnormal while Delta < 87);
      so every e_p, and with them the exact sum of the e_p, is within (Delta + 2) u; the fold of d terms and the division add gamma(d):
      rel(alpha) <= 2 (Delta + 2) u + gamma(d)                                                      (alpha_bound)
  softmax backward, grad_p = alpha_p (g_p - t), t = sum alpha g, with A = sum |alpha g| over the row:
      t is off by (gamma(d) + rel(alpha)) A, the difference adds u |g_p - t|, the product u again and alpha_p its rel(alpha):
      |grad_p - exact| <= alpha_p ((gamma(d) + rel(alpha)) A + (rel(alpha) + 2 u) |g_p - t|)       (softmax_backward_bound)
  graph_attention against float64 from the same query, key and values: the scores are off by ds <= gamma(D + 1) sum |q k| scale (the
      scaling is one more rounding), which moves alpha by the factor exp(2 ds) at most; then rule A:
      |y - exact| <= (rel(alpha) + exp(2 ds) - 1 + gamma(d)) * sum_p |alpha_p v|                    (attention_bound)
Each is multiplied by 1 + 2^-10 for the products of these first-order terms."""
import ctypes as C

import numpy as np

from aggregate_ref import gamma, rows_of

F32 = np.float32
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10


def expf(x):
    """crf_expf of every element of a float32 array, on the host."""
    from fast_slic_amd import _binding as B
    x = np.ascontiguousarray(x, F32)
    out = np.empty_like(x)
    B._check(B.load_library().fslic_hip_crf_expf_host(x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), x.size, 0))
    return out


class Entries(object):
    """Of every entry: its row, frame, node, index and whether it is valid; of every row its clamped bounds."""

    def __init__(self, offsets, indices, N, K):
        offsets, nnz = np.asarray(offsets, np.int64), len(indices)
        assert offsets[0] == 0 and len(offsets) == N * K + 1
        self.N, self.K, self.nnz = N, K, nnz
        self.rows, self.j = rows_of(offsets, nnz), np.asarray(indices, np.int64)
        self.valid = (self.j >= 0) & (self.j < K) & (self.rows < N * K)
        self.f, self.i = np.where(self.valid, self.rows // K, 0), np.where(self.valid, self.rows % K, 0)
        self.jj = np.where(self.valid, self.j, 0)
        self.begin = np.clip(offsets[:-1], 0, nnz)
        self.degree = np.maximum(np.clip(offsets[1:], 0, nnz) - self.begin, 0)
        self.valid_degree = np.bincount(self.rows[self.valid], minlength=N * K)

    def walk(self):
        """(rows, entries): the valid ones among the k-th entries of all rows, for k = 0, 1, ..: every row at most once a step."""
        for k in range(int(self.degree.max()) if self.degree.size else 0):
            r = np.nonzero(self.degree > k)[0]
            p = self.begin[r] + k
            yield r[self.valid[p]], p[self.valid[p]]

    def walk_transposed(self):
        """(targets, entries, rows of the entries): the k-th entry, in ascending p, of every target (frame, index)."""
        p = np.nonzero(self.valid)[0]
        target = self.f[p] * self.K + self.j[p]
        order = np.argsort(target, kind="stable")
        p, target = p[order], target[order]
        begin = np.searchsorted(target, np.arange(self.N * self.K))
        count = np.bincount(target, minlength=self.N * self.K)
        for k in range(int(count.max()) if count.size else 0):
            t = np.nonzero(count > k)[0]
            q = p[begin[t] + k]
            yield t, q, self.rows[q]


def dot(a, b, ent, Hd):
    """Rule 1 -> float32 [Hd, nnz]."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    D = a.shape[1] // Hd
    out = np.zeros((Hd, ent.nnz), F32)
    for h in range(Hd):
        acc = np.zeros(ent.nnz, F32)
        for c in range(h * D, h * D + D):                                  # every entry at once, the channels in order
            acc = acc + a[ent.f, c, ent.i] * b[ent.f, c, ent.jj]
        out[h] = np.where(ent.valid, acc, F32(0))
    return out


def softmax(s, ent):
    """Rule 2 -> float32 [Hd, nnz]."""
    s = np.asarray(s, F32)
    Hd, R, v = s.shape[0], ent.N * ent.K, ent.valid
    m = np.full((Hd, R), -np.inf, F32)
    for r, p in ent.walk():
        m[:, r] = np.maximum(m[:, r], s[:, p])
    e = np.zeros_like(s)
    e[:, v] = expf(s[:, v] - m[:, ent.rows[v]])
    Z = np.zeros((Hd, R), F32)
    for r, p in ent.walk():
        Z[:, r] = Z[:, r] + e[:, p]
    alpha = np.zeros_like(s)
    alpha[:, v] = e[:, v] / Z[:, ent.rows[v]]
    return alpha


def softmax_backward(alpha, g, ent):
    """Rule 4 -> float32 [Hd, nnz]."""
    alpha, g, v = np.asarray(alpha, F32), np.asarray(g, F32), ent.valid
    t = np.zeros((alpha.shape[0], ent.N * ent.K), F32)
    for r, p in ent.walk():
        t[:, r] = t[:, r] + alpha[:, p] * g[:, p]
    out = np.zeros_like(alpha)
    out[:, v] = alpha[:, v] * (g[:, v] - t[:, ent.rows[v]])
    return out


def apply(x, w, ent):
    """Rule A -> float32 [N, C, K]; w float32 [Hd, nnz]."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    N, Cc, K = x.shape
    head = np.arange(Cc) // (Cc // w.shape[0])
    acc = np.zeros((N * K, Cc), F32)
    for r, p in ent.walk():
        acc[r] = acc[r] + w[np.ix_(head, p)].T * x[ent.f[p], :, ent.jj[p]]
    return np.ascontiguousarray(acc.reshape(N, K, Cc).transpose(0, 2, 1))


def apply_transposed(g, w, ent):
    """Rule A over the transposed lists -> float32 [N, C, K]."""
    g, w = np.asarray(g, F32), np.asarray(w, F32)
    N, Cc, K = g.shape
    head = np.arange(Cc) // (Cc // w.shape[0])
    acc = np.zeros((N * K, Cc), F32)
    for t, p, r in ent.walk_transposed():
        acc[t] = acc[t] + w[np.ix_(head, p)].T * g[r // K, :, r % K]
    return np.ascontiguousarray(acc.reshape(N, K, Cc).transpose(0, 2, 1))


def attention(q, k, v, ent, Hd, scale=None, gy=None):
    """Rule 5 -> (y, alpha), and with gy also the gradients (gq, gk, gv) of the composition."""
    q, k, v = np.asarray(q, F32), np.asarray(k, F32), np.asarray(v, F32)
    scale = F32((q.shape[1] // Hd) ** -0.5 if scale is None else scale)
    qs = q * scale
    alpha = softmax(dot(qs, k, ent, Hd), ent)
    y = apply(v, alpha, ent)
    if gy is None:
        return y, alpha
    gy = np.asarray(gy, F32)
    gs = softmax_backward(alpha, dot(gy, v, ent, Hd), ent)
    return y, alpha, (apply(k, gs, ent) * scale, apply_transposed(qs, gs, ent), apply_transposed(gy, alpha, ent))


# ---- the float64 restatement, in torch: dense [N, Hd, K, K] arrays, row i, column j; the graphs hold no entry twice ----
def to_dense(w, ent):
    """A per-entry tensor [Hd, nnz] as dense [N, Hd, K, K]: the valid entries, 0 elsewhere."""
    import torch
    p = np.nonzero(ent.valid)[0]
    assert len(np.unique(ent.rows[p] * ent.K + ent.j[p])) == len(p)
    out = torch.zeros((ent.N, w.shape[0], ent.K, ent.K), dtype=torch.float64)
    return out.index_put((torch.from_numpy(ent.f[p])[:, None], torch.arange(w.shape[0])[None, :], torch.from_numpy(ent.i[p])[:, None],
                          torch.from_numpy(ent.jj[p])[:, None]), w[:, torch.from_numpy(p)].T)


def from_dense(W, ent):
    import torch
    p = torch.from_numpy(np.nonzero(ent.valid)[0])
    out = torch.zeros((W.shape[1], ent.nnz), dtype=torch.float64)
    return out.index_put((torch.arange(W.shape[1])[:, None], p[None, :]), W[torch.from_numpy(ent.f)[p], :, torch.from_numpy(ent.i)[p], torch.from_numpy(ent.jj)[p]].T)


def heads_of(x, Hd):
    return x.reshape(x.shape[0], Hd, x.shape[1] // Hd, x.shape[2])


def dot64(a, b, ent, Hd):
    import torch
    return from_dense(torch.einsum("fhdi,fhdj->fhij", heads_of(a, Hd), heads_of(b, Hd)), ent)


def softmax64(s, ent):
    import torch
    mask = to_dense(torch.ones_like(s), ent) > 0
    S = to_dense(s, ent).masked_fill(~mask, -float("inf"))
    some = mask.any(-1, keepdim=True)
    return from_dense(torch.where(some, torch.softmax(torch.where(some, S, torch.zeros_like(S)), -1), torch.zeros_like(S)) * mask, ent)


def apply64(x, w, ent):
    import torch
    return torch.einsum("fhij,fhdj->fhdi", to_dense(w, ent), heads_of(x, w.shape[0])).reshape(x.shape)


def attention64(q, k, v, ent, Hd, scale=None):
    """Dense masked attention per frame and head -> (y, alpha per entry), float64 torch tensors."""
    scale = float(F32((q.shape[1] // Hd) ** -0.5 if scale is None else scale))
    alpha = softmax64(dot64(q * scale, k, ent, Hd), ent)
    return apply64(v, alpha, ent), alpha


# ---- the bounds of the module's text ----
def row_max(x, ent):
    """The largest |x| over the valid entries of each row -> [Hd, N * K]."""
    out = np.zeros((x.shape[0], ent.N * ent.K))
    for r, p in ent.walk():
        out[:, r] = np.maximum(out[:, r], np.abs(x[:, p]))
    return out


def row_sum(x, ent):
    out = np.zeros((x.shape[0], ent.N * ent.K))
    for r, p in ent.walk():
        out[:, r] += np.abs(x[:, p])
    return out


def alpha_bound(s, ent):
    """rel(alpha) of every entry [Hd, nnz]: 2 (Delta + 2) u + gamma(d), Delta <= the spread of the row's scores."""
    s = np.asarray(s, np.float64)
    hi, lo = np.full((s.shape[0], ent.N * ent.K), -np.inf), np.full((s.shape[0], ent.N * ent.K), np.inf)
    for r, p in ent.walk():
        hi[:, r], lo[:, r] = np.maximum(hi[:, r], s[:, p]), np.minimum(lo[:, r], s[:, p])
    rows = np.minimum(ent.rows, ent.N * ent.K - 1)
    delta = np.where(ent.valid, (hi - lo)[:, rows], 0.0)
    return (2.0 * (delta + 2.0) * U + gamma(ent.valid_degree[rows])) * SLACK


def softmax_backward_bound(alpha64, g, rel, ent):
    """[Hd, nnz]: alpha_p ((gamma(d) + rel) A + (rel + 2 u) |g_p - t|), rel the row's rel(alpha)."""
    rows = np.minimum(ent.rows, ent.N * ent.K - 1)
    t = np.zeros((alpha64.shape[0], ent.N * ent.K))
    for r, p in ent.walk():
        t[:, r] += alpha64[:, p] * g[:, p]
    A = row_sum(alpha64 * g, ent)[:, rows]
    return alpha64 * ((gamma(ent.valid_degree[rows]) + rel) * A + (rel + 2.0 * U) * np.abs(g - t[:, rows])) * SLACK


def attention_bound(q, k, v, ent, Hd, scale=None):
    """-> (y, alpha) of attention64 as numpy arrays and the attention_bound of the module's text, [N, Cv, K]."""
    import torch
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    sc = float(F32((q.shape[1] // Hd) ** -0.5 if scale is None else scale))
    D, rows = q.shape[1] // Hd, np.minimum(ent.rows, ent.N * ent.K - 1)
    y, alpha = attention64(t64(q), t64(k), t64(v), ent, Hd, scale)
    s = dot64(t64(q) * sc, t64(k), ent, Hd).numpy()
    ds = row_max(gamma(D + 1) * dot64(t64(np.abs(q)) * sc, t64(np.abs(k)), ent, Hd).numpy(), ent)      # [Hd, N * K]
    rel = row_max(alpha_bound(s, ent), ent) + np.expm1(2.0 * ds) + gamma(ent.valid_degree)[None, :]
    head = np.arange(v.shape[1]) // (v.shape[1] // Hd)
    rel = rel.reshape(Hd, ent.N, ent.K)[head].transpose(1, 0, 2)                                        # [N, Cv, K]
    return y.numpy(), alpha.numpy(), rel * apply64(t64(np.abs(v)), alpha, ent).numpy() * SLACK
