"""A plain-torch model of SimpleCRF's mean-field sweeps, differentiable through torch autograd: the reference of the backward of
superpixel_crf (tests/test_crf_tensor_grad_cpu.py, tests/test_gpu_crf_tensor_grad.py).  Everything is computed in `dtype` on the CPU.

    m[i,c] = sum_k w_k q[j_k,c] + a_i q[n-1,i,c] + b_i q[n+1,i,c]      w_k = energy * member factor of entry k of row i
    g[i,c] = sum_{o != c} compat[o] m[i,o],  ex = exp(-(u + g)),  q' = ex / max(sum_c ex, 1e-5)

The edge weights follow csrc/crf.h: the spatial energy (0 for a self-loop), the temporal energy and the member factor
sqrt(m_from / max(int(m_to), 1)).  Messages are taken with index_add; entries whose index is outside [0, K) are dropped."""
import numpy as np
import torch

DEFAULTS = dict(spatial_w=10.0, temporal_w=10.0, spatial_srgb=13.0, temporal_srgb=13.0, spatial_sxy=80.0, spatial_smooth_w=0.0,
                spatial_smooth_sxy=3.0)


def edge_weights(offsets, indices, yxrgb, members, params, temporal, dtype):
    """-> (row, src, w) per live entry over (frame, node), and the temporal weights a, b [N, 1, K] (zero when off or at the ends)."""
    p = dict(DEFAULTS)
    p.update(params or {})
    yx = torch.as_tensor(yxrgb).detach().cpu().to(dtype)                       # [N, 5, K]
    N, _, K = yx.shape
    mem = torch.as_tensor(members).cpu().to(torch.int64)                       # [N, K], the 32 bits of num_members
    m_from = (mem & 0xFFFFFFFF).to(dtype)
    m_to = mem.clamp_min(1).to(dtype)                                          # read as int, taken as 1 when <= 0
    off = np.asarray(torch.as_tensor(offsets).cpu(), dtype=np.int64)
    idx = np.asarray(torch.as_tensor(indices).cpu(), dtype=np.int64)
    row = np.repeat(np.arange(N * K), np.diff(off))
    keep = (idx >= 0) & (idx < K)
    row, j = torch.from_numpy(row[keep]), torch.from_numpy(idx[keep])
    n, i = row // K, row % K
    y, x, rgb = yx[:, 0], yx[:, 1], yx[:, 2:]
    d_rgb = ((rgb[n, :, i] - rgb[n, :, j]) / p["spatial_srgb"]).pow(2).sum(1)
    dx, dy = x[n, i] - x[n, j], y[n, i] - y[n, j]
    d_xy = (dx / p["spatial_sxy"]).pow(2) + (dy / p["spatial_sxy"]).pow(2)
    d_smooth = (dx / p["spatial_smooth_sxy"]).pow(2) + (dy / p["spatial_smooth_sxy"]).pow(2)
    e = p["spatial_w"] * torch.exp(-d_rgb / 2 - d_xy / 2) + p["spatial_smooth_w"] * torch.exp(-d_smooth / 2)
    e = torch.where(i == j, torch.zeros_like(e), e)
    w = e * torch.sqrt(m_from[n, j] / m_to[n, i])
    a = torch.zeros(N, 1, K, dtype=dtype)
    b = torch.zeros(N, 1, K, dtype=dtype)
    if temporal and N > 1:
        e_t = p["temporal_w"] * torch.exp(-((rgb[1:] - rgb[:-1]) / p["temporal_srgb"]).pow(2).sum(1) / 2)       # [N - 1, K]
        a[1:, 0] = e_t * torch.sqrt(m_from[:-1] / m_to[1:])                    # towards n - 1
        b[:-1, 0] = e_t * torch.sqrt(m_from[1:] / m_to[:-1])                   # towards n + 1
    return row, n * K + j, w, a, b


def mean_field(unaries, offsets, indices, yxrgb, members, max_iter, params=None, compat=None, temporal=False, q0=None,
               dtype=torch.float64):
    """q after max_iter sweeps, [N, C, K] in `dtype`.  unaries, q0 and compat may be tensors of `dtype` that require gradients
    (anything else is converted)."""
    u = torch.as_tensor(unaries).to(dtype)
    N, Cn, K = u.shape
    row, src, w, a, b = edge_weights(offsets, indices, yxrgb, members, params, temporal, dtype)
    comp = torch.ones(Cn, dtype=dtype) if compat is None else torch.as_tensor(compat).to(dtype)
    potts = (1.0 - torch.eye(Cn, dtype=dtype)) * comp[None, :]                 # [c, o]: compat[o] for o != c
    q = torch.exp(-u) if q0 is None else torch.as_tensor(q0).to(dtype)
    for _ in range(max_iter):
        flat = q.permute(1, 0, 2).reshape(Cn, N * K)
        m = torch.zeros(Cn, N * K, dtype=dtype).index_add(1, row, flat[:, src] * w[None, :])
        m = m.reshape(Cn, N, K).permute(1, 0, 2)
        m = m + a * torch.cat([torch.zeros_like(q[:1]), q[:-1]]) + b * torch.cat([q[1:], torch.zeros_like(q[:1])])
        ex = torch.exp(-(u + torch.einsum("co,nok->nck", potts, m)))
        q = ex / ex.sum(1, keepdim=True).clamp_min(1e-5)
    return q


def gradients(weight, unaries, offsets, indices, yxrgb, members, max_iter, params=None, compat=None, temporal=False, q0=None,
              dtype=torch.float64):
    """The gradients of (q * weight).sum() -> dict(q, unaries, compat, q0 (None without q0)), all detached tensors of `dtype`."""
    u = torch.as_tensor(unaries).detach().cpu().to(dtype).requires_grad_(True)
    Cn = u.shape[1]
    comp = (torch.ones(Cn) if compat is None else torch.as_tensor(compat)).detach().cpu().to(dtype).requires_grad_(True)
    start = None if q0 is None else torch.as_tensor(q0).detach().cpu().to(dtype).requires_grad_(True)
    q = mean_field(u, offsets, indices, yxrgb, members, max_iter, params, comp, temporal, start, dtype)
    (q * torch.as_tensor(weight).detach().cpu().to(dtype)).sum().backward()
    zero = torch.zeros_like
    return dict(q=q.detach(), unaries=u.grad if u.grad is not None else zero(u), compat=comp.grad if comp.grad is not None else zero(comp),
                q0=None if start is None else (start.grad if start.grad is not None else zero(start)))


def rel_err(x, ref):
    """max |x - ref| / max |ref| (the absolute error where the reference is all zero)."""
    x, ref = torch.as_tensor(x).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    scale = float(ref.abs().max())
    return float((x - ref).abs().max()) / (scale if scale > 0 else 1.0)


def transpose_loop(offsets, indices, N, K):
    """The transposed lists by a loop: per (frame, target) the (entry, row) pairs in ascending entry order."""
    off, idx = [int(v) for v in offsets], [int(v) for v in indices]
    lists = [[] for _ in range(N * K)]
    for r in range(N * K):
        for k in range(off[r], off[r + 1]):
            if 0 <= idx[k] < K:
                lists[(r // K) * K + idx[k]].append((k, r))
    return lists
