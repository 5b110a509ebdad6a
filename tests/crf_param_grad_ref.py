"""A plain-torch model of the learnable energies of superpixel_crf: the reference of crf_edge_energies, of the `energies` argument and
of a params tensor (tests/test_crf_tensor_param_grad_cpu.py, tests/test_gpu_crf_tensor_param_grad.py).  It follows the formulas of
tests/crf_grad_ref.py; everything is computed in `dtype` on the CPU.

The seven params are a [7] tensor in PARAM_NAMES order.  The energies are intermediate tensors whose gradients are kept:

    edge[k]     = w E1 + w_s E2,  E1 = exp(-(D_rgb / s_rgb^2 + D_xy / s_xy^2) / 2),  E2 = exp(-D_xy / s_s^2 / 2)     per neighbour entry k
                  (0 for a self-loop, for an index outside [0, K) and for an entry behind the last row)
    links[n,0,i] = w_t exp(-D_rgb(n, n - 1) / s_t^2 / 2),  links[n,1,i] likewise with n + 1      (0 without that frame or temporal)

with D_* the raw squared differences.  The sweeps take the weight of entry k as edge[k] * member factor (also for a self-loop when the
energies are given), the temporal weights as links * member factor."""
import numpy as np
import torch

PARAM_NAMES = ("spatial_w", "temporal_w", "spatial_srgb", "temporal_srgb", "spatial_sxy", "spatial_smooth_w", "spatial_smooth_sxy")
SPATIAL = (0, 2, 4, 5, 6)             # the names whose gradient comes through edge; the other two come through links
DEFAULTS = dict(spatial_w=10.0, temporal_w=10.0, spatial_srgb=13.0, temporal_srgb=13.0, spatial_sxy=80.0, spatial_smooth_w=0.0,
                spatial_smooth_sxy=3.0)


def theta_of(params, dtype=torch.float64):
    """A dict (or None) -> the [7] tensor of the float32 values the GPU call gets, in `dtype`."""
    p = dict(DEFAULTS)
    p.update(params or {})
    return torch.tensor([p[n] for n in PARAM_NAMES], dtype=torch.float32).to(dtype)


def _lists(offsets, indices, N, K):
    """-> per entry its row over (frame, node) (N * K: behind the last row), its index, and the live mask."""
    off = np.asarray(torch.as_tensor(offsets).cpu(), dtype=np.int64)
    idx = np.asarray(torch.as_tensor(indices).cpu(), dtype=np.int64)
    row = np.searchsorted(off[1:], np.arange(idx.shape[0]), side="right")
    live = (idx >= 0) & (idx < K) & (row < N * K)
    return torch.from_numpy(row), torch.from_numpy(idx), torch.from_numpy(live)


def energies(theta, offsets, indices, yxrgb, temporal, dtype=torch.float64, derivatives=False):
    """-> edge [nnz], links [N, 2, K], differentiable with respect to `theta`; with derivatives=True also the list of the seven
    d energy / d theta[p] ([nnz] for the spatial names, [N, 2, K] for the temporal ones), by the closed formulas."""
    yx = torch.as_tensor(yxrgb).detach().cpu().to(dtype)
    N, _, K = yx.shape
    row, idx, live = _lists(offsets, indices, N, K)
    w, wt, srgb, st, sxy, ws, ss = theta.unbind(0)
    nnz = idx.shape[0]
    r, j = row[live], idx[live]
    n, i = r // K, r % K
    y, x, rgb = yx[:, 0], yx[:, 1], yx[:, 2:]
    D_rgb = (rgb[n, :, i] - rgb[n, :, j]).pow(2).sum(1)
    D_xy = (x[n, i] - x[n, j]).pow(2) + (y[n, i] - y[n, j]).pow(2)
    off_diag = (i != j).to(dtype)                                               # a self-loop has the constant energy 0
    E1 = torch.exp(-(D_rgb / srgb ** 2 + D_xy / sxy ** 2) / 2) * off_diag
    E2 = torch.exp(-D_xy / ss ** 2 / 2) * off_diag
    where = torch.nonzero(live)[:, 0]

    def full(v):
        return torch.zeros(nnz, dtype=dtype).index_add(0, where, v)

    edge = full(w * E1 + ws * E2)
    links = torch.zeros(N, 2, K, dtype=dtype)
    Et = D_t = None
    if temporal and N > 1:
        D_t = (rgb[1:] - rgb[:-1]).pow(2).sum(1)                                # [N - 1, K]: between n and n + 1
        Et = torch.exp(-D_t / st ** 2 / 2)
        zero = torch.zeros(1, K, dtype=dtype)
        links = torch.stack([torch.cat([zero, wt * Et]), torch.cat([wt * Et, zero])], dim=1)
    if not derivatives:
        return edge, links
    with torch.no_grad():
        de = [None] * 7
        de[0], de[5] = full(E1), full(E2)
        de[2] = full(w * E1 * D_rgb / srgb ** 3)
        de[4] = full(w * E1 * D_xy / sxy ** 3)
        de[6] = full(ws * E2 * D_xy / ss ** 3)
        de[1] = de[3] = torch.zeros(N, 2, K, dtype=dtype)
        if Et is not None:
            zero = torch.zeros(1, K, dtype=dtype)
            d3 = wt * Et * D_t / st ** 3
            de[1] = torch.stack([torch.cat([zero, Et]), torch.cat([Et, zero])], dim=1)
            de[3] = torch.stack([torch.cat([zero, d3]), torch.cat([d3, zero])], dim=1)
    return edge, links, de


def scales(g_edge, g_links, de):
    """A_p = sum |g_k de_k/dp| and B_p = max |g| sum_k |de_k/dp|, with g the gradient of edge for the spatial names and of links for the
    two temporal ones -> two [7] float64 tensors."""
    A, Bs = torch.zeros(7, dtype=torch.float64), torch.zeros(7, dtype=torch.float64)
    for p in range(7):
        g = (g_edge if p in SPATIAL else g_links).detach().double()
        d = de[p].double()
        A[p] = (g * d).abs().sum()
        Bs[p] = (float(g.abs().max()) if g.numel() else 0.0) * d.abs().sum()
    return A, Bs


def mean_field(unaries, offsets, indices, members, edge, links, max_iter, compat=None, temporal=False, q0=None, dtype=torch.float64):
    """q after max_iter sweeps on given energies, [N, C, K] in `dtype` (the second entry: tests/crf_grad_ref.mean_field with the weights
    taken from edge [nnz] and links [N, 2, K] or None)."""
    u = torch.as_tensor(unaries).to(dtype)
    N, Cn, K = u.shape
    mem = torch.as_tensor(members).cpu().to(torch.int64)
    m_from = (mem & 0xFFFFFFFF).to(dtype)
    m_to = mem.clamp_min(1).to(dtype)
    row, idx, live = _lists(offsets, indices, N, K)
    r, j = row[live], idx[live]
    n, i = r // K, r % K
    w = edge[live] * torch.sqrt(m_from[n, j] / m_to[n, i])
    src = n * K + j
    a = torch.zeros(N, 1, K, dtype=dtype)
    b = torch.zeros(N, 1, K, dtype=dtype)
    if temporal and N > 1 and links is not None:
        zero = torch.zeros(1, K, dtype=dtype)
        a = torch.cat([zero, links[1:, 0] * torch.sqrt(m_from[:-1] / m_to[1:])])[:, None]       # towards n - 1
        b = torch.cat([links[:-1, 1] * torch.sqrt(m_from[1:] / m_to[:-1]), zero])[:, None]      # towards n + 1
    comp = torch.ones(Cn, dtype=dtype) if compat is None else torch.as_tensor(compat).to(dtype)
    potts = (1.0 - torch.eye(Cn, dtype=dtype)) * comp[None, :]
    q = torch.exp(-u) if q0 is None else torch.as_tensor(q0).to(dtype)
    for _ in range(max_iter):
        flat = q.permute(1, 0, 2).reshape(Cn, N * K)
        m = torch.zeros(Cn, N * K, dtype=dtype).index_add(1, r, flat[:, src] * w[None, :])
        m = m.reshape(Cn, N, K).permute(1, 0, 2)
        m = m + a * torch.cat([torch.zeros_like(q[:1]), q[:-1]]) + b * torch.cat([q[1:], torch.zeros_like(q[:1])])
        ex = torch.exp(-(u + torch.einsum("co,nok->nck", potts, m)))
        q = ex / ex.sum(1, keepdim=True).clamp_min(1e-5)
    return q


def gradients(weight, unaries, offsets, indices, yxrgb, members, max_iter, theta=None, energies_given=None, compat=None, temporal=False,
              q0=None, dtype=torch.float64):
    """The gradients of (q * weight).sum().  With `theta` ([7], any dtype) the energies are computed from it and kept as intermediate
    tensors; with energies_given = (edge, links or None) they are leaves.  -> dict(q, unaries, compat, q0, edge, links (the gradients
    of the two energies), edge_value, links_value, and with theta: theta (its gradient), A, B (the scales))."""
    u = torch.as_tensor(unaries).detach().cpu().to(dtype).requires_grad_(True)
    Cn = u.shape[1]
    comp = (torch.ones(Cn) if compat is None else torch.as_tensor(compat)).detach().cpu().to(dtype).requires_grad_(True)
    start = None if q0 is None else torch.as_tensor(q0).detach().cpu().to(dtype).requires_grad_(True)
    th = de = None
    if energies_given is None:
        th = torch.as_tensor(theta).detach().cpu().to(dtype).requires_grad_(True)
        edge, links, de = energies(th, offsets, indices, yxrgb, temporal, dtype, derivatives=True)
        if edge.requires_grad:
            edge.retain_grad()
        if links.requires_grad:
            links.retain_grad()
    else:
        edge = torch.as_tensor(energies_given[0]).detach().cpu().to(dtype).requires_grad_(True)
        links = None if energies_given[1] is None else torch.as_tensor(energies_given[1]).detach().cpu().to(dtype).requires_grad_(True)
    q = mean_field(u, offsets, indices, members, edge, links, max_iter, comp, temporal, start, dtype)
    (q * torch.as_tensor(weight).detach().cpu().to(dtype)).sum().backward()

    def grad(t):
        return None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t)).detach()

    out = dict(q=q.detach(), unaries=grad(u), compat=grad(comp), q0=grad(start), edge=grad(edge), links=grad(links),
               edge_value=edge.detach(), links_value=None if links is None else links.detach())
    if th is not None:
        out["theta"] = grad(th)
        out["A"], out["B"] = scales(out["edge"], out["links"], de)
    return out


def energies_backward(theta, offsets, indices, yxrgb, temporal, g_edge, g_links, dtype=torch.float64):
    """The backward of energies() alone for given upstream gradients -> (the gradient of theta [7] in `dtype`, A [7])."""
    th = torch.as_tensor(theta).detach().cpu().to(dtype).requires_grad_(True)
    edge, links, de = energies(th, offsets, indices, yxrgb, temporal, dtype, derivatives=True)
    ge, gl = torch.as_tensor(g_edge).detach().cpu().to(dtype), torch.as_tensor(g_links).detach().cpu().to(dtype)
    total = (edge * ge).sum() + (links * gl).sum()
    if total.requires_grad:
        total.backward()
    A, _ = scales(ge, gl, de)
    return (th.grad if th.grad is not None else torch.zeros_like(th)).detach(), A
