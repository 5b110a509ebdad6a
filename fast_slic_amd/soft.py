"""Soft superpixel assignment on float feature tensors over a regular seed grid, with gradients (csrc/soft.hip).

    x = with_coords(features, grid, compactness=10.0)              # [N, C, H, W] -> [N, C + 2, H, W]: the scaled pixel coordinates appended
    Q, centres = soft_slic(x, grid, max_iter=10)                   # Q: [N, 9, H, W], centres: [N, C + 2, K]
    labels = soft_labels(Q, grid)                                  # int32 [N, H, W], for superpixel_pool / superpixel_graph / label_overlap
    Q = soft_assign(features, centres, grid)                       # one assignment step
    centres, weights = soft_pool(features, Q, grid, return_weights=True)
    recon = soft_unpool(centres, Q, grid)                          # [N, C, K] -> [N, C, H, W]

SLIC's k-means on arbitrary float32 features with soft assignments (Superpixel Sampling Networks, Jampani et al. 2018).  `grid` =
(gh, gw) cuts the frame into K = gh * gw cells, 1 <= gh <= H, 1 <= gw <= W, K <= 65534: pixel (y, x) lies in cell
(cy, cx) = ((y * gh) // H, (x * gw) // W).  Every pixel is distributed over the 3 x 3 cells around its own: slot j = 3 (dy + 1) + (dx + 1),
dy, dx in {-1, 0, 1}, names cell (cy + dy, cx + dx), superpixel k = (cy + dy) * gw + (cx + dx); a slot outside the grid is invalid, its Q
is exactly +0.0 and it takes part in nothing.  Tensors are float32, channel-first, on a ROCm GPU; [C, H, W] is accepted wherever
[N, C, H, W] is (centres and values then [C, K], Q [9, H, W]) and the result loses the batch dimension.  The work runs on torch's current
stream of the features' device without host synchronisation; scratch memory comes from torch's caching allocator.  No atomics: a
superpixel gathers from its own window in a fixed order, so results are bitwise reproducible and independent of the batch position and
of the other channels.  Every function is differentiable once (features, centres, values, Q).  This module imports torch; the package
itself does not import it.
"""
import numbers

import torch
from torch.autograd.function import once_differentiable

from . import _binding as B, _tensors as T

__all__ = ["soft_assign", "soft_pool", "soft_unpool", "soft_labels", "soft_slic", "with_coords"]


_ENTRY = ("fslic_hip_soft_assign", "soft assignment entry points")


# ---- argument checks: all of them run before any device work ----
def _check_grid(grid, H, W):
    if not isinstance(grid, (tuple, list)) or len(grid) != 2:
        raise ValueError("grid must be a pair (gh, gw)")
    if any(isinstance(g, bool) or not isinstance(g, numbers.Integral) for g in grid):
        raise ValueError("grid must be a pair of integers")
    gh, gw = int(grid[0]), int(grid[1])
    if not (1 <= gh <= H and 1 <= gw <= W):
        raise ValueError("grid must satisfy 1 <= gh <= H and 1 <= gw <= W, got %s for %d x %d pixels" % ((gh, gw), H, W))
    if gh * gw > T.MAX_COMPONENTS:
        raise ValueError("grid must have at most %d cells, got %d" % (T.MAX_COMPONENTS, gh * gw))
    if H * W >= 1 << 31:
        raise ValueError("H * W must be below 2^31")
    return gh, gw


def _check_map(t, what):
    """features-like: [C, H, W] or [N, C, H, W] -> batched?"""
    T.check_float_map(t, (3, 4), what, "[C, H, W] or [N, C, H, W]")
    return t.dim() == 4


def _check_table(t, what, batched, lead, K):
    """centres / values: [C, K] or [N, C, K] matching the batch and the grid; lead: the expected (N,) or ()"""
    T.check_float_map(t, (3,) if batched else (2,), what, "[N, C, K]" if batched else "[C, K]")
    if tuple(t.shape[:len(lead)]) != tuple(lead) or t.shape[-1] != K:
        raise ValueError("%s must have shape %s to match the batch and the grid, got %s" % (what, tuple(lead) + ("C", K), tuple(t.shape)))


def _check_q(q, batched, lead, H, W):
    T.check_float_map(q, (4,) if batched else (3,), "Q", "[N, 9, H, W]" if batched else "[9, H, W]")
    want = tuple(lead) + (9, H, W)
    if tuple(q.shape) != want:
        raise ValueError("Q must have shape %s, got %s" % (want, tuple(q.shape)))


def _same_device(a, b, what):
    if b.device != a.device:
        raise ValueError("%s must be on the device of the other tensors (%s), got %s" % (what, a.device, b.device))


# ---- the raw calls: contiguous [N, ...] tensors on one device ----
def _geom(t, N, Cc, H, W, grid):
    return (t.device.index, T.stream(t.device), N, Cc, H, W, grid[0], grid[1])


def _assign_raw(feat, cen, grid):
    N, Cc, H, W = feat.shape
    q = torch.empty((N, 9, H, W), dtype=torch.float32, device=feat.device)
    B._check(T.library(*_ENTRY).fslic_hip_soft_assign(*_geom(feat, N, Cc, H, W, grid), feat.data_ptr(), cen.data_ptr(), q.data_ptr()))
    return q


def _pool_raw(feat, q, grid, centres=None, weights=True):
    N, Cc, H, W = feat.shape
    K = grid[0] * grid[1]
    sums = torch.empty((N, Cc, K), dtype=torch.float32, device=feat.device)
    wts = torch.empty((N, K), dtype=torch.float32, device=feat.device) if weights else None
    B._check(T.library(*_ENTRY).fslic_hip_soft_pool(*_geom(feat, N, Cc, H, W, grid), feat.data_ptr(), q.data_ptr(),
                                                    T.ptr(centres), sums.data_ptr(), T.ptr(wts)))
    return sums, wts


def _unpool_raw(values, q, grid):
    N, Cc, _ = values.shape
    H, W = q.shape[-2:]
    out = torch.empty((N, Cc, H, W), dtype=torch.float32, device=values.device)
    B._check(T.library(*_ENTRY).fslic_hip_soft_unpool(*_geom(values, N, Cc, H, W, grid), values.data_ptr(), q.data_ptr(), out.data_ptr()))
    return out


def _dot_raw(a, b, bias, grid):
    N, Cc, H, W = a.shape
    out = torch.empty((N, 9, H, W), dtype=torch.float32, device=a.device)
    B._check(T.library(*_ENTRY).fslic_hip_soft_dot(*_geom(a, N, Cc, H, W, grid), a.data_ptr(), b.data_ptr(), T.ptr(bias), out.data_ptr()))
    return out


class _Assign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, cen, grid):
        q = _assign_raw(feat, cen, grid)
        ctx.grid = grid
        ctx.save_for_backward(feat, cen, q)
        return q

    @staticmethod
    @once_differentiable
    def backward(ctx, gq):
        feat, cen, q = ctx.saved_tensors
        N, Cc, H, W = feat.shape
        gq = gq.contiguous()
        gd, gf = torch.empty_like(q), torch.empty_like(feat)
        B._check(T.library(*_ENTRY).fslic_hip_soft_assign_backward(*_geom(feat, N, Cc, H, W, ctx.grid), feat.data_ptr(), cen.data_ptr(),
                                                                   q.data_ptr(), gq.data_ptr(), gd.data_ptr(), gf.data_ptr()))
        gs = None
        if ctx.needs_input_grad[1]:          # -2 sum_p gd (F - S[k]), accumulated as written: no difference of two pooled sums
            gs = _pool_raw(feat, gd, ctx.grid, centres=cen, weights=False)[0].mul_(-2.0)
        return (gf if ctx.needs_input_grad[0] else None), gs, None


class _Pool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, q, grid):
        sums, weights = _pool_raw(feat, q, grid)
        ctx.grid = grid
        ctx.save_for_backward(feat, q)
        return sums, weights

    @staticmethod
    @once_differentiable
    def backward(ctx, gsums, gweights):
        feat, q = ctx.saved_tensors
        gsums = gsums.contiguous()
        gf = _unpool_raw(gsums, q, ctx.grid) if ctx.needs_input_grad[0] else None
        gq = _dot_raw(feat, gsums, gweights.contiguous(), ctx.grid) if ctx.needs_input_grad[1] else None
        return gf, gq, None


class _Unpool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, q, grid):
        ctx.grid = grid
        ctx.save_for_backward(values, q)
        return _unpool_raw(values, q, grid)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        values, q = ctx.saved_tensors
        g = g.contiguous()
        gv = _pool_raw(g, q, ctx.grid, weights=False)[0] if ctx.needs_input_grad[0] else None
        gq = _dot_raw(g, values, None, ctx.grid) if ctx.needs_input_grad[1] else None
        return gv, gq, None


# ---- the public functions ----
def soft_assign(features, centres, grid):
    """Q [N, 9, H, W]: the soft assignment of every pixel of `features` ([N, C, H, W]) to the centres ([N, C, K]) of its nine slots.
    d_j = sum_c (F[c, p] - S[c, k_j])^2, Q_j = exp(-(d_j - min d)) / sum over the valid slots; +0.0 on an invalid slot.
    Differentiable with respect to features and centres."""
    batched = _check_map(features, "features")
    H, W = features.shape[-2:]
    gh, gw = _check_grid(grid, H, W)
    lead = tuple(features.shape[:1]) if batched else ()
    _check_table(centres, "centres", batched, lead, gh * gw)
    if centres.shape[-2] != features.shape[-3]:
        raise ValueError("centres must have the features' %d channels, got %d" % (features.shape[-3], centres.shape[-2]))
    T.check_device(features, "features")
    _same_device(features, centres, "centres")
    q = _Assign.apply(T.batch_of(features, batched), T.batch_of(centres, batched), (gh, gw))
    return q if batched else q.squeeze(0)


def soft_pool(features, Q, grid, normalize=True, return_weights=False):
    """[N, C, K]: sum[c, k] = sum_p Q_{j_k(p)}(p) F[c, p] over the pixels of the 3 x 3 cell window of k, and weight[k] = the same sum of
    Q alone ([N, K] with return_weights).  With normalize the result is sum / weight, 0 where the weight is 0.  Differentiable with
    respect to features and Q."""
    batched = _check_map(features, "features")
    H, W = features.shape[-2:]
    gh, gw = _check_grid(grid, H, W)
    _check_q(Q, batched, tuple(features.shape[:1]) if batched else (), H, W)
    T.check_device(features, "features")
    _same_device(features, Q, "Q")
    sums, weights = _Pool.apply(T.batch_of(features, batched), T.batch_of(Q, batched), (gh, gw))
    out = sums
    if normalize:
        w = weights.unsqueeze(1)
        some = w != 0
        out = torch.where(some, sums / torch.where(some, w, torch.ones_like(w)), torch.zeros_like(sums))
    if not batched:
        out, weights = out.squeeze(0), weights.squeeze(0)
    return (out, weights) if return_weights else out


def soft_unpool(values, Q, grid):
    """[N, C, H, W]: out[c, p] = sum over the valid slots of Q_j(p) V[c, k_j] (SSN's reconstruction).  Differentiable with respect to
    values and Q."""
    if not isinstance(Q, torch.Tensor) or Q.dim() not in (3, 4):
        raise ValueError("Q must be a torch tensor of shape [9, H, W] or [N, 9, H, W]")
    batched = Q.dim() == 4
    H, W = Q.shape[-2:]
    lead = tuple(Q.shape[:1]) if batched else ()
    _check_q(Q, batched, lead, H, W)
    gh, gw = _check_grid(grid, H, W)
    _check_table(values, "values", batched, lead, gh * gw)
    T.check_device(values, "values")
    _same_device(values, Q, "Q")
    out = _Unpool.apply(T.batch_of(values, batched), T.batch_of(Q, batched), (gh, gw))
    return out if batched else out.squeeze(0)


def _slots(H, W, gh, gw, device):
    """k [9, H, W] int64 (0 where the slot is invalid) and valid [9, H, W] bool."""
    cy = (torch.arange(H, device=device) * gh) // H
    cx = (torch.arange(W, device=device) * gw) // W
    d = torch.arange(3, device=device) - 1
    ny = (cy.view(1, H) + d.view(3, 1)).view(3, 1, H, 1)
    nx = (cx.view(1, W) + d.view(3, 1)).view(1, 3, 1, W)
    valid = ((ny >= 0) & (ny < gh) & (nx >= 0) & (nx < gw)).reshape(9, H, W)
    k = (ny * gw + nx).reshape(9, H, W)
    return torch.where(valid, k, torch.zeros_like(k)), valid


def soft_labels(Q, grid):
    """int32 [N, H, W]: per pixel the superpixel of its largest valid Q (on a tie the lowest slot), for superpixel_pool,
    superpixel_graph and label_overlap."""
    if not isinstance(Q, torch.Tensor) or Q.dim() not in (3, 4):
        raise ValueError("Q must be a torch tensor of shape [9, H, W] or [N, 9, H, W]")
    batched = Q.dim() == 4
    H, W = Q.shape[-2:]
    _check_q(Q, batched, tuple(Q.shape[:1]) if batched else (), H, W)
    gh, gw = _check_grid(grid, H, W)
    k, valid = _slots(H, W, gh, gw, Q.device)
    q = Q.detach() if batched else Q.detach().unsqueeze(0)
    q = torch.where(valid.unsqueeze(0), q, torch.full_like(q, float("-inf")))
    best = q.max(dim=1, keepdim=True).values
    rank = (9 - torch.arange(9, device=Q.device)).view(1, 9, 1, 1)                     # the lowest slot that holds the maximum:
    first = (((q == best) & valid.unsqueeze(0)) * rank).argmax(dim=1)                  # a unique largest rank, whatever argmax does on ties
    lab = torch.gather(k.unsqueeze(0).expand(q.shape[0], 9, H, W), 1, first.unsqueeze(1)).squeeze(1).to(torch.int32)
    return lab if batched else lab.squeeze(0)


def soft_slic(features, grid, max_iter=10):
    """(Q, centres): soft SLIC on `features`.  The centres start as the cell means (soft_pool of the one-hot Q on slot 4); then
    `max_iter` rounds of Q = soft_assign(F, S), S = soft_pool(F, Q) (a centre of weight 0 keeps its previous value), and a last
    soft_assign.  Composed from the functions above: autograd reaches `features` through every round."""
    batched = _check_map(features, "features")
    H, W = features.shape[-2:]
    gh, gw = _check_grid(grid, H, W)
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or max_iter < 0:
        raise ValueError("max_iter must be a non-negative integer")
    T.check_device(features, "features")
    feat = T.batch_of(features, batched)
    q0 = torch.zeros((feat.shape[0], 9, H, W), dtype=torch.float32, device=feat.device)
    q0[:, 4] = 1.0
    centres = soft_pool(feat, q0, (gh, gw))
    for _ in range(int(max_iter)):
        q = soft_assign(feat, centres, (gh, gw))
        new, w = soft_pool(feat, q, (gh, gw), return_weights=True)
        centres = torch.where(w.unsqueeze(1) != 0, new, centres)
    q = soft_assign(feat, centres, (gh, gw))
    return (q, centres) if batched else (q.squeeze(0), centres.squeeze(0))


def with_coords(features, grid, compactness):
    """`features` with two more channels, y * s and x * s, s = compactness * max(gh / H, gw / W): the spatial term of SLIC's distance."""
    batched = _check_map(features, "features")
    H, W = features.shape[-2:]
    gh, gw = _check_grid(grid, H, W)
    if isinstance(compactness, bool) or not isinstance(compactness, numbers.Real):
        raise ValueError("compactness must be a real number")
    s = float(compactness) * max(gh / H, gw / W)
    y = (torch.arange(H, dtype=torch.float32, device=features.device) * s).view(H, 1).expand(H, W)
    x = (torch.arange(W, dtype=torch.float32, device=features.device) * s).view(1, W).expand(H, W)
    yx = torch.stack([y, x])
    if batched:
        yx = yx.unsqueeze(0).expand(features.shape[0], 2, H, W)
    return torch.cat([features, yx], dim=-3)
