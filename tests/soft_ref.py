"""The model of fast_slic_amd/soft.py: the five functions in plain torch, written from the specification, in the dtype of their input
(float64 is the reference; cast the input to float32 for the same arithmetic in single precision).  Dense index_add over the nine
slots; everything is differentiable by autograd.  Batched tensors only: features [N, C, H, W], centres / values [N, C, K],
Q [N, 9, H, W]."""
import torch


def cells(H, W, grid):
    """cy [H], cx [W] int64: the cell row of every pixel row and the cell column of every pixel column."""
    gh, gw = grid
    return (torch.arange(H) * gh) // H, (torch.arange(W) * gw) // W


def cell_labels(H, W, grid):
    """int32 [H, W]: the cell map, cy * gw + cx."""
    cy, cx = cells(H, W, grid)
    return (cy.view(H, 1) * grid[1] + cx.view(1, W)).to(torch.int32)


def slots(H, W, grid):
    """k [9, H, W] int64 (0 where the slot is invalid), valid [9, H, W] bool; slot j = 3 (dy + 1) + (dx + 1)."""
    gh, gw = grid
    cy, cx = cells(H, W, grid)
    ks, oks = [], []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ny, nx = (cy + dy).view(H, 1).expand(H, W), (cx + dx).view(1, W).expand(H, W)
            ok = (ny >= 0) & (ny < gh) & (nx >= 0) & (nx < gw)
            ks.append(torch.where(ok, ny * gw + nx, torch.zeros_like(ny)))
            oks.append(ok)
    return torch.stack(ks), torch.stack(oks)


def one_hot(N, H, W, dtype=torch.float64):
    q = torch.zeros(N, 9, H, W, dtype=dtype)
    q[:, 4] = 1
    return q


def soft_assign(F, S, grid):
    N, C, H, W = F.shape
    k, ok = slots(H, W, grid)
    d = torch.stack([((F - S[:, :, k[j].reshape(-1)].reshape(N, C, H, W)) ** 2).sum(1) for j in range(9)], 1)
    okb = ok.unsqueeze(0)
    d = torch.where(okb, d, torch.full_like(d, float("inf")))
    m = d.min(dim=1, keepdim=True).values.detach()          # a shift: the quotient does not depend on it
    e = torch.where(okb, torch.exp(-(torch.where(okb, d, m) - m)), torch.zeros_like(d))
    return e / e.sum(1, keepdim=True)


def soft_pool_raw(F, Q, grid):
    """(sums [N, C, K], weights [N, K])"""
    N, C, H, W = F.shape
    K = grid[0] * grid[1]
    k, ok = slots(H, W, grid)
    sums = torch.zeros(N, C, K, dtype=F.dtype)
    weights = torch.zeros(N, K, dtype=F.dtype)
    for j in range(9):
        w = Q[:, j] * ok[j].to(F.dtype)
        idx = k[j].reshape(-1)
        sums = sums.index_add(2, idx, (w.unsqueeze(1) * F).reshape(N, C, H * W))
        weights = weights.index_add(1, idx, w.reshape(N, H * W))
    return sums, weights


def soft_pool(F, Q, grid, normalize=True, return_weights=False):
    sums, weights = soft_pool_raw(F, Q, grid)
    out = sums
    if normalize:
        w = weights.unsqueeze(1)
        some = w != 0
        out = torch.where(some, sums / torch.where(some, w, torch.ones_like(w)), torch.zeros_like(sums))
    return (out, weights) if return_weights else out


def soft_unpool(V, Q, grid):
    N, C, K = V.shape
    H, W = Q.shape[-2:]
    k, ok = slots(H, W, grid)
    out = torch.zeros(N, C, H, W, dtype=V.dtype)
    for j in range(9):
        out = out + (Q[:, j] * ok[j].to(V.dtype)).unsqueeze(1) * V[:, :, k[j].reshape(-1)].reshape(N, C, H, W)
    return out


def soft_labels(Q, grid):
    H, W = Q.shape[-2:]
    k, ok = slots(H, W, grid)
    q = torch.where(ok.unsqueeze(0), Q.detach(), torch.full_like(Q, float("-inf")))
    lab = torch.zeros(Q.shape[0], H, W, dtype=torch.int64)
    best = torch.full((Q.shape[0], H, W), float("-inf"), dtype=Q.dtype)
    for j in range(9):                                         # strictly greater: on a tie the lowest slot stays
        take = ok[j].unsqueeze(0) & (q[:, j] > best)
        lab = torch.where(take, k[j].unsqueeze(0).expand_as(lab), lab)
        best = torch.where(take, q[:, j], best)
    return lab.to(torch.int32)


def soft_slic(F, grid, max_iter=10):
    N, C, H, W = F.shape
    S = soft_pool(F, one_hot(N, H, W, F.dtype), grid)
    for _ in range(max_iter):
        Q = soft_assign(F, S, grid)
        new, w = soft_pool(F, Q, grid, return_weights=True)
        S = torch.where(w.unsqueeze(1) != 0, new, S)
    return soft_assign(F, S, grid), S


def with_coords(F, grid, compactness):
    N, C, H, W = F.shape
    s = float(compactness) * max(grid[0] / H, grid[1] / W)
    y = (torch.arange(H, dtype=F.dtype) * s).view(1, 1, H, 1).expand(N, 1, H, W)
    x = (torch.arange(W, dtype=F.dtype) * s).view(1, 1, 1, W).expand(N, 1, H, W)
    return torch.cat([F, y, x], 1)
