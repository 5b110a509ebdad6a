"""Soft superpixel assignment throughput (fast_slic_amd/soft.py): device-event time per call of every kernel and of every public
forward and backward, each kernel's algorithmic bytes (features 4C B/px, the nine Q planes 36 B/px, the [N, C, K] tables) against the
8 TB/s of the MI355X, and the same functions written with plain torch (gathers and `index_add_` over the nine slots, autograd for the
backwards).

    python scripts/soft_throughput.py [--reps 20] [--json out.json]

Kernel names for a separate `rocprofv3 --kernel-trace --stats` run: k_soft_assign, k_soft_assign_bwd, k_soft_pool, k_soft_unpool,
k_soft_dot."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fast_slic_amd import soft as S                               # noqa: E402

HBM = 8.0e12
CONFIGS = [(8, 720, 1280, (40, 40), 5), (8, 720, 1280, (40, 40), 20)]


def timed(fn, reps, warmup=3):
    """Median device time (us) of fn() on the current stream, CUDA events around each call."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


# ---- the plain-torch formulation ----
def torch_assign(F, Sc, k, ok):
    N, Cc, H, W = F.shape
    d = torch.stack([((F - Sc[:, :, k[j].reshape(-1)].reshape(N, Cc, H, W)) ** 2).sum(1) for j in range(9)], 1)
    d = torch.where(ok.unsqueeze(0), d, torch.full_like(d, float("inf")))
    return torch.softmax(-d, dim=1)


def torch_pool(F, Q, k, ok, K):
    N, Cc, H, W = F.shape
    sums = torch.zeros(N, Cc, K, device=F.device)
    weights = torch.zeros(N, K, device=F.device)
    for j in range(9):
        w = Q[:, j] * ok[j]
        sums = sums.index_add(2, k[j].reshape(-1), (w.unsqueeze(1) * F).reshape(N, Cc, H * W))
        weights = weights.index_add(1, k[j].reshape(-1), w.reshape(N, H * W))
    return sums, weights


def torch_unpool(V, Q, k, ok):
    N, Cc, _ = V.shape
    H, W = Q.shape[-2:]
    out = torch.zeros(N, Cc, H, W, device=V.device)
    for j in range(9):
        out = out + (Q[:, j] * ok[j]).unsqueeze(1) * V[:, :, k[j].reshape(-1)].reshape(N, Cc, H, W)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--configs", default=None, help="indices into the config list, comma-separated")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    cfgs = CONFIGS if not args.configs else [CONFIGS[int(i)] for i in args.configs.split(",")]
    for N, H, W, grid, Cc in cfgs:
        K = grid[0] * grid[1]
        px = N * H * W
        fb, qb, tb = px * 4 * Cc, px * 36, N * Cc * K * 4
        F = torch.randn(N, Cc, H, W, device=dev) * 0.5
        q1 = torch.zeros(N, 9, H, W, device=dev)
        q1[:, 4] = 1.0
        cen = S.soft_pool(F, q1, grid) + torch.randn(N, Cc, K, device=dev) * (0.6 / Cc ** 0.5)
        Q = S.soft_assign(F, cen, grid)
        gQ, gS, gW, gO = torch.randn_like(Q), torch.randn(N, Cc, K, device=dev), torch.randn(N, K, device=dev), torch.randn_like(F)
        gd, gF = torch.empty_like(Q), torch.empty_like(F)
        lib = S.T.library(*S._ENTRY)
        geom = S._geom(F, N, Cc, H, W, grid)
        res = {}
        # the kernels, one launch each
        res["k_soft_assign"] = (timed(lambda: S._assign_raw(F, cen, grid), args.reps), fb + tb + qb)
        res["k_soft_assign_bwd"] = (timed(lambda: lib.fslic_hip_soft_assign_backward(*geom, F.data_ptr(), cen.data_ptr(), Q.data_ptr(),
                                                                                    gQ.data_ptr(), gd.data_ptr(), gF.data_ptr()), args.reps),
                                    2 * fb + tb + 3 * qb)
        res["k_soft_pool"] = (timed(lambda: S._pool_raw(F, Q, grid), args.reps), fb + qb + tb + N * K * 4)
        res["k_soft_pool centred"] = (timed(lambda: S._pool_raw(F, Q, grid, centres=cen, weights=False), args.reps), fb + qb + 2 * tb)
        res["k_soft_unpool"] = (timed(lambda: S._unpool_raw(cen, Q, grid), args.reps), fb + qb + tb)
        res["k_soft_dot"] = (timed(lambda: S._dot_raw(F, gS, gW, grid), args.reps), fb + qb + tb + N * K * 4)
        # the public functions: forward, then backward alone (autograd.grad on a kept graph)
        x, s, q, v = (t.detach().requires_grad_(True) for t in (F, cen, Q, cen))
        res["soft_assign fwd"] = (timed(lambda: S.soft_assign(F, cen, grid), args.reps), None)
        y = S.soft_assign(x, s, grid)
        res["soft_assign bwd"] = (timed(lambda: torch.autograd.grad(y, (x, s), gQ, retain_graph=True), args.reps), None)
        res["soft_pool fwd"] = (timed(lambda: S.soft_pool(F, Q, grid), args.reps), None)
        y2 = S.soft_pool(x, q, grid)
        res["soft_pool bwd"] = (timed(lambda: torch.autograd.grad(y2, (x, q), gS, retain_graph=True), args.reps), None)
        res["soft_unpool fwd"] = (timed(lambda: S.soft_unpool(cen, Q, grid), args.reps), None)
        y3 = S.soft_unpool(v, q, grid)
        res["soft_unpool bwd"] = (timed(lambda: torch.autograd.grad(y3, (v, q), gO, retain_graph=True), args.reps), None)
        res["soft_slic max_iter=10"] = (timed(lambda: S.soft_slic(F, grid, max_iter=10), max(3, args.reps // 4), 1), None)
        del y, y2, y3
        # plain torch
        k, ok = S._slots(H, W, grid[0], grid[1], dev)
        treps = max(3, args.reps // 4)
        try:
            res["torch assign fwd"] = (timed(lambda: torch_assign(F, cen, k, ok), treps, 1), None)
            t = torch_assign(x, s, k, ok)
            res["torch assign bwd"] = (timed(lambda: torch.autograd.grad(t, (x, s), gQ, retain_graph=True), treps, 1), None)
            del t
            res["torch pool fwd"] = (timed(lambda: torch_pool(F, Q, k, ok, K), treps, 1), None)
            t = torch_pool(x, q, k, ok, K)
            res["torch pool bwd"] = (timed(lambda: torch.autograd.grad(t, (x, q), (gS, gW), retain_graph=True), treps, 1), None)
            del t
            res["torch unpool fwd"] = (timed(lambda: torch_unpool(cen, Q, k, ok), treps, 1), None)
            t = torch_unpool(v, q, k, ok)
            res["torch unpool bwd"] = (timed(lambda: torch.autograd.grad(t, (v, q), gO, retain_graph=True), treps, 1), None)
            del t
        except RuntimeError as e:
            res["torch"] = (None, str(e).splitlines()[0][:100])
        print("N=%d %dx%d grid=%dx%d C=%d" % (N, W, H, grid[0], grid[1], Cc))
        for name, (us, b) in res.items():
            if us is None:
                print("   %-26s  %s" % (name, b))
                rows.append(dict(N=N, H=H, W=W, K=K, C=Cc, op=name, us=None, error=b))
            elif b is None:
                print("   %-26s %10.1f us" % (name, us))
                rows.append(dict(N=N, H=H, W=W, K=K, C=Cc, op=name, us=us))
            else:
                print("   %-26s %10.1f us  %8.1f MB  %6.2f TB/s  %5.2f of 8 TB/s" % (name, us, b / 1e6, b / us / 1e6, b / us / 1e6 / (HBM / 1e12)))
                rows.append(dict(N=N, H=H, W=W, K=K, C=Cc, op=name, us=us, bytes=b, frac_8tbs=b / us / 1e6 / (HBM / 1e12)))
        sys.stdout.flush()
        del F, Q, gQ, gO, gd, gF, x, s, q, v
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
