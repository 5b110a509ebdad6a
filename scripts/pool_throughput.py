"""Superpixel pooling throughput (fast_slic_amd/pool.py): device-event time per call of every forward and backward, its algorithmic bytes
(labels 2 B/px, features 4C B/px, the [N, C, K] outputs) against the 8 TB/s of the MI355X, and the same pooling written with torch
(`index_add_` + `bincount`) in torch's default mode and under torch.use_deterministic_algorithms(True).

    python scripts/pool_throughput.py [--reps 20] [--json out.json]

Label maps are Slic's on synthetic frames (one per frame of the batch).  Kernel names for a separate
`rocprofv3 --kernel-trace --stats` run: k_pool_tiles, k_pool_finalize, k_unpool."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fast_slic_amd import Slic                                    # noqa: E402
from fast_slic_amd.pool import superpixel_pool, superpixel_unpool  # noqa: E402
from fast_slic_amd.synth import variant                           # noqa: E402

HBM = 8.0e12
CONFIGS = [(8, 720, 1280, 1600, 3), (8, 720, 1280, 1600, 21), (8, 720, 1280, 1600, 64), (8, 2160, 3840, 6000, 21)]


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


def torch_pool(feat, lab, K, reduce):
    """The straightforward torch form: index_add_ of the valid pixels' channel vectors, bincount for the counts."""
    N, Cc, H, W = feat.shape
    flat = lab.view(N, H * W).long()
    ok = (flat >= 0) & (flat < K)
    idx = (flat + torch.arange(N, device=feat.device)[:, None] * K)[ok]
    rows = feat.permute(0, 2, 3, 1).reshape(N, H * W, Cc)[ok]
    out = torch.zeros(N * K, Cc, device=feat.device).index_add_(0, idx, rows)
    cnt = torch.bincount(idx, minlength=N * K)
    if reduce == "mean":
        out = out / cnt.clamp_min(1)[:, None]
    return out.view(N, K, Cc).transpose(1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--configs", default=None, help="indices into the config list, comma-separated")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    cfgs = CONFIGS if not args.configs else [CONFIGS[int(i)] for i in args.configs.split(",")]
    for N, H, W, K, Cc in cfgs:
        labs = np.stack([Slic(num_components=K).iterate(variant("A", H, W, seed=s)) for s in range(N)])
        lab = torch.from_numpy(labs).to(dev)
        feat = torch.randn(N, Cc, H, W, device=dev)
        px = N * H * W
        out_b = N * Cc * K * 4
        fwd_b = px * 2 + px * 4 * Cc + out_b
        unpool_b = px * 2 + px * 4 * Cc + out_b
        g = torch.randn(N, Cc, K, device=dev)
        gx = torch.randn(N, Cc, H, W, device=dev)
        res = {}
        for r in ("sum", "mean", "max"):
            res["fwd_" + r] = (timed(lambda: superpixel_pool(feat, lab, K, reduce=r), args.reps), fwd_b)
        vals = superpixel_pool(feat, lab, K, reduce="mean")
        res["unpool"] = (timed(lambda: superpixel_unpool(vals, lab), args.reps), unpool_b)
        for r in ("sum", "mean", "max"):
            x = feat.detach().requires_grad_(True)
            v = superpixel_pool(x, lab, K, reduce=r)
            res["bwd_" + r] = (timed(lambda: torch.autograd.grad(v, x, g, retain_graph=True), args.reps),
                               px * 2 + px * 4 * Cc + out_b * (2 if r == "max" else 1))
        vv = vals.detach().requires_grad_(True)
        y = superpixel_unpool(vv, lab)
        res["bwd_unpool"] = (timed(lambda: torch.autograd.grad(y, vv, gx, retain_graph=True), args.reps), fwd_b)
        for mode in ("default", "deterministic"):
            prev = torch.are_deterministic_algorithms_enabled()
            torch.use_deterministic_algorithms(mode == "deterministic")
            try:
                for r in ("sum", "mean"):
                    try:
                        res["torch_%s_%s" % (mode, r)] = (timed(lambda: torch_pool(feat, lab, K, r), max(3, args.reps // 4), 1), fwd_b)
                    except RuntimeError as e:
                        res["torch_%s_%s" % (mode, r)] = (None, str(e).splitlines()[0][:100])
            finally:
                torch.use_deterministic_algorithms(prev)
        print("N=%d %dx%d K=%d C=%d" % (N, W, H, K, Cc))
        for name, (us, b) in res.items():
            if us is None:
                print("   %-26s  %s" % (name, b))
                rows.append(dict(N=N, H=H, W=W, K=K, C=Cc, op=name, us=None, error=b))
                continue
            print("   %-26s %10.1f us  %8.1f MB  %6.2f TB/s  %5.2f of 8 TB/s" % (name, us, b / 1e6, b / us / 1e6, b / us / 1e6 / (HBM / 1e12)))
            rows.append(dict(N=N, H=H, W=W, K=K, C=Cc, op=name, us=us, bytes=b, frac_8tbs=b / us / 1e6 / (HBM / 1e12)))
        sys.stdout.flush()
        del feat, lab, g, gx
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
