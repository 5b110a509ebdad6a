"""Device time of the connectivity pass on label tensors (fast_slic_amd/connect.py): enforce_connectivity and connected_components on
an [8, 720, 1280] int32 soft_labels map (soft_slic on the synthetic frame with noise, grid 40 x 40, min_size 144), and on a constant
map, noise over 3 labels, all singletons, the same map as int16 / int64 and one frame of it.

    python scripts/connect_throughput.py events [--json OUT.json]    # HIP events over warmed repetitions: 7 windows of up to 100 calls
    rocprofv3 --kernel-trace --stats -f csv -d OUT -- python scripts/connect_throughput.py calls
                                                                      # the soft_labels map alone, few calls: a kernel trace of its own

`events` first checks frame 0 of the result against the model of the rules (tests/connect_ref.py).  The bytes the pass must move are
the label read and the label written, 8 B/px for an int32 map; DESIGN.md sets the times against that and against what the eight
launches move."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, H, W, GRID, MIN_SIZE = 8, 720, 1280, (40, 40), 144


def soft_map(dev):
    import torch
    from fast_slic_amd.soft import soft_labels, soft_slic, with_coords
    from fast_slic_amd.synth import variant
    img = torch.from_numpy(variant("A", H, W).astype(np.float32) / 255.0).permute(2, 0, 1)
    g = torch.Generator().manual_seed(1)
    feat = (img.unsqueeze(0) * 4.0 + 0.15 * torch.randn(N, 3, H, W, generator=g)).to(dev)
    q, _ = soft_slic(with_coords(feat, GRID, 0.5), GRID, max_iter=5)
    return soft_labels(q, GRID)


def timed(fn, reps, windows):
    """Sorted per-call times in microseconds, one per window of `reps` calls between two HIP events (fewer calls for a slow map)."""
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.time()
    fn()
    torch.cuda.synchronize()
    reps = max(3, min(reps, int(0.1 / max(time.time() - t0, 1e-6))))
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / reps)
    return sorted(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["events", "calls"])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import connect_ref as R
    from fast_slic_amd.connect import connected_components, enforce_connectivity
    dev = torch.device("cuda", 0)
    lab = soft_map(dev)
    out, n = enforce_connectivity(lab, MIN_SIZE)
    _, nc = connected_components(lab)
    torch.cuda.synchronize()
    res = dict(shape=[N, H, W], grid=list(GRID), min_size=MIN_SIZE, components=nc.tolist(), n=n.tolist(), bound=H * W // MIN_SIZE)
    print(res, flush=True)
    maps = {"soft_labels": lab}
    reps, windows = 3, 1
    if args.mode == "events":
        want, want_n = R.enforce(lab[0].cpu().numpy(), MIN_SIZE)
        assert np.array_equal(out[0].cpu().numpy(), want) and int(n[0]) == want_n, "frame 0 differs from the model"
        print("frame 0 equals the model", flush=True)
        reps, windows = 100, 7
        maps["constant"] = torch.zeros((N, H, W), dtype=torch.int32, device=dev)
        maps["noise over 3 labels"] = torch.randint(0, 3, (N, H, W), dtype=torch.int32, device=dev)
        maps["singletons"] = torch.arange(N * H * W, dtype=torch.int32, device=dev).view(N, H, W)
        maps["soft_labels int64"] = lab.to(torch.int64)
        maps["soft_labels int16"] = lab.to(torch.int16)
        maps["soft_labels, one frame"] = lab[:1].contiguous()
    for name, m in maps.items():
        te = timed(lambda: enforce_connectivity(m, MIN_SIZE), reps, windows)
        tc = timed(lambda: connected_components(m), reps, windows)
        res[name] = dict(enforce_us=[round(t, 1) for t in te], components_us=[round(t, 1) for t in tc], pixels=m.numel())
        print("%-24s enforce_connectivity median %7.1f us (%.1f .. %.1f)   connected_components median %7.1f us"
              % (name, te[len(te) // 2], te[0], te[-1], tc[len(tc) // 2]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
