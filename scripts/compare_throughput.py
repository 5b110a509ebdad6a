"""Throughput of the comparison of two label maps (fast_slic_amd/compare.py): Slic K = 1600 against LSC K = 1600 maps of the
synthetic frames, int16, 8 x 1280x720 and 8 x 3840x2160.

    python scripts/compare_throughput.py maps DIR                # the maps, once: DIR/maps_<H>.npz
    rocprofv3 --kernel-trace --stats -f csv -d OUT -- python scripts/compare_throughput.py calls DIR --height 720 [--reps 10]
                                                                  # the calls alone, for a counter-free kernel trace of their own
    python scripts/compare_throughput.py trace OUT --reps 10     # per kernel the durations of that trace, the first call discarded
    python scripts/compare_throughput.py events DIR [--reps 20]  # by HIP events: the whole calls, the torch.unique formulation of
                                                                  # the same table, and the box's streaming-copy rate

`calls` runs, in this order, 1 + reps times each: label_overlap, boundary_match at tolerance 0, at tolerance 11, superpixel_graph
(connectivity 4, no image: k_rag_tiles on the same bytes of one map).  `trace` relies on that order to tell the two tolerances apart.
The byte floor of a kernel is the bytes it must read (2 B/px a map) over the measured copy rate (bytes read + written per second)."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {720: (8, 720, 1280), 2160: (8, 2160, 3840)}
K = 1600
TOLERANCES = (0, 11)


def make_maps(out):
    from fast_slic_amd import LSC, Slic
    from fast_slic_amd.synth import variant
    os.makedirs(out, exist_ok=True)
    for key, (N, H, W) in SIZES.items():
        frames = [variant("A", H, W, seed=s) for s in range(N)]
        slic, lsc = Slic(num_components=K), LSC(num_components=K)
        np.savez(os.path.join(out, "maps_%d.npz" % key), slic=np.stack([slic.iterate(f) for f in frames]),
                 lsc=np.stack([lsc.iterate(f) for f in frames]))
        print("maps %dx%d x %d written" % (W, H, N))


def load_maps(d, key):
    import torch
    z = np.load(os.path.join(d, "maps_%d.npz" % key))
    dev = torch.device("cuda", 0)
    return torch.from_numpy(z["slic"]).to(dev), torch.from_numpy(z["lsc"]).to(dev)


def calls(d, key, reps):
    import torch
    from fast_slic_amd.compare import boundary_match, label_overlap
    from fast_slic_amd.rag import superpixel_graph
    a, b = load_maps(d, key)
    for fn in ([lambda: label_overlap(a, b, K, K)] + [lambda t=t: boundary_match(a, b, t) for t in TOLERANCES]
               + [lambda: superpixel_graph(a, K)]):
        for _ in range(1 + reps):
            fn()
        torch.cuda.synchronize()
    t = label_overlap(a, b, K, K)
    print("pairs %d capacity %d best_overlap %s" % (t.pairs.shape[1], t.capacity, t.best_overlap().tolist()))
    print("boundary_match", [boundary_match(a, b, tol).sum(0).tolist() for tol in TOLERANCES])


def trace(out, reps):
    rows = []
    for fn in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn) as f:
            rows += [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    result = {}
    for name in ("k_overlap_tiles", "k_pair_compact<false>", "k_boundary_match", "k_rag_tiles", "k_pair_compact<true>"):
        d = [(e - s) / 1e3 for n, s, e in rows if name in n]
        parts = {name: d}
        if name == "k_boundary_match":
            assert len(d) == len(TOLERANCES) * (1 + reps) + len(TOLERANCES), len(d)      # and one more call each for the printout
            parts = {"%s tolerance %d" % (name, t): d[i * (1 + reps):(i + 1) * (1 + reps)] for i, t in enumerate(TOLERANCES)}
        for what, v in parts.items():
            v = v[1:1 + reps]                                                            # the first call discarded
            if v:
                result[what] = dict(n=len(v), median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)))
                print("%-34s n=%3d  median %9.2f us  min %9.2f  max %9.2f" % (what, len(v), np.median(v), min(v), max(v)))
    return result


def event_time(fn, reps, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return float(np.median(ts)), float(min(ts))


def events(d, reps):
    import torch
    from fast_slic_amd import Engine
    from fast_slic_amd.compare import boundary_match, label_overlap
    engine = Engine(0, 1)
    rate = engine.copy_bandwidth()                                      # GB/s, bytes read + written
    engine.close()
    print("streaming copy %.0f GB/s" % rate)
    result = dict(copy_gbs=rate)
    for key, (N, H, W) in SIZES.items():
        a, b = load_maps(d, key)
        px = N * H * W
        floor = px * 4 / (rate * 1e3)                                   # us: two int16 maps read once
        print("%d x %dx%d: %.1f MB of maps, byte floor %.1f us (one map: %.1f us)" % (N, W, H, px * 4 / 1e6, floor, floor / 2))

        def unique():
            key64 = (a.to(torch.int64) * K + b.to(torch.int64))[(a >= 0) & (b >= 0)]
            frame = torch.arange(N, device=a.device).view(N, 1, 1).expand_as(a)[(a >= 0) & (b >= 0)]
            return torch.unique(frame * (K * K) + key64, return_counts=True)
        got = unique()
        t = label_overlap(a, b, K, K)
        assert got[0].shape[0] == t.pairs.shape[1] and torch.equal(got[1].to(torch.int32), t.count)
        rows = {"label_overlap, whole call": lambda: label_overlap(a, b, K, K), "torch.unique(..., return_counts=True)": unique}
        for tol in TOLERANCES:
            rows["boundary_match tolerance %d, whole call" % tol] = lambda tol=tol: boundary_match(a, b, tol)
        result[str(key)] = dict(floor_us=floor)
        for what, fn in rows.items():
            med, mn = event_time(fn, reps)
            result[str(key)][what] = dict(median_us=med, min_us=mn)
            print("   %-44s median %10.1f us  min %10.1f us" % (what, med, mn))
        del a, b, got, t
        torch.cuda.empty_cache()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["maps", "calls", "trace", "events"])
    ap.add_argument("dir")
    ap.add_argument("--height", type=int, default=720, choices=sorted(SIZES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    result = None
    if args.mode == "maps":
        make_maps(args.dir)
    elif args.mode == "calls":
        calls(args.dir, args.height, args.reps)
    elif args.mode == "trace":
        result = trace(args.dir, args.reps)
    else:
        result = events(args.dir, args.reps)
    if args.json and result is not None:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
