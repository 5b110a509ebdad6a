"""Device time of merging on the region adjacency graph (fast_slic_amd/merge.py), by HIP events over warmed repetitions.

    python scripts/merge_timing.py [--json OUT.json]

merge_labels on an [8, 2160, 3840] int16 map with K = 1600 against the torch expression it replaces
(torch.where(ok, mapping[f, labels.long().clamp(0, K - 1)], -1)) on the same inputs, and against the plain-copy rate of the GPU
(Engine.copy_bandwidth): the pass must move 2 B read and 4 B written a pixel.  Then, for K = 1600 and K = 6000 graphs of the 8
frames (a jittered grid of K cells, with an image), the microseconds a call of best_neighbour_edges, merge_components,
compose_mappings and contract_graph, and of the superpixel_graph on the merged map that contract_graph saves.  Every result is first
checked against the torch expression or the identity contract_graph == superpixel_graph(merge_labels).  DESIGN.md holds the figures."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W = 8, 2160, 3840
GRIDS = {1600: (40, 40), 6000: (60, 100)}            # K: cells down, across


def timed(fn, reps=20, windows=7):
    """Sorted per-call times in microseconds, one per window of `reps` calls between two HIP events (fewer calls for a slow one)."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.time()
    fn()
    torch.cuda.synchronize()
    reps = max(3, min(reps, int(0.2 / max(time.time() - t0, 1e-6))))
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


def grid_map(K, dev):
    """int16 [N, H, W]: a grid of K cells whose edges wobble, a different phase per frame."""
    import torch
    gy, gx = GRIDS[K]
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    frames = []
    for n in range(N):
        yy = (y + 6.0 * torch.sin(x / 13.0 + n)).clamp(0, H - 1)
        xx = (x + 6.0 * torch.sin(y / 17.0 + 2 * n)).clamp(0, W - 1)
        frames.append(((yy * gy / H).long().clamp(0, gy - 1) * gx + (xx * gx / W).long().clamp(0, gx - 1)).to(torch.int16))
    return torch.stack(frames)


def torch_expression(labels, mapping, K):
    import torch
    l64 = labels.long()
    ok = (l64 >= 0) & (l64 < K)
    picked = torch.gather(mapping, 1, l64.clamp(0, K - 1).view(labels.shape[0], -1)).view(labels.shape)
    return torch.where(ok, picked, torch.full_like(picked, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from fast_slic_amd import Engine
    from fast_slic_amd.merge import best_neighbour_edges, compose_mappings, contract_graph, merge_components, merge_labels
    from fast_slic_amd.pool import superpixel_pool
    from fast_slic_amd.rag import superpixel_graph
    dev = torch.device("cuda", 0)
    res = dict(shape=[N, H, W])
    res["copy_GBps"] = Engine(0, 1).copy_bandwidth()
    print("plain copy %.0f GB/s" % res["copy_GBps"], flush=True)
    gen = torch.Generator(device=dev).manual_seed(1)
    image = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    med = lambda ts: ts[len(ts) // 2]
    for K in GRIDS:
        labels = grid_map(K, dev)
        g = superpixel_graph(labels, K, image=image)
        counts = superpixel_pool(torch.zeros((N, 1, H, W), device=dev), labels, K, reduce="sum", return_counts=True)[1]
        value = torch.rand((N, K), device=dev, generator=gen)
        a, b = g.edge_index
        frame = torch.searchsorted(g.offsets[1:].contiguous(), torch.arange(a.numel(), device=dev), right=True)
        w = (value[frame, a] - value[frame, b]).abs()
        join = best_neighbour_edges(g, w, 0.25)
        mapping, n = merge_components(g, join, counts)
        coarse = merge_labels(labels, mapping)
        assert torch.equal(coarse, torch_expression(labels, mapping, K)), "merge_labels differs from the torch expression"
        small, direct = contract_graph(g, mapping, K), superpixel_graph(coarse, K, image=image)
        assert all(torch.equal(p, q) for p, q in ((small.edge_index, direct.edge_index), (small.boundary, direct.boundary),
                                                    (small.contrast, direct.contrast), (small.offsets, direct.offsets))), "the identity fails"
        r = dict(edges=int(a.numel()), groups=n.tolist(), edges_after=int(small.edge_index.shape[1]))
        calls = {"best_neighbour_edges": lambda: best_neighbour_edges(g, w, 0.25), "merge_components": lambda: merge_components(g, join, counts),
                 "compose_mappings": lambda: compose_mappings(mapping, mapping), "contract_graph": lambda: contract_graph(g, mapping, K),
                 "superpixel_graph of the merged map": lambda: superpixel_graph(coarse, K, image=image),
                 "merge_labels": lambda: merge_labels(labels, mapping)}
        if K == 1600:
            calls["the torch expression"] = lambda: torch_expression(labels, mapping, K)
        for name, fn in calls.items():
            ts = timed(fn)
            r[name] = [round(t, 1) for t in ts]
            print("K = %4d  %-36s median %9.1f us (%.1f .. %.1f)" % (K, name, med(ts), ts[0], ts[-1]), flush=True)
        t = med(r["merge_labels"]) * 1e-6
        r["merge_labels_GBps"] = 6.0 * N * H * W / t / 1e9
        print("K = %4d  merge_labels moves 6 B/px at %.0f GB/s, %.0f %% of the plain copy" % (K, r["merge_labels_GBps"], 100 * r["merge_labels_GBps"] / res["copy_GBps"]), flush=True)
        res[str(K)] = r
        del labels, g, coarse, small, direct
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
