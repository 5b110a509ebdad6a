"""Device time of one merging round by similarity (fast_slic_amd/regions.py) beside the torch loop it replaces, by HIP events over
warmed repetitions.

    python scripts/region_timing.py [--json OUT.json]

N = 8 frames of 1280 x 720, Slic maps of K = 1600, the image's three channels as features.  One round of merge_hierarchical (weights,
best edges, components, contraction, group sums) against one round of the README's former loop on the same inputs (searchsorted, two
gathers and a norm for the weights; scatter_add_ on float32 for the sums), the two alternating window by window; then the parts
that differ, each beside its torch form.  The results are compared first: the same mapping, the same counts, and sums that agree
(bit for bit here, where the features are integers).  DESIGN.md holds the figures."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W, K = 8, 720, 1280, 1600


def windows(fns, reps=20, count=9):
    """Per function the sorted per-call microseconds of `count` windows of `reps` calls between two HIP events; the functions
    alternate window by window, after three warm-up calls each."""
    import torch
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(count):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / reps)
    return {name: sorted(ts) for name, ts in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from fast_slic_amd import Slic
    from fast_slic_amd.merge import best_neighbour_edges, contract_graph, merge_components
    from fast_slic_amd.pool import superpixel_pool
    from fast_slic_amd.rag import superpixel_graph
    from fast_slic_amd.regions import edge_weights, group_sums, merge_hierarchical
    from fast_slic_amd.synth import variant
    dev = torch.device("cuda", 0)
    frames = [variant("A", H, W, seed=s) for s in range(N)]
    slic = Slic(num_components=K)
    labels = torch.from_numpy(np.stack([slic.iterate(f) for f in frames])).to(dev)
    image = torch.from_numpy(np.stack(frames)).to(dev)
    features = image.permute(0, 3, 1, 2).float().contiguous()
    g = superpixel_graph(labels, K, image=image)
    sums, counts = superpixel_pool(features, labels, K, reduce="sum", return_counts=True)
    E = int(g.edge_index.shape[1])

    def torch_weights(g, sums, counts):
        a, b = g.edge_index
        frame = torch.searchsorted(g.offsets[1:].contiguous(), torch.arange(a.numel(), device=a.device), right=True)
        mean = sums / counts.clamp_min(1).unsqueeze(1)
        return (mean[frame, :, a] - mean[frame, :, b]).norm(dim=1)

    def torch_sums(sums, counts, mapping):
        idx = mapping.clamp_min(0).long()
        return (torch.zeros_like(sums).scatter_add_(2, idx.unsqueeze(1).expand_as(sums), sums),
                torch.zeros_like(counts).scatter_add_(1, idx, counts))

    w = edge_weights(g, sums, counts)
    threshold = float(w[torch.isfinite(w)].median())                       # half of the edges are eligible

    def torch_round():
        wt = torch_weights(g, sums, counts)
        mapping, n = merge_components(g, best_neighbour_edges(g, wt, threshold), members=counts)
        return mapping, n, contract_graph(g, mapping, K), torch_sums(sums, counts, mapping)

    def new_round():
        return merge_hierarchical(g, sums, counts, threshold=threshold, max_rounds=1)

    res, (mapping, n, g2, (tsums, tcounts)) = new_round(), torch_round()
    wt = torch_weights(g, sums, counts)
    res_w = dict(edges=E, threshold=threshold, groups=res.n.tolist(), edges_after=int(res.graph.edge_index.shape[1]),
                 weights_equal_bits=bool(torch.equal(w.view(torch.int32), wt.view(torch.int32))),
                 weights_max_abs_diff=float((w - wt).abs().max()), same_mapping=bool(torch.equal(res.mapping, mapping)),
                 same_counts=bool(torch.equal(res.counts, tcounts)), sums_equal_bits=bool(torch.equal(res.sums.view(torch.int32), tsums.view(torch.int32))))
    print(res_w, flush=True)
    assert res_w["same_counts"] or not res_w["same_mapping"]
    join = best_neighbour_edges(g, w, threshold)
    ts = windows({"merge_hierarchical, one round": new_round, "the torch loop, one round": torch_round})
    ts.update(windows({"edge_weights": lambda: edge_weights(g, sums, counts), "the torch weights": lambda: torch_weights(g, sums, counts)}))
    ts.update(windows({"group_sums": lambda: group_sums(sums, res.mapping, K, counts), "the torch scatter_add_": lambda: torch_sums(sums, counts, res.mapping)}))
    ts.update(windows({"best_neighbour_edges": lambda: best_neighbour_edges(g, w, threshold), "merge_components": lambda: merge_components(g, join, counts),
                       "contract_graph": lambda: contract_graph(g, res.mapping, K)}))
    for name, t in ts.items():
        print("%-32s median %8.1f us (%.1f .. %.1f)" % (name, t[len(t) // 2], t[0], t[-1]), flush=True)
    res_w["microseconds"] = {name: [round(v, 1) for v in t] for name, t in ts.items()}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res_w, f, indent=1)


if __name__ == "__main__":
    main()
