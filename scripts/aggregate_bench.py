"""Device time of graph_aggregate(reduce="sum", weight=w) (fast_slic_amd/propagate.py), forward and forward + backward, beside the torch
composition it replaces, by HIP events over warmed repetitions.

    python scripts/aggregate_bench.py [--json OUT.json]

The graphs are those of slic_tensor maps of 1280 x 720 frames, at two sizes: N = 8, C = 64, K = 1600 and N = 16, C = 256, K = 6000.
The baseline on the same values, laid out [C, N K] so that one flat index serves every frame: xf[:, src] * w, then index_add_ over the
rows (a [C, nnz] intermediate and float atomics); its backward is autograd's.  The two forms alternate window by window.  Each
backward launch is also timed alone, through a result with one differentiable input.  The results are compared first (the composition
adds in another order: a tolerance, not bits).  Beside the times the script prints the
algorithmic bytes of each launch and the time a streaming copy of as many bytes as the forward's values and result takes.
DESIGN.md holds the figures."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 720, 1280
SIZES = [(8, 64, 1600), (16, 256, 6000)]


def windows(fns, reps, count=9):
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


def algorithmic_bytes(N, C, K, nnz):
    """What each launch has to move at least: every value, gradient and result once, the lists once per 32 channels of an item."""
    cells, groups = 4 * N * C * K, (C + 31) // 32
    return {"forward": 2 * cells + groups * (8 * nnz + 8 * N * K), "backward_values": 2 * cells + groups * (16 * nnz + 8 * N * K),
            "backward_weight": 12 * nnz + 2 * cells, "torch intermediate [C, nnz]": 4 * C * nnz}


def one_size(N, C, K, reps):
    import torch
    from fast_slic_amd import Slic
    from fast_slic_amd.frames import slic_tensor
    from fast_slic_amd.propagate import graph_aggregate, neighbour_lists
    from fast_slic_amd.rag import superpixel_graph
    from fast_slic_amd.synth import variant
    dev = torch.device("cuda", 0)
    images = torch.from_numpy(np.stack([variant("A", H, W, seed=s) for s in range(N)])).to(dev)
    labels = slic_tensor(images, Slic(num_components=K)).labels
    nl = neighbour_lists(superpixel_graph(labels, K))
    nl.transposed()
    nnz = int(nl.indices.shape[0])
    gen = torch.Generator(device=dev).manual_seed(K)
    x = torch.randn((N, C, K), device=dev, generator=gen).requires_grad_()
    w = torch.rand(nnz, device=dev, generator=gen).requires_grad_()
    g = torch.randn((N, C, K), device=dev, generator=gen)
    rows = nl.rows.long()
    src = torch.div(rows, K, rounding_mode="floor") * K + nl.indices.long()      # the flat (frame, node) of every entry's neighbour

    def flat(t):
        return t.detach().transpose(0, 1).reshape(C, N * K).contiguous()   # [C, N K]: the rows over (frame, node) innermost

    xf, gf = flat(x).requires_grad_(), flat(g)

    def torch_forward(xf, w):
        return torch.zeros_like(xf).index_add_(1, rows, xf[:, src] * w)

    def backward_of(fn, x, g):
        def run():
            x.grad = w.grad = None
            fn(x, w).backward(g)
        return run

    y, yt = graph_aggregate(x, nl, w), torch_forward(xf, w)
    y.backward(g)
    gx, gw = x.grad, w.grad
    backward_of(torch_forward, xf, gf)()
    res = dict(N=N, C=C, K=K, nnz=nnz, max_degree=int(nl.degree().max()), bytes=algorithmic_bytes(N, C, K, nnz),
               max_abs_diff=dict(y=float((flat(y) - yt.detach()).abs().max()), grad_values=float((flat(gx) - xf.grad).abs().max()), grad_weight=float((gw - w.grad).abs().max())))
    assert res["max_abs_diff"]["y"] < 1e-4 and res["max_abs_diff"]["grad_values"] < 1e-4 and res["max_abs_diff"]["grad_weight"] < 1e-2 * C ** 0.5
    copy_src, copy_dst = x.detach(), torch.empty_like(x)
    with torch.no_grad():
        ts = windows({"graph_aggregate, forward": lambda: graph_aggregate(x, nl, w), "torch composition, forward": lambda: torch_forward(xf, w),
                      "streaming copy of the values": lambda: copy_dst.copy_(copy_src)}, reps)
    ts.update(windows({"graph_aggregate, forward + backward": backward_of(lambda x, w: graph_aggregate(x, nl, w), x, g),
                       "torch composition, forward + backward": backward_of(torch_forward, xf, gf)}, reps))
    # each backward launch alone: a result whose only differentiable input is the one in question, its graph kept
    y_x, y_w = graph_aggregate(x, nl, w.detach()), graph_aggregate(x.detach(), nl, w)
    ts.update(windows({"backward to the values alone": lambda: torch.autograd.grad(y_x, x, g, retain_graph=True),
                       "backward to the weights alone": lambda: torch.autograd.grad(y_w, w, g, retain_graph=True)}, reps))
    print("N = %d, C = %d, K = %d: nnz = %d, largest degree %d, bytes %s, differences %s" % (N, C, K, nnz, res["max_degree"], res["bytes"], res["max_abs_diff"]), flush=True)
    for name, t in ts.items():
        print("  %-40s median %9.1f us (%.1f .. %.1f)" % (name, t[len(t) // 2], t[0], t[-1]), flush=True)
    res["microseconds"] = {name: [round(v, 1) for v in t] for name, t in ts.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    results = [one_size(N, C, K, reps) for (N, C, K), reps in zip(SIZES, (50, 10))]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
