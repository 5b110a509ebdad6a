"""Device time and peak memory of pixel_dot, pixel_softmax, pixel_mix and pixel_scatter (fast_slic_amd/pixels.py), forward and forward +
backward, beside the torch composition they replace, in the same process, by HIP events over warmed repetitions.

    python scripts/pixels_bench.py [--json OUT.json] [--frames N] [--reps R] [--windows C]

The map is slic_tensor's of N = 8 frames of 1280 x 720 with K = 1600 and the lists are those of its region adjacency graph; S = 9
slots, (C, Hd) in {8, 32} x {1, 4}.  The composition takes pixel_slots' [N, S, H, W] (computed once, outside the timed window, in its
favour), gathers the node table through it into [C, N, S, H, W], multiplies and sums; its scatter is zeros.index_add_ (float atomics),
its softmax torch's over the masked slots, and autograd gives its backwards.  The two forms alternate window by window.  The results
are compared first, within a tolerance (the composition adds in another order).  Peak memory is torch's max_memory_allocated over one
forward + backward, the gradients included, above what was allocated before it.  Beside the times the script prints the algorithmic
bytes of each call, the rate of a streaming copy of an [N, C, H, W] tensor in the same process, and each forward's bytes over its time
as a fraction of that rate.  DESIGN.md holds the figures."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from aggregate_bench import H, W, windows      # noqa: E402
from knn_bench import peak_bytes               # noqa: E402

K, S = 1600, 9
SHAPES = ((8, 1), (8, 4), (32, 1), (32, 4))      # C, Hd


def algorithmic_bytes(N, C, Hd):
    """What each call has to move at least: every pixel feature, per-slot value and result once, the int16 map once, the node table
    once; the scatter's accumulator is written (cleared) and read once."""
    px, slots, nodes, labels = 4 * N * C * H * W, 4 * N * Hd * S * H * W, 4 * N * C * K, 2 * N * H * W
    return {"dot": px + slots + nodes + labels, "softmax": 2 * slots + labels, "mix": px + slots + nodes + labels,
            "scatter": px + slots + labels + nodes + 2 * 56 * N * C * K, "an [N, C, H, W] tensor": px, "torch intermediate [C, N, S, H, W]": px * S}


def one_shape(labels, nl, N, C, Hd, reps, count):
    import torch
    from fast_slic_amd.pixels import pixel_dot, pixel_mix, pixel_scatter, pixel_slots, pixel_softmax
    dev, D = torch.device("cuda", 0), C // Hd
    gen = torch.Generator(device=dev).manual_seed(C + Hd)
    a = torch.randn((N, C, H, W), device=dev, generator=gen).requires_grad_()
    b = torch.randn((N, C, K), device=dev, generator=gen).requires_grad_()
    w = torch.randn((N, Hd, S, H, W), device=dev, generator=gen).requires_grad_()
    g_px, g_nodes = torch.randn((N, C, H, W), device=dev, generator=gen), torch.randn((N, C, K), device=dev, generator=gen)
    g_slots = torch.randn((N, Hd, S, H, W), device=dev, generator=gen)
    sl = pixel_slots(labels, nl, S)
    valid = sl >= 0                                                                     # [N, S, H, W]
    flat = (torch.arange(N, device=dev).view(N, 1, 1, 1) * K + sl.clamp(min=0)).reshape(-1)

    def at_nodes(t):                                                                    # [N, C, K] -> [C, N, S, H, W], 0 on empty slots
        return t.transpose(0, 1).reshape(C, N * K).index_select(1, flat).view(C, N, S, H, W) * valid

    def per_channel(t):                                                                 # [N, Hd, S, H, W] -> [C, N, S, H, W] (a view for D = 1)
        return t.transpose(0, 1).repeat_interleave(D, dim=0) if D > 1 else t.transpose(0, 1)

    def t_dot(a_, b_):
        return (a_.transpose(0, 1).unsqueeze(2) * at_nodes(b_)).view(Hd, D, N, S, H, W).sum(1).transpose(0, 1)

    def t_softmax(s_):
        return torch.nan_to_num(s_.masked_fill(~valid.unsqueeze(1), -float("inf")).softmax(2), nan=0.0)

    def t_mix(v_, w_):
        return (per_channel(w_) * at_nodes(v_)).sum(2).transpose(0, 1)

    def t_scatter(x_, w_):
        prod = (per_channel(w_) * x_.transpose(0, 1).unsqueeze(2) * valid).reshape(C, -1)
        return torch.zeros((C, N * K), device=dev).index_add_(1, flat, prod).view(C, N, K).transpose(0, 1)

    ours = {"dot": (lambda: pixel_dot(a, b, labels, nl, S, Hd), (a, b), g_slots),
            "softmax": (lambda: pixel_softmax(w, labels, nl), (w,), g_slots),
            "mix": (lambda: pixel_mix(b, w, labels, nl), (b, w), g_px),
            "scatter": (lambda: pixel_scatter(a, w, labels, nl, K), (a, w), g_nodes)}
    theirs = {"dot": (lambda: t_dot(a, b), (a, b), g_slots), "softmax": (lambda: t_softmax(w), (w,), g_slots),
              "mix": (lambda: t_mix(b, w), (b, w), g_px), "scatter": (lambda: t_scatter(a, w), (a, w), g_nodes)}

    def both(f):
        def run():
            for leaf in f[1]:
                leaf.grad = None
            f[0]().backward(f[2])
        return run

    with torch.no_grad():
        for n in ours:
            got, want = ours[n][0](), theirs[n][0]()
            diff = float((got - want).abs().max() / want.abs().max())
            assert got.shape == want.shape and diff < 1e-4, (n, diff)

    def peak(f):
        a.grad = b.grad = w.grad = None      # (a gradient left by the run before would be freed inside the measured call)
        return peak_bytes(both(f))

    bytes_ = algorithmic_bytes(N, C, Hd)
    res = dict(N=N, H=H, W=W, K=K, S=S, C=C, heads=Hd, nnz=int(nl.indices.shape[0]), bytes=bytes_,
               peak_bytes={"%s%s" % (who, n): peak(fs[n]) for who, fs in (("", ours), ("torch ", theirs)) for n in fs})
    print("N = %d, C = %d, heads = %d: bytes %s" % (N, C, Hd, bytes_), flush=True)
    copy_src, copy_dst = a.detach(), torch.empty_like(a)
    ts = {}
    for n in ours:
        with torch.no_grad():
            fwd = {"%s, forward" % n: ours[n][0], "torch %s, forward" % n: theirs[n][0]}
            if n == "dot":
                fwd["streaming copy of an [N, C, H, W] tensor"] = lambda: copy_dst.copy_(copy_src)
            ts.update(windows(fwd, reps, count))
        ts.update(windows({"%s, forward + backward" % n: both(ours[n]), "torch %s, forward + backward" % n: both(theirs[n])}, reps, count))
    med = {n: t[len(t) // 2] for n, t in ts.items()}
    rate = 2 * bytes_["an [N, C, H, W] tensor"] / med["streaming copy of an [N, C, H, W] tensor"] * 1e-6      # TB/s: bytes / us * 1e-6
    res["copy_rate_TB_per_s"] = round(rate, 3)
    for n, t in ts.items():
        print("  %-46s median %10.1f us (%.1f .. %.1f)   peak %s" % (n, med[n], t[0], t[-1], res["peak_bytes"].get(n.replace(", forward + backward", ""), "")), flush=True)
    res["fraction_of_copy_rate"] = {n: round(bytes_[n] / med["%s, forward" % n] * 1e-6 / rate, 3) for n in ours}
    print("  copy rate %.2f TB/s; forward calls at this fraction of it: %s" % (rate, res["fraction_of_copy_rate"]), flush=True)
    res["microseconds"] = {n: [round(v, 1) for v in t] for n, t in ts.items()}
    return res


def main():
    import torch
    from fast_slic_amd import Slic
    from fast_slic_amd.frames import slic_tensor
    from fast_slic_amd.propagate import neighbour_lists
    from fast_slic_amd.rag import superpixel_graph
    from fast_slic_amd.synth import variant
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    N = args.frames
    images = torch.from_numpy(np.stack([variant("A", H, W, seed=s) for s in range(N)])).to(torch.device("cuda", 0))
    labels = slic_tensor(images, Slic(num_components=K)).labels
    nl = neighbour_lists(superpixel_graph(labels, K))
    print("map %s %s, nnz = %d, largest degree %d" % (tuple(labels.shape), labels.dtype, int(nl.indices.shape[0]), int(nl.degree().max())), flush=True)
    results = [one_shape(labels, nl, N, C, Hd, args.reps, args.windows) for C, Hd in SHAPES]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
