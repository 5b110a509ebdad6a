"""Device time and peak memory of entry_gather and entry_reduce (fast_slic_amd/messages.py), forward and forward + backward, beside the
torch composition they replace, in the same process, by HIP events over warmed repetitions.

    python scripts/messages_bench.py [--json OUT.json]

The lists are those of the region adjacency graph of slic_tensor maps of N = 8 frames of 1280 x 720 with K = 1600, and the fixed-degree
lists of knn_graph with k = 16 on the same nodes (no padding: every entry is valid), each with F = 8 and F = 64 features.  The
composition works on the same values laid out [F, N K], so that one flat index serves every frame: x[..., idx] (index_select) for a
gather, whose backward is index_add_ (float atomics); zeros.index_add_ for the sum and scatter_reduce("amax") for the max, autograd's
backward for both.  The two forms alternate window by window.  The results are compared first: the gather and the max bit for bit, the
sum within a tolerance (the composition adds in another order).  Peak memory is torch's max_memory_allocated over one forward +
backward, above what was allocated before it.  Beside the times the script prints the algorithmic bytes of each launch, the rate of a
streaming copy of a [F, nnz] tensor in the same process, and each forward launch's bytes over its time as a fraction of that rate.
DESIGN.md holds the figures."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from aggregate_bench import windows      # noqa: E402
from attention_bench import graph_of     # noqa: E402
from knn_bench import peak_bytes         # noqa: E402

N, K, KNN = 8, 1600, 16
FEATURES = (8, 64)
REPS = 20


def algorithmic_bytes(Fc, nnz):
    """What each launch has to move at least: every value, message and result once; rows and indices once per (feature, entry) thread
    of the gather (as attention_bench counts the dot); offsets and indices (transposed: entries and rows) once per four features of
    the reduce."""
    cells, R, groups = 4 * N * Fc * K, N * K, (Fc + 3) // 4
    return {"gather": cells + 12 * Fc * nnz, "reduce": cells + 4 * Fc * nnz + groups * (4 * nnz + 8 * R),
            "reduce to source": cells + 4 * Fc * nnz + groups * (8 * nnz + 8 * R), "a [F, nnz] tensor": 4 * Fc * nnz}


def one_case(name, nl, Fc):
    import torch
    from fast_slic_amd.messages import entry_gather, entry_reduce
    dev, R = torch.device("cuda", 0), N * K
    nnz = int(nl.indices.shape[0])
    gen = torch.Generator(device=dev).manual_seed(Fc + nnz)
    x = torch.randn((N, Fc, K), device=dev, generator=gen).requires_grad_()
    m = torch.randn((Fc, nnz), device=dev, generator=gen).requires_grad_()
    gm, gy = torch.randn((Fc, nnz), device=dev, generator=gen), torch.randn((N, Fc, K), device=dev, generator=gen)
    rows = nl.rows.long()
    src = torch.div(rows, K, rounding_mode="floor") * K + nl.indices.long()      # the flat (frame, node) of every entry's neighbour
    rows_f, src_f = rows.expand(Fc, nnz), src.expand(Fc, nnz)

    def flat(t):
        return t.detach().transpose(0, 1).reshape(Fc, R).contiguous()      # [F, N K]: the rows over (frame, node) innermost

    xf, gyf = flat(x).requires_grad_(), flat(gy)
    ours = {"gather, source": (lambda t: entry_gather(t, nl, "source"), x, gm),
            "gather, target": (lambda t: entry_gather(t, nl, "target"), x, gm),
            "reduce sum": (lambda t: entry_reduce(t, nl, "sum"), m, gy),
            "reduce mean": (lambda t: entry_reduce(t, nl, "mean"), m, gy),
            "reduce max": (lambda t: entry_reduce(t, nl, "max"), m, gy),
            "reduce sum, to source": (lambda t: entry_reduce(t, nl, "sum", "source"), m, gy),
            "reduce max, to source": (lambda t: entry_reduce(t, nl, "max", "source"), m, gy)}
    theirs = {"gather, source": (lambda t: t.index_select(1, src), xf, gm),
              "gather, target": (lambda t: t.index_select(1, rows), xf, gm),
              "reduce sum": (lambda t: torch.zeros((Fc, R), device=dev).index_add_(1, rows, t), m, gyf),
              "reduce max": (lambda t: torch.full((Fc, R), -float("inf"), device=dev).scatter_reduce(1, rows_f, t, "amax"), m, gyf),
              "reduce sum, to source": (lambda t: torch.zeros((Fc, R), device=dev).index_add_(1, src, t), m, gyf),
              "reduce max, to source": (lambda t: torch.full((Fc, R), -float("inf"), device=dev).scatter_reduce(1, src_f, t, "amax"), m, gyf)}

    def both(f):
        def run():
            f[1].grad = None
            f[0](f[1]).backward(f[2])
        return run

    with torch.no_grad():
        for end in ("source", "target"):
            assert torch.equal(ours["gather, " + end][0](x), theirs["gather, " + end][0](xf))
        for to in ("", ", to source"):
            has = (theirs["reduce max" + to][0](m) > -float("inf"))       # (a node without an entry is +0.0 here and -inf there)
            assert torch.equal(flat(ours["reduce max" + to][0](m))[has], theirs["reduce max" + to][0](m)[has])
            diff = float((flat(ours["reduce sum" + to][0](m)) - theirs["reduce sum" + to][0](m)).abs().max())
            assert diff < 1e-4, diff
    bytes_ = algorithmic_bytes(Fc, nnz)
    res = dict(lists=name, N=N, K=K, F=Fc, nnz=nnz, max_degree=int(nl.degree().max()), bytes=bytes_,
               peak_bytes={"%s%s" % (who, n): peak_bytes(both(fs[n])) for who, fs in (("", ours), ("torch ", theirs)) for n in fs})
    print("%s, F = %d: nnz = %d, largest degree %d, bytes %s" % (name, Fc, nnz, res["max_degree"], bytes_), flush=True)
    copy_src, copy_dst = m.detach(), torch.empty_like(m)
    ts = {}
    for n in ours:
        with torch.no_grad():
            fwd = {"%s, forward" % n: lambda f=ours[n]: f[0](f[1])}
            if n in theirs:
                fwd["torch %s, forward" % n] = lambda f=theirs[n]: f[0](f[1])
            if n == "gather, source":
                fwd["streaming copy of a [F, nnz] tensor"] = lambda: copy_dst.copy_(copy_src)
            ts.update(windows(fwd, REPS))
        fb = {"%s, forward + backward" % n: both(ours[n])}
        if n in theirs:
            fb["torch %s, forward + backward" % n] = both(theirs[n])
        ts.update(windows(fb, REPS))
    med = {n: t[len(t) // 2] for n, t in ts.items()}
    rate = 2 * bytes_["a [F, nnz] tensor"] / med["streaming copy of a [F, nnz] tensor"] * 1e-6      # TB/s: bytes / us * 1e-6
    res["copy_rate_TB_per_s"] = round(rate, 3)
    res["fraction_of_copy_rate"] = {}
    for n, t in ts.items():
        print("  %-50s median %9.1f us (%.1f .. %.1f)   peak %s" % (n, med[n], t[0], t[-1], res["peak_bytes"].get(n.replace(", forward + backward", ""), "")), flush=True)
    for n in ours:
        b = bytes_["gather" if n.startswith("gather") else "reduce to source" if n.endswith("to source") else "reduce"]
        res["fraction_of_copy_rate"][n] = round(b / med["%s, forward" % n] * 1e-6 / rate, 3)
    print("  copy rate %.2f TB/s; forward launches at this fraction of it: %s" % (rate, res["fraction_of_copy_rate"]), flush=True)
    res["microseconds"] = {n: [round(v, 1) for v in t] for n, t in ts.items()}
    return res


def main():
    import torch
    from fast_slic_amd.knn import knn_graph
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    graph = graph_of(N, K)
    gen = torch.Generator(device=graph.indices.device).manual_seed(1)
    knn, _ = knn_graph(torch.rand((N, 5, K), device=graph.indices.device, generator=gen), KNN)
    knn.transposed()
    results = [one_case(name, nl, Fc) for name, nl in (("region adjacency graph", graph), ("knn_graph, k = %d" % KNN, knn)) for Fc in FEATURES]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
