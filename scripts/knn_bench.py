"""Device time and peak memory of knn_graph (fast_slic_amd/knn.py) beside the torch composition it replaces, torch.cdist + topk on the
same tensors in the same process, by HIP events over warmed repetitions.

    python scripts/knn_bench.py [--json OUT.json] [--variant NAME=fast_slic_amd/libfslic_hip_var_NAME.so ...]

The shapes are N = 8, K in {1600, 6000}, D in {5, 64}, k in {8, 16}, and N = 1, K = 1600, D = 5, k = 8, which leaves most of the chip
without a row of its own.  The points are uniform in [0, 1): positions and colours of pooled superpixels have no structure the kernel
could use.  The composition is cdist of the [N, K, D] layout (made outside the timed window), +inf on the diagonal, topk(k,
largest=False): it materialises [N, K, K] distances, computes |a|^2 + |b|^2 - 2 a.b and breaks ties as the sort pleases, so the two
are compared by the share of equal indices and the largest difference of the distances they agree on, not by bits.  The two forms
alternate window by window.  Peak memory is torch's max_memory_allocated over one call, above what was allocated before it.  Beside
the times the script prints the pair-channel rate N K^2 D / t: three float operations each.

--variant: further builds of the library (make VAR=rows16 DEFS=-DFSLIC_KNN_ROWS=16, make VAR=rows64 DEFS=-DFSLIC_KNN_ROWS=64: one
block shape throughout) whose fslic_hip_knn_graph is timed against the loaded library's at every shape, alternating window by window;
all give the same bytes.  DESIGN.md holds the figures."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from aggregate_bench import windows      # noqa: E402

SHAPES = [(8, K, D, k) for K in (1600, 6000) for D in (5, 64) for k in (8, 16)] + [(1, 1600, 5, 8)]


def peak_bytes(fn):
    import torch
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def one_shape(N, K, D, k, variants):
    import torch
    from fast_slic_amd import _binding as B, _tensors as T
    from fast_slic_amd.knn import knn_graph
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(K + D + k)
    x = torch.rand((N, D, K), device=dev, generator=gen)
    xt = x.transpose(1, 2).contiguous()

    def ours():
        return knn_graph(x, k)

    def theirs():
        d = torch.cdist(xt, xt)
        d.diagonal(dim1=1, dim2=2).fill_(float("inf"))
        return d.topk(k, largest=False)

    (nl, dist), (val, idx) = ours(), theirs()
    mine = nl.indices.view(N, K, k).long()
    same = mine == idx
    diff = float(((dist.view(N, K, k).sqrt() - val).abs() * same).max())
    res = dict(N=N, K=K, D=D, k=k, equal_indices=float(same.float().mean()), max_abs_diff_of_equal_entries=diff,
               peak_bytes={"knn_graph": peak_bytes(ours), "cdist + topk": peak_bytes(theirs)}, distance_matrix_bytes=4 * N * K * K)
    assert res["equal_indices"] > 0.5 and diff < 1e-3, res
    reps = 20 if K < 3000 else 5
    fns = {"knn_graph": ours, "cdist + topk": theirs}
    outs = {}
    for name, path in variants:
        lib = ctypes.CDLL(path)
        lib.fslic_hip_knn_graph.restype, lib.fslic_hip_knn_graph.argtypes = dict((n, (r, a)) for n, r, a in B.SIGNATURES)["fslic_hip_knn_graph"]
        outs[name] = (torch.empty_like(nl.indices), torch.empty_like(dist))

        def call(lib=lib, out=outs[name]):
            B._check(lib.fslic_hip_knn_graph(0, T.stream(dev), N, D, K, k, 0, x.data_ptr(), None, None, out[0].data_ptr(), out[1].data_ptr()))
        fns["fslic_hip_knn_graph, %s" % name] = call
    with torch.no_grad():
        ts = windows(fns, reps)
    for name, (i, d) in outs.items():
        assert torch.equal(i, nl.indices) and torch.equal(d.view(torch.int32), dist.view(torch.int32)), name      # the same bytes from every block shape
    print("N = %d, K = %d, D = %d, k = %d: %.1f %% equal indices, peak bytes %s, [N, K, K] is %d bytes" % (
        N, K, D, k, 100 * res["equal_indices"], res["peak_bytes"], res["distance_matrix_bytes"]), flush=True)
    for name, t in ts.items():
        med = t[len(t) // 2]
        print("  %-40s median %9.1f us (%.1f .. %.1f)  %7.1f G pair-channels/s" % (name, med, t[0], t[-1], N * K * K * D / med * 1e-3), flush=True)
    res["microseconds"] = {name: [round(v, 1) for v in t] for name, t in ts.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--variant", action="append", default=[])
    args = ap.parse_args()
    variants = [tuple(v.split("=", 1)) for v in args.variant]
    results = [one_shape(N, K, D, k, variants) for N, K, D, k in SHAPES]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
