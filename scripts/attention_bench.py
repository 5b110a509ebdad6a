"""Device time of neighbour_dot, neighbour_softmax, head_aggregate and graph_attention (fast_slic_amd/attention.py), forward and forward +
backward, beside the torch composition they replace, by HIP events over warmed repetitions.

    python scripts/attention_bench.py [--json OUT.json] [--variant fast_slic_amd/libfslic_hip_var_NAME.so]

The graphs are those of slic_tensor maps of 1280 x 720 frames, at two sizes: N = 8, C = 64, K = 1600 with 4 and 8 heads, and N = 16,
C = 256, K = 6000 with 8 heads.  The baseline on the same tensors, laid out [C, N K] so that one flat index serves every frame:
index_select of both ends and a sum over the head's channels for the scores, scatter_reduce("amax") and index_add_ for the softmax,
index_add_ of the weighted gather for the sum (float atomics and [C, nnz] intermediates); its backward is autograd's.  The two forms
alternate window by window.  The results are compared first (the composition adds in another order and uses torch's exp: a tolerance,
not bits).  Beside the times the script prints the algorithmic bytes of each launch and the time of a streaming copy of the values.

--variant: a second build of the library (make VAR=item DEFS=-DFSLIC_ATTEND_PACK=0: an item of the neighbour sum is 32 channels of ONE
head) whose fslic_hip_attend_apply is timed against the loaded library's on both graphs at D = 8 and D = 32, forward and transposed,
the two alternating window by window.  DESIGN.md holds the figures."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from aggregate_bench import H, W, windows      # noqa: E402

SIZES = [(8, 64, 1600, (4, 8), 50), (16, 256, 6000, (8,), 10)]


def algorithmic_bytes(N, C, K, nnz, Hd):
    """What each launch has to move at least: every value, gradient and result once; the lists once per (head, entry) for the dot, once
    per four heads for the softmax, once per four eight-channel chunks for the sum (with its weight window per chunk)."""
    cells, R, groups = 4 * N * C * K, N * K, (Hd * ((C // Hd + 7) // 8) + 3) // 4
    return {"dot": 2 * cells + Hd * 12 * nnz, "softmax": (Hd + 3) // 4 * (4 * nnz + 8 * R) + 8 * Hd * nnz,
            "softmax backward": (Hd + 3) // 4 * (4 * nnz + 8 * R) + 12 * Hd * nnz, "sum": 2 * cells + groups * (4 * nnz + 8 * R + 16 * nnz),
            "sum transposed": 2 * cells + groups * (8 * nnz + 8 * R + 16 * nnz), "torch intermediates [C, nnz]": 4 * C * nnz}


def graph_of(N, K):
    import torch
    from fast_slic_amd import Slic
    from fast_slic_amd.frames import slic_tensor
    from fast_slic_amd.propagate import neighbour_lists
    from fast_slic_amd.rag import superpixel_graph
    from fast_slic_amd.synth import variant
    images = torch.from_numpy(np.stack([variant("A", H, W, seed=s) for s in range(N)])).to(torch.device("cuda", 0))
    nl = neighbour_lists(superpixel_graph(slic_tensor(images, Slic(num_components=K)).labels, K))
    nl.transposed()
    return nl


def show(ts):
    for name, t in ts.items():
        print("  %-46s median %9.1f us (%.1f .. %.1f)" % (name, t[len(t) // 2], t[0], t[-1]), flush=True)
    return {name: [round(v, 1) for v in t] for name, t in ts.items()}


def one_size(nl, N, C, K, Hd, reps):
    import torch
    from fast_slic_amd.attention import graph_attention, head_aggregate, neighbour_dot, neighbour_softmax
    dev, D, R = torch.device("cuda", 0), C // Hd, N * K
    nnz = int(nl.indices.shape[0])
    gen = torch.Generator(device=dev).manual_seed(K + Hd)
    q, k, v = (torch.randn((N, C, K), device=dev, generator=gen).requires_grad_() for _ in range(3))
    g = torch.randn((N, C, K), device=dev, generator=gen)
    s0 = torch.randn((Hd, nnz), device=dev, generator=gen).requires_grad_()
    w0 = torch.rand((Hd, nnz), device=dev, generator=gen).requires_grad_()
    gs = torch.randn((Hd, nnz), device=dev, generator=gen)
    rows = nl.rows.long()
    src = torch.div(rows, K, rounding_mode="floor") * K + nl.indices.long()      # the flat (frame, node) of every entry's neighbour
    rows_h = rows.expand(Hd, nnz)

    def flat(t):
        return t.detach().transpose(0, 1).reshape(C, R).contiguous()      # [C, N K]: the rows over (frame, node) innermost

    qf, kf, vf, gf = flat(q).requires_grad_(), flat(k).requires_grad_(), flat(v).requires_grad_(), flat(g)

    def t_dot(qf, kf):
        return (qf.index_select(1, rows) * kf.index_select(1, src)).view(Hd, D, nnz).sum(1)

    def t_softmax(s):
        m = torch.full((Hd, R), -float("inf"), device=dev).scatter_reduce(1, rows_h, s.detach(), "amax")
        e = torch.exp(s - m[:, rows])
        return e / torch.zeros((Hd, R), device=dev).index_add_(1, rows, e)[:, rows]

    def t_sum(vf, w):
        return torch.zeros_like(vf).index_add_(1, rows, vf.index_select(1, src) * w.repeat_interleave(D, 0))

    def t_attention(qf, kf, vf):
        return t_sum(vf, t_softmax(t_dot(qf * D ** -0.5, kf)))

    def both(fn, inputs, grad):
        def run():
            for t in inputs:
                t.grad = None
            fn(*inputs).backward(grad)
        return run

    ours = {"dot": (lambda a, b: neighbour_dot(a, b, nl, Hd), [q, k], gs), "softmax": (lambda s: neighbour_softmax(s, nl), [s0], gs),
            "sum": (lambda x, w: head_aggregate(x, nl, w), [v, w0], g), "graph_attention": (lambda a, b, c: graph_attention(a, b, c, nl, Hd), [q, k, v], g)}
    theirs = {"dot": (t_dot, [qf, kf], gs), "softmax": (t_softmax, [s0], gs), "sum": (t_sum, [vf, w0], gf), "graph_attention": (t_attention, [qf, kf, vf], gf)}
    y, yt = graph_attention(q, k, v, nl, Hd), t_attention(qf, kf, vf)
    both(*ours["graph_attention"])()
    gq = q.grad.clone()
    both(*theirs["graph_attention"])()
    diff = dict(y=float((flat(y) - yt.detach()).abs().max()), grad_query=float((flat(gq) - qf.grad).abs().max()),
                scores=float((neighbour_dot(q, k, nl, Hd) - t_dot(qf, kf)).detach().abs().max()),
                alpha=float((neighbour_softmax(s0, nl) - t_softmax(s0)).detach().abs().max()))
    assert diff["y"] < 1e-4 and diff["grad_query"] < 1e-4 and diff["scores"] < 1e-4 * D ** 0.5 and diff["alpha"] < 1e-6
    res = dict(N=N, C=C, K=K, heads=Hd, nnz=nnz, max_degree=int(nl.degree().max()), bytes=algorithmic_bytes(N, C, K, nnz, Hd), max_abs_diff=diff)
    print("N = %d, C = %d, K = %d, heads = %d: nnz = %d, largest degree %d, bytes %s, differences %s" % (N, C, K, Hd, nnz, res["max_degree"], res["bytes"], diff), flush=True)
    copy_src, copy_dst = v.detach(), torch.empty_like(v)
    ts = {}
    for name in ours:
        with torch.no_grad():
            fwd = {"%s, forward" % name: lambda f=ours[name]: f[0](*f[1]), "torch %s, forward" % name: lambda f=theirs[name]: f[0](*f[1])}
            if name == "sum":
                fwd["streaming copy of the values"] = lambda: copy_dst.copy_(copy_src)
            ts.update(windows(fwd, reps))
        ts.update(windows({"%s, forward + backward" % name: both(*ours[name]), "torch %s, forward + backward" % name: both(*theirs[name])}, reps))
    res["microseconds"] = show(ts)
    return res


def item_shapes(nl, N, C, K, path, reps):
    """fslic_hip_attend_apply of the loaded library against the variant's, at D = 8 and D = 32."""
    import torch
    from fast_slic_amd import _binding as B, _tensors as T
    dev = torch.device("cuda", 0)
    libs = {"packed (four chunks of any head)": B.load_library(), "one head an item": ctypes.CDLL(path)}
    for lib in libs.values():
        lib.fslic_hip_attend_apply.restype, lib.fslic_hip_attend_apply.argtypes = dict((n, (r, a)) for n, r, a in B.SIGNATURES)["fslic_hip_attend_apply"]
    nnz = int(nl.indices.shape[0])
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((N, C, K), device=dev, generator=gen)
    out = {name: torch.empty_like(x) for name in libs}
    res = {}
    for D in (8, 32):
        Hd = C // D
        w = torch.rand((Hd, nnz), device=dev, generator=gen)
        for transposed in (0, 1):
            offsets, ia, ib = nl.transposed() if transposed else (nl.offsets, nl.indices, None)

            def call(name):
                B._check(libs[name].fslic_hip_attend_apply(0, T.stream(dev), N, C, K, nnz, Hd, transposed, offsets.data_ptr(), ia.data_ptr(), T.ptr(ib),
                                                           w.data_ptr(), x.data_ptr(), out[name].data_ptr()))
            ts = windows({"D = %d, %s, %s" % (D, "transposed" if transposed else "forward", name): (lambda name=name: call(name)) for name in libs}, reps)
            a, b = out.values()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))      # the same bits from both item shapes
            res.update(show(ts))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--variant", default=None)
    args = ap.parse_args()
    results = []
    for N, C, K, heads, reps in SIZES:
        nl = graph_of(N, K)
        if args.variant:
            print("item shapes of the neighbour sum, N = %d, C = %d, K = %d:" % (N, C, K), flush=True)
            results.append(dict(N=N, C=C, K=K, item_shapes=item_shapes(nl, N, C, K, args.variant, reps)))
        results += [one_size(nl, N, C, K, Hd, reps) for Hd in heads]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
