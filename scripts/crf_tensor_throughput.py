"""superpixel_crf(..., max_iter=10) on the GPU at the shapes of DESIGN.md's SimpleCRF table (K, classes, frames, temporal=True) and on
8 independent 1280x720 frames at K = 1600, C = 21: device time between two events around one call (1 start + 1 edge launch + 10
sweeps, the Python side included as far as it delays the stream), median of `--reps` calls after a warm-up, next to the host wall time
of SimpleCRF.inference(10) on the same clusters, neighbour lists and unaries.  Neighbour lists are real: get_connectivity on
1280x720 synthetic frames per K.  Beside the forward: the same call with the unaries and a compat tensor requiring a gradient (the
saved-iterates forward) and the backward of q.sum() through it (the transposition of the lists, the edge pass again, 10 adjoint
sweeps, the closing gather and the compat sum), each between two events.
    python scripts/crf_tensor_throughput.py [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fast_slic_amd import Slic                          # noqa: E402
from fast_slic_amd.crf import SimpleCRF                 # noqa: E402
from fast_slic_amd.crf_torch import superpixel_crf      # noqa: E402
from fast_slic_amd.synth import variant                 # noqa: E402

SHAPES = [(1600, 2, 1, True), (1600, 21, 4, True), (6000, 21, 4, True), (1600, 21, 8, False)]      # K, C, frames, temporal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    slics = {}
    for K in sorted({s[0] for s in SHAPES}):
        frames = []
        for v in "ABCD":
            s = Slic(num_components=K)
            s.iterate(variant(v, 720, 1280, seed=1))
            frames.append(s)
        slics[K] = frames
    for K, Cn, N, temporal in SHAPES:
        models = [slics[K][n % 4].slic_model for n in range(N)]
        lists = [m.get_connectivity(slics[K][n % 4].last_assignment).tolist() for n, m in enumerate(models)]
        proba = [rng.dirichlet(np.ones(Cn), K).T.astype(np.float32).copy() for _ in range(N)]
        # SimpleCRF: one window with temporal links, or one CRF per independent frame (timed together)
        crfs = []
        for group in ([list(range(N))] if temporal else [[n] for n in range(N)]):
            crf = SimpleCRF(Cn, K)
            for n in group:
                f = crf.push_frame()
                f.set_clusters(models[n].cluster_array)
                f.set_connectivity(lists[n])
                f.set_proba(proba[n])
            crf.initialize()
            crf.inference(10)                               # warm-up: allocation and first upload
            crfs.append(crf)
        unaries = np.stack([crf.get_frame(t).unaries for crf in crfs for t in range(crf.first_time, crf.last_time + 1)])
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for crf in crfs:
                crf.inference(10)
            ts.append((time.perf_counter() - t0) * 1e3)
        simple_ms = float(np.median(ts))
        # the tensors
        cl = [m.cluster_array for m in models]
        yxrgb = torch.from_numpy(np.stack([np.stack([c[n] for n in ("y", "x", "r", "g", "b")]) for c in cl]).astype(np.float32)).to(dev)
        members = torch.from_numpy(np.stack([c["num_members"].view(np.int32) for c in cl])).to(dev)
        rows = [r for frame in lists for r in frame]
        off = np.zeros(len(rows) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in rows])
        graph = (torch.from_numpy(off).to(dev), torch.tensor([v for r in rows for v in r], dtype=torch.int32, device=dev))
        un = torch.from_numpy(unaries).to(dev)
        for _ in range(3):
            q = superpixel_crf(un, graph, yxrgb, members, max_iter=10, temporal=temporal)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            q = superpixel_crf(un, graph, yxrgb, members, max_iter=10, temporal=temporal)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms = float(np.median(ts))
        # ten further sweeps alone: (20 sweeps - 10 sweeps) / 10 is one sweep without the start, the edge pass and the Python side
        ts20 = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            superpixel_crf(un, graph, yxrgb, members, max_iter=20, temporal=temporal)
            e1.record()
            e1.synchronize()
            ts20.append(e0.elapsed_time(e1))
        sweep_us = (float(np.median(ts20)) - ms) * 100
        # the differentiable call: the forward that keeps its iterates, and the backward
        un_g, comp_g = un.clone().requires_grad_(True), torch.ones(Cn, device=dev).requires_grad_(True)
        g_out = torch.ones_like(un)
        fwd, bwd = [], []
        for rep in range(3 + a.reps):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            un_g.grad = comp_g.grad = None
            e0.record()
            qg = superpixel_crf(un_g, graph, yxrgb, members, max_iter=10, compat=comp_g, temporal=temporal)
            e1.record()
            qg.backward(g_out)
            e2.record()
            e2.synchronize()
            if rep >= 3:
                fwd.append(e0.elapsed_time(e1))
                bwd.append(e1.elapsed_time(e2))
        print(json.dumps(dict(K=K, classes=Cn, frames=N, temporal=temporal, entries=int(off[-1]), tensor_ms_per_call10=round(ms, 4),
                              tensor_us_per_sweep=round(sweep_us, 2),
                              grad_forward_ms_per_call10=round(float(np.median(fwd)), 4),
                              backward_ms_per_call10=round(float(np.median(bwd)), 4), simple_crf_ms_per_inference10=round(simple_ms, 4),
                              ratio=round(simple_ms / ms, 2))))


if __name__ == "__main__":
    main()
