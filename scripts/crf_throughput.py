"""SimpleCRF inference(10) on the GPU at the shapes of the issue's CPU table (K, classes, frames): host wall time per call (upload of
nothing new + 1 edge launch + 10 sweeps + one synchronisation), median of `--reps` calls after a warm-up, next to the reference's
single-threaded CPU figure.  Neighbour lists are real: fast_slic get_connectivity on a 1280x720 synthetic frame per K.
upload_ms_per_inference1 is the upload path: the wall time of inference(1) right after set_clusters was called again on every
frame, which makes every graph dirty (the CSR rebuild, the staging of the clusters and the upload of the window); median of `--reps`.
    python scripts/crf_throughput.py [--reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fast_slic_amd import Slic                      # noqa: E402
from fast_slic_amd.crf import SimpleCRF             # noqa: E402
from fast_slic_amd.synth import variant             # noqa: E402

SHAPES = [(1600, 2, 1, 8.3), (1600, 21, 4, 502.0), (6000, 21, 4, 1954.0)]      # K, C, T, reference CPU ms (issue table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    slics = {}
    for K in sorted({s[0] for s in SHAPES}):
        frames = []
        for v in "ABCD":
            s = Slic(num_components=K)
            s.iterate(variant(v, 720, 1280, seed=1))
            frames.append(s)
        slics[K] = frames
    rows = []
    for K, Cn, T, ref_ms in SHAPES:
        crf = SimpleCRF(Cn, K)
        for t in range(T):
            f = crf.push_slic_frame(slics[K][t])
            f.set_proba(rng.dirichlet(np.ones(Cn), K).T.astype(np.float32).copy())
        crf.initialize()
        crf.inference(10)                                   # warm-up: allocation and first upload
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            crf.inference(10)
            ts.append((time.perf_counter() - t0) * 1e3)
        ms = float(np.median(ts))
        live = [crf.get_frame(crf.first_time + t) for t in range(T)]
        clusters = [f.get_clusters() for f in live]
        ups = []
        for _ in range(a.reps):
            for f, cl in zip(live, clusters):
                f.set_clusters(cl)
            t0 = time.perf_counter()
            crf.inference(1)
            ups.append((time.perf_counter() - t0) * 1e3)
        edges = sum(len(l) for l in crf.get_frame(crf.first_time).get_connectivity())
        rows.append(dict(K=K, classes=Cn, frames=T, edges_per_frame=edges, gpu_ms_per_inference10=round(ms, 4),
                         gpu_us_per_iteration=round(ms * 100, 2), ref_cpu_ms=ref_ms, speedup=round(ref_ms / ms, 1),
                         upload_ms_per_inference1=round(float(np.median(ups)), 4)))
        print(json.dumps(rows[-1]))


if __name__ == "__main__":
    main()
