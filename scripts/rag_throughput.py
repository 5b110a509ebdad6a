"""Region adjacency graph throughput (fast_slic_amd/rag.py): per configuration the device-event time of accumulate + compact alone (the
two library entries on preallocated buffers), the whole superpixel_graph call with its host synchronisation, sort and gathers (wall
clock), the algorithmic bytes read (labels 2 B/px, image C B/px) against the 8 TB/s of the MI355X, and next to them the existing
Engine.get_connectivity on the same maps with the labels left in HBM (wall clock per batch, frame after frame: it returns host arrays).

    python scripts/rag_throughput.py [--reps 20] [--json out.json]

Label maps are Slic's on synthetic frames (one per frame of the batch).  Kernel names for a separate
`rocprofv3 --kernel-trace --stats` run: k_rag_tiles, k_pair_compact<true>, k_adjacent_pairs."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fast_slic_amd import Slic, _binding as B                     # noqa: E402
from fast_slic_amd.rag import first_capacity, superpixel_graph    # noqa: E402
from fast_slic_amd.synth import variant                           # noqa: E402

HBM = 8.0e12
CONFIGS = [(8, 720, 1280, 1600), (8, 2160, 3840, 6000)]


def device_time(fn, reps, warmup=3):
    """Median device time (us) of fn() on the current stream, events around each call."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def wall_time(fn, reps, warmup=2):
    """Median wall-clock time (us) of fn() followed by a device synchronisation."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts))


def kernels_only(lab, img, K, connectivity):
    """A closure that enqueues accumulate + compact on buffers sized for the first table (Slic maps fit it)."""
    lib = B.load_library()
    N, H, W = lab.shape
    Cc = img.shape[-1] if img is not None else 0
    cap = first_capacity(K)
    nbytes = C.c_size_t()
    B._check(lib.fslic_hip_rag_workspace_size(N, K, Cc, cap, C.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=lab.device)
    E = N * cap // 2
    keys = torch.empty(E, dtype=torch.int64, device=lab.device)
    boundary = torch.empty(E, dtype=torch.int32, device=lab.device)
    contrast = torch.empty((E, max(Cc, 1)), dtype=torch.int64, device=lab.device) if img is not None else None
    st = C.c_void_p(torch.cuda.current_stream(lab.device).cuda_stream)

    def run():
        B._check(lib.fslic_hip_rag_accumulate(lab.device.index, st, N, H, W, K, connectivity, lab.data_ptr(), 0,
                                              img.data_ptr() if img is not None else None, Cc, cap, ws.data_ptr(), nbytes.value))
        B._check(lib.fslic_hip_rag_compact(lab.device.index, st, N, Cc, cap, ws.data_ptr(), nbytes.value, keys.data_ptr(),
                                           boundary.data_ptr(), contrast.data_ptr() if contrast is not None else None, E))
    run()
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0, "the first table overflowed"
    return run, (ws, keys, boundary, contrast)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--configs", default=None, help="indices into the config list, comma-separated")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    cfgs = CONFIGS if not args.configs else [CONFIGS[int(i)] for i in args.configs.split(",")]
    for N, H, W, K in cfgs:
        frames = [variant("A", H, W, seed=s) for s in range(N)]
        slic = Slic(num_components=K)
        labs = np.stack([slic.iterate(f) for f in frames])
        lab = torch.from_numpy(labs).to(dev)
        image = torch.from_numpy(np.stack(frames)).to(dev)
        px = N * H * W
        print("N=%d %dx%d K=%d" % (N, W, H, K))
        engine = slic.slic_model._engine
        HWb = H * W * 2

        def existing():
            for n in range(N):
                engine.get_connectivity(lab.data_ptr() + n * HWb, H, W, K)
        us = wall_time(existing, max(3, args.reps // 4))
        print("   %-44s %10.1f us wall  (%.1f us a frame)" % ("Engine.get_connectivity, labels in HBM", us, us / N))
        rows.append(dict(N=N, H=H, W=W, K=K, op="get_connectivity", wall_us=us))
        for connectivity in (4, 8):
            for img in (None, image):
                b = px * 2 + (px * img.shape[-1] if img is not None else 0)
                run, keep = kernels_only(lab, img, K, connectivity)
                dus = device_time(run, args.reps)
                wus = wall_time(lambda: superpixel_graph(lab, K, connectivity=connectivity, image=img), args.reps)
                g = superpixel_graph(lab, K, connectivity=connectivity, image=img)
                name = "connectivity %d%s" % (connectivity, ", image" if img is not None else "")
                print("   %-20s E=%7d  accumulate + compact %8.1f us  %7.1f MB  %5.2f TB/s  %5.3f of 8 TB/s   whole call %9.1f us wall"
                      % (name, g.edge_index.shape[1], dus, b / 1e6, b / dus / 1e6, b / dus / 1e6 / (HBM / 1e12), wus))
                rows.append(dict(N=N, H=H, W=W, K=K, op=name, edges=int(g.edge_index.shape[1]), device_us=dus, bytes=b,
                                 frac_8tbs=b / dus / 1e6 / (HBM / 1e12), wall_us=wus))
                del keep
        sys.stdout.flush()
        del lab, image
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
