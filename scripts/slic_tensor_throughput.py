"""Slic on torch tensors (fast_slic_amd/frames.py) at 1280 x 720, K = 1600, on 8 - 64 frames that are resident in HBM:

  (a) slic_tensor on a contiguous uint8 [N, H, W, 3] batch (used in place)
  (b) slic_tensor on a float32 [N, 3, H, W] batch (one k_pack_rgb launch first)
  (c) the per-frame loop Slic.iterate(numpy) on the same frames (each copied up, its int16 map copied down)
  (d) k_pack_rgb alone on the float32 batch against the torch composition
      (x * s).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    python scripts/slic_tensor_throughput.py [--json OUT.json] [--frames 8 16 32 64]

(a) - (c) are host-clock times around the call, which synchronises itself; (d) is HIP events around one launch or composition.  Every
shape is warmed up first; the figure is the median of 20.  The script first checks (a) and (b) against (c) on the first frames, by ==.
The two ratios DESIGN.md records: (c) / (a) per frame, and composition / k_pack_rgb."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, K, REPS = 720, 1280, 1600, 20


def median_host_ms(fn):
    import torch
    for _ in range(3):
        fn()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[REPS // 2]


def median_event_ms(fn):
    import torch
    for _ in range(3):
        fn()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[REPS // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 16, 32, 64])
    args = ap.parse_args()
    import torch
    from fast_slic_amd import Slic
    from fast_slic_amd.frames import pack_rgb, slic_tensor
    from fast_slic_amd.synth import variant
    dev = torch.device("cuda", 0)
    nmax = max(args.frames)
    host = np.stack([variant("A", H, W, seed=i % 8) for i in range(nmax)])
    u8 = torch.from_numpy(host).to(dev)
    f32 = torch.from_numpy(host.astype(np.float32) / np.float32(255)).to(dev).permute(0, 3, 1, 2).contiguous()
    slic = Slic(num_components=K)

    ra, rb = slic_tensor(u8[:2], slic), slic_tensor(f32[:2], slic)
    for n in range(2):
        s = Slic(num_components=K)
        lab = s.iterate(host[n])
        for r in (ra, rb):
            assert np.array_equal(r.labels[n].cpu().numpy(), lab) and r.clusters[n].tobytes() == s.slic_model.cluster_array.tobytes()
    print("slic_tensor (uint8 NHWC, float32 NCHW) equals Slic.iterate(numpy) on 2 frames", flush=True)

    models = [Slic(num_components=K) for _ in range(nmax)]      # one per frame, as a video pipeline keeps them

    def loop(n):
        for i in range(n):
            models[i].iterate(host[i])

    res = dict(shape=[H, W], K=K, reps=REPS, rows=[])
    mp = H * W / 1e6
    for n in args.frames:
        a = median_host_ms(lambda: slic_tensor(u8[:n], slic))
        b = median_host_ms(lambda: slic_tensor(f32[:n], slic))
        c = median_host_ms(lambda: loop(n))
        out = torch.empty((n, (3 * H * W + 15) & ~15), dtype=torch.uint8, device=dev)
        x = f32[:n]
        d_pack = median_event_ms(lambda: pack_rgb(x, out=out))
        d_torch = median_event_ms(lambda: (x * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous())
        row = dict(frames=n, a_ms=a, b_ms=b, c_ms=c, pack_ms=d_pack, torch_ms=d_torch, c_over_a=c / a, torch_over_pack=d_torch / d_pack)
        res["rows"].append(row)
        print("N %2d  (a) uint8 in place %7.3f ms = %6.3f ms/frame %5.1f GP/s   (b) float32 %7.3f ms = %6.3f ms/frame %5.1f GP/s   "
              "(c) numpy loop %7.3f ms = %6.3f ms/frame %5.1f GP/s   (c)/(a) %.2f" % (n, a, a / n, n * mp / a, b, b / n, n * mp / b, c, c / n, n * mp / c, c / a),
              flush=True)
        print("      (d) k_pack_rgb %7.3f ms (%5.0f GB/s of 15 B/px)   torch composition %7.3f ms   ratio %.2f"
              % (d_pack, n * H * W * 15 / d_pack / 1e6, d_torch, d_torch / d_pack), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
