"""Golden fixtures of debug_mode (tests/golden/recorder/): the recorder reports of the REFERENCE's own Cython binding
(oracle/_ref/integration's cfast_slic, built by __graft_entry__.build() where the reference is present), arch "standard", one
thread, debug_mode on, plus the inputs that produced them.

    python scripts/make_recorder_golden.py

Writes tests/golden/recorder/cases.json (the parameters of every case), inputs.npz (the frames) and <case>.json.gz (the report of
the case's last iterate() call, exactly as SlicModel.last_recorder_report holds it).  tests/test_gpu_recorder.py replays every case
on the GPU and compares the bytes."""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref", "integration"))
sys.path.insert(1, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "recorder")

# name, frame kind, H, W, K, max_iter, stride, options of the model (SlicModel attributes), calls (2: a warm second call)
CASES = [
    ("slic_s1", "A", 32, 40, 8, 2, 1, {}, 1),
    ("slic_s3", "A", 48, 64, 12, 3, 3, {}, 1),
    ("slic_s5", "B", 40, 48, 10, 3, 5, {}, 1),
    ("preemptive", "A", 48, 64, 12, 4, 3, {"preemptive": True, "preemptive_thres": 0.3}, 1),
    ("euclidean", "A", 40, 48, 10, 3, 3, {"manhattan_spatial_dist": False}, 1),
    ("no_lab", "A", 40, 48, 10, 3, 2, {"convert_to_lab": False}, 1),
    ("realdist", "A", 40, 48, 10, 3, 3, {"real_dist": True, "real_dist_type": "standard"}, 1),
    ("realdist_l2", "A", 40, 48, 10, 3, 3, {"real_dist": True, "real_dist_type": "l2"}, 1),
    ("realdist_noq", "A", 40, 48, 10, 3, 3, {"real_dist": True, "real_dist_type": "noq"}, 1),
    ("short_frame", "A", 32, 40, 6, 2, 36, {}, 1),
    ("small_s", "B", 32, 40, 40, 3, 3, {}, 1),
    ("warm", "A", 48, 64, 12, 3, 3, {}, 2),
]
COMPACTNESS, MIN_SIZE_FACTOR = 10.0, 0.25


def configure(m, opts):
    """What fast_slic.base_slic.BaseSlic sets on a SlicModel, with debug_mode on."""
    m.real_dist = bool(opts.get("real_dist", False))
    if m.real_dist:
        m.real_dist_type = opts["real_dist_type"]
    m.convert_to_lab = bool(opts.get("convert_to_lab", True))
    m.preemptive = bool(opts.get("preemptive", False))
    m.preemptive_thres = float(opts.get("preemptive_thres", 0.05))
    m.manhattan_spatial_dist = bool(opts.get("manhattan_spatial_dist", True))
    m.num_threads = 1
    m.debug_mode = True


def main():
    import cfast_slic
    from fast_slic_amd.synth import variant
    os.makedirs(OUT, exist_ok=True)
    index, frames = [], {}
    for name, kind, H, W, K, iters, stride, opts, calls in CASES:
        img = variant(kind, H, W, seed=7)
        m = cfast_slic.SlicModel(K, "standard")
        configure(m, opts)
        m.initialize(img)
        for _ in range(calls):
            m.iterate(img, iters, COMPACTNESS, MIN_SIZE_FACTOR, stride)
        report = m.last_recorder_report
        assert isinstance(report, bytes) and len(json.loads(report)["snapshots"]) == iters + 1
        with gzip.GzipFile(os.path.join(OUT, name + ".json.gz"), "wb", mtime=0) as f:
            f.write(report)
        frames[name] = img
        index.append(dict(name=name, H=H, W=W, K=K, max_iter=iters, stride=stride, options=opts, calls=calls,
                          compactness=COMPACTNESS, min_size_factor=MIN_SIZE_FACTOR, report_bytes=len(report)))
        print("%-14s %dx%d K=%d iters=%d stride=%d %s: %d bytes" % (name, H, W, K, iters, stride, opts, len(report)))
    np.savez_compressed(os.path.join(OUT, "inputs.npz"), **frames)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(index, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
