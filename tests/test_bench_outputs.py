"""bench.py --dump-outputs: what the last timed step computed, written as float .npy files so that two builds can be compared
output for output.  CPU: the files, their dtypes and shapes, the fixed sample of label maps too large to write whole, the size
budget of every workload.  GPU: a plain run times exactly --steps steps and the dumped step is the oracle's result."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from fast_slic_amd import CLUSTER_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Workload(object):
    """The part of bench.Workload that dump_outputs() reads: one buffer set of n label maps and n Cluster blocks."""

    def __init__(self, H, W, K, n, seed=0):
        import torch
        rng = np.random.default_rng(seed)
        self.H, self.W = H, W
        d_lab = [torch.from_numpy(rng.integers(0, K, (H, W)).astype(np.int16)) for _ in range(n)]
        cls = np.zeros((n, K), CLUSTER_DTYPE)
        for f in CLUSTER_DTYPE.names:
            cls[f] = rng.integers(0, 200, (n, K)).astype(CLUSTER_DTYPE[f])
        cls["y"] += 0.25
        self.sets = [None, (d_lab, cls, None, None)]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f), allow_pickle=False) for f in sorted(os.listdir(d))}


def test_dump_writes_label_maps_and_every_cluster_field_exactly(tmp_path):
    wl = _Workload(36, 52, 40, 3)
    bench.dump_outputs(wl, 1, str(tmp_path))
    got = _load(str(tmp_path))
    assert sorted(got) == sorted(["labels"] + ["cluster_" + f for f in CLUSTER_DTYPE.names])
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    d_lab, cls, _, _ = wl.sets[1]
    assert got["labels"].shape == (3, 36, 52)
    assert np.array_equal(got["labels"], np.stack([t.numpy() for t in d_lab]).astype(np.float32))
    for f in CLUSTER_DTYPE.names:
        assert got["cluster_" + f].shape == (3, 40)
        assert np.array_equal(got["cluster_" + f], cls[f]), f


def test_large_label_maps_are_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LABEL_BYTES", (4 * 2 + 8) * 500)
    wl = _Workload(40, 60, 30, 2)
    for d in ("a", "b"):
        bench.dump_outputs(wl, 1, str(tmp_path / d))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert a["labels"].shape == (2, 500) and a["labels_index"].shape == (500,)
    assert a["labels"].dtype == np.float32 and a["labels_index"].dtype == np.float64
    assert np.array_equal(a["labels_index"], b["labels_index"]) and np.array_equal(a["labels"], b["labels"])
    idx = a["labels_index"].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 40 * 60
    full = np.stack([t.numpy() for t in wl.sets[1][0]]).reshape(2, -1)
    assert np.array_equal(a["labels"], full[:, idx].astype(np.float32))


@pytest.mark.parametrize("workload", sorted(bench.WORKLOADS))
def test_dump_of_every_workload_stays_under_64_mb(workload):
    cfg = bench.WORKLOADS[workload]
    n, hw = cfg["fpg"], cfg["H"] * cfg["W"]
    m = hw if 4 * n * hw <= bench.DUMP_LABEL_BYTES else bench.DUMP_LABEL_BYTES // (4 * n + 8)
    label_bytes, index_bytes = 4 * n * m, (8 * m if m < hw else 0)
    cluster_bytes = sum(np.dtype(t).itemsize for t in bench.CLUSTER_DUMP_TYPES.values()) * n * cfg["K"]
    assert label_bytes + index_bytes + cluster_bytes <= 64 << 20
    assert sorted(bench.CLUSTER_DUMP_TYPES) == sorted(CLUSTER_DTYPE.names)


@pytest.mark.gpu
def test_plain_run_times_the_steps_it_is_given_and_dumps_the_oracles_result(tmp_path):
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert "parity" not in line and "cpu_baseline" not in line          # the legs of --full
    from fast_slic_amd.synth import variant
    from oracle import oracle as orc
    got = _load(out)
    assert got["labels"].shape == (8, 720, 1280)
    img = variant("A", 720, 1280, seed=0)                              # frame 0 of every step: seed 0 (batch.weak_shard)
    labels, cl = orc.slic_iterate(img, orc.initialize_clusters(img, 1600))
    assert np.array_equal(got["labels"][0], orc.to_int16(labels).astype(np.float32))
    for f in CLUSTER_DTYPE.names:
        assert np.array_equal(got["cluster_" + f][0], cl[f]), f
