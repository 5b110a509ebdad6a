"""The host transposition of a SimpleCRF window's clusters (crf_stage_clusters, csrc/crf.h) under the host sanitizers: a stand-alone
program (tests/native/crf_stage_check.cpp) stages windows of K = 1, 63, 65 clusters and T = 1, 3 frames into buffers of exactly the
promised size and compares every word.  No GPU and no Python extension is involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_staging_under_address_and_undefined_sanitizers(tmp_path):
    exe = str(tmp_path / "crf_stage_check")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "fast_slic_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "crf_stage_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count(": 0 of ") == 6, r.stdout
