"""crf_expf (fast_slic_amd/csrc/crf.h) against the host libm's expf over all 2^32 float bit patterns, on the host (the library's
test-only entry fslic_hip_crf_expf_host, the same function the kernels use).  Prints the number of mismatches and the first few.
    python scripts/crf_expf_sweep.py [--threads 8]"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fast_slic_amd import _binding as B              # noqa: E402

CHUNK = 1 << 24


def chunk(c):
    lib = B.load_library()
    u = (np.arange(CHUNK, dtype=np.uint64) + c * CHUNK).astype(np.uint32)
    x = u.view(np.float32)
    ours, libm = np.empty_like(x), np.empty_like(x)
    lib.fslic_hip_crf_expf_host(x.ctypes.data, ours.ctypes.data, x.size, 0)
    lib.fslic_hip_crf_expf_host(x.ctypes.data, libm.ctypes.data, x.size, 1)
    bad = np.nonzero(ours.view(np.uint32) != libm.view(np.uint32))[0]
    return [(int(u[i]), int(ours.view(np.uint32)[i]), int(libm.view(np.uint32)[i])) for i in bad]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    t0 = time.time()
    with ThreadPoolExecutor(a.threads) as ex:
        bad = [b for r in ex.map(chunk, range((1 << 32) // CHUNK)) for b in r]
    print("crf_expf vs host expf: %d mismatches over 2^32 inputs (%.0f s)" % (len(bad), time.time() - t0))
    for u, o, l in bad[:10]:
        print("  x=0x%08x crf_expf=0x%08x expf=0x%08x" % (u, o, l))


if __name__ == "__main__":
    main()
