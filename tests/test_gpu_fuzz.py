"""A fixed stretch of every mode of tests/fuzz_parity.py (the randomized sweep that found three defects in round 6: DESIGN.md section 13)
as part of the suite: seeds and case counts are fixed, so every run covers the same cases.  Each mode runs in a child process (one engine
per sequence on purpose -- arenas are re-carved over what earlier geometries left -- and a device fault must not take the session with it).

The time budget handed to the sweep is effectively unlimited: FUZZ_CASES alone ends a stretch, and the count the sweep prints at its end is
compared with it (with a budget of 600 s a slow machine ended a stretch early, with exit 0 and fewer cases than the suite claims to run)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NEEDS_REF = {"variants", "graph"}
NO_BUDGET = "1000000"


def run_stretch(mode, seed, cases, extra_env=None):
    if mode in NEEDS_REF and not os.path.exists(os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libfslic_ref.so")):
        pytest.skip("oracle/_ref (the reference build) is not present")
    args = [sys.executable, os.path.join(HERE, "fuzz_parity.py"), str(seed), NO_BUDGET] + ([] if mode == "slic" else [mode])
    r = subprocess.run(args, env=dict(os.environ, FUZZ_CASES=str(cases), **(extra_env or {})), capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    last = r.stdout.splitlines()[-1]
    assert "fuzz_parity" in last, tail
    done = int(re.search(r": (\d+) (?:cases|maps|submissions)", last).group(1))
    assert done == cases, "the stretch ran %d of %d cases\n%s" % (done, cases, tail)
    return last


@pytest.mark.parametrize("mode,seed,cases", [("slic", 11, 60), ("variants", 11, 80), ("warm", 11, 120), ("cca", 11, 400),
                                             ("lsc", 11, 60), ("pipeline", 11, 150), ("graph", 11, 60)])
def test_fixed_stretch_of_the_randomized_sweep(mode, seed, cases):
    run_stretch(mode, seed, cases)


# The forms the launch size selects (16 rows per wavefront from 3072 eight-row blocks on, 32 from 24576 on: assign.hip) on the sweep's own
# shapes: FSLIC_BLOCKS_SCALE (engine_internal.h) multiplies the size the rules see, so that every launch of the stretch lies beyond the rule.
@pytest.mark.parametrize("shapes,cases", [("tiny", 150), ("", 10)], ids=["tiny", "default"])
@pytest.mark.parametrize("scale,rows", [(3073, "r16"), (24577, "r32")])
@pytest.mark.parametrize("mode", ["slic", "variants"])
def test_fixed_stretch_with_the_forms_of_chip_filling_launches(mode, scale, rows, shapes, cases):      # noqa: ARG001 (rows: the id)
    last = run_stretch(mode, 23, cases, dict(FSLIC_BLOCKS_SCALE=str(scale), FUZZ_SHAPES=shapes))
    forms = last.split("; forms ")[1]
    print(last)
    # every launch of the stretch lies beyond the rule, whatever its frame: no full pass of the block kernel or of the 32-bit kernel
    # may have kept 8 rows per wavefront (tiny shapes and the variants are mostly other kernels' work, but this holds for all)
    assert "blk r8 full" not in forms and "k32 r8 full" not in forms, last
    # the default shapes of the slic mode draw block-kernel frames on both tables (superpixel sides of 6 .. 60): 16 rows beyond 3072
    # on the 2-D table, and beyond 24576 the 32 rows of the row-vector table
    if mode == "slic" and shapes == "":
        assert "blk r16 full" in forms, last
        if scale > 24576:
            assert "blk r32 full" in forms, last
