"""CPU check of the boundary the label-free assign passes added: the redo counter is declared in include/fslic_hip.h, exported by
the library and bound as Engine.uncovered_redos.  No kernel is launched here."""
import os
import re

from fast_slic_amd import _binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_uncovered_redos_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fslic_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+fslic_hip_uncovered_redos\s*\(\s*fslic_engine\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    lib = B.load_library()
    assert hasattr(lib, "fslic_hip_uncovered_redos")
    assert "fslic_hip_uncovered_redos" in B.EXPORTS
    assert lib.fslic_hip_uncovered_redos(None, 0) == -1      # no engine: refused like the other per-slot counters
    assert callable(getattr(B.Engine, "uncovered_redos"))
