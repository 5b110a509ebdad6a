"""CPU check of the form record's boundary (csrc/forms.h, DESIGN.md "The form record"): both debug entry points are declared in
include/fslic_hip.h, exported by the library and bound, and the complete list of forms is a set that decodes to distinct names.  No
kernel is launched here."""
import ctypes
import os
import re

from fast_slic_amd import _binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_form_record_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fslic_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+fslic_hip_debug_forms_seen\s*\(\s*uint32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+fslic_hip_debug_forms_all\s*\(\s*uint32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    lib = B.load_library()
    for name in ("fslic_hip_debug_forms_seen", "fslic_hip_debug_forms_all"):
        assert hasattr(lib, name) and name in B.EXPORTS
    assert lib.fslic_hip_debug_forms_seen(None, 4, 0) == -1 and lib.fslic_hip_debug_forms_all(None, 4) == -1      # no buffer: refused
    assert lib.fslic_hip_debug_forms_seen(None, 0, 0) >= 0      # the count alone
    assert callable(B.forms_seen) and callable(B.forms_all) and callable(B.form_name)
    assert isinstance(B.forms_seen(), set)


def test_complete_list_has_no_duplicates_and_decodes_to_distinct_names():
    lib = B.load_library()
    n = lib.fslic_hip_debug_forms_all(None, 0)
    assert n > 0
    short = (ctypes.c_uint32 * 3)()
    assert lib.fslic_hip_debug_forms_all(short, 3) == n      # a short buffer takes what fits and still learns the length
    codes = B.form_codes_all()
    assert len(codes) == n and list(short) == codes[:3]
    assert len(set(codes)) == n, "a form is listed twice"
    names = B.forms_all()
    assert len(set(names)) == n, "two codes decode to one name"
    assert not any(re.search(r"\b(family|table)\d", x) for x in names), names      # (every field decodes to a word, none to its number)
    assert "blk r16 fused s2 rowvec nolab" in names and "preempt_update allpairs" in names and "k32 r8 fused srt lut lab" in names
    # every family of the dispatch appears
    assert {x.split()[0] for x in names} == set(B.FORM_FAMILIES.values())


def test_the_set_of_forms_is_the_pinned_one():
    """tests/golden/assign_forms.txt: the names of forms_all() as the library listed them before the forms became rows of one table
    (csrc/assign.hip, csrc/preempt.hip).  A row lost or added is a form lost or added."""
    pinned = open(os.path.join(ROOT, "tests", "golden", "assign_forms.txt")).read().split("\n")
    pinned = [x for x in pinned if x]
    assert len(pinned) == len(set(pinned)) == 65
    names = set(B.forms_all())
    assert names == set(pinned), (sorted(names - set(pinned)), sorted(set(pinned) - names))
