"""Every kernel form of the assign family and of k_preempt_update, at small ragged shapes, bit for bit ("The form record").

The assign pass is a family of template instantiations picked by the spatial table, the stride, the mode and the SIZE of the launch
(assign.hip: launch_assign*, group.cpp: cluster_pass_fused), so the forms for chip-filling launches used to run on large tidy frames
only.  FSLIC_BLOCKS_SCALE multiplies the size the rules look at and nothing else; with it a frame of one or two blocks takes the
16- and 32-row forms, and meets a last column tile of one pixel, a frame shorter than a block, K = 1 and the like.

One child interpreter per switch setting (tests/assign_forms_child.py; the switches are read when the library is loaded) runs the whole
case table with FSLIC_GRAPH=0 and reports, per case, whether the results equal the reference's and which forms the call recorded
(Engine.forms_seen).  Reference: the plain-C oracle (labels, pre-connectivity labels, every Cluster byte), computed here once and
handed to the children in a file; for the preemptive mode the fixtures tests/golden/preemptive_form_cases.npz from the unmodified
reference.  The census: the union of the recorded forms over all children is the library's own complete list.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from fast_slic_amd import _binding as B
from fast_slic_amd.synth import variant
from test_gpu_deferred_labels import uncovered_in_some_pass

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Sizes the rules of assign.hip / group.cpp compare the launch size with: a scale equal to one of them puts a ONE-block launch exactly on
# the rule's low side and every launch of two blocks and more beyond it; the last value puts every launch beyond every rule.
SCALES = [1, 384, 640, 2048, 3072, 24576, 30000]
SETTINGS = [(s, fb) for fb in (None, 0, 2) for s in SCALES]


def setting_id(s):
    return "scale%d-fusebin%s" % (s[0], "default" if s[1] is None else s[1])


# ---- the case table --------------------------------------------------------------------------------------------------------------------
def K_for(H, W, target_S):
    """The largest K for which the frame's S (the oracle's) is at least target_S."""
    K = max(1, H * W // (target_S * target_S))
    while K > 1 and orc.S_of(H, W, K) < target_S:
        K -= 1
    return K


def mk(name, kind, H, W, K, stride=3, max_iter=10, compactness=10.0, manhattan=True, frames=1, scatter=None, table=None, pre=None,
       debug=False, want=()):
    return dict(name=name, kind=kind, H=H, W=W, K=K, stride=stride, max_iter=max_iter, compactness=compactness, manhattan=manhattan,
                frames=frames, scatter=scatter, table=table, pre=pre, debug=debug, want=tuple(want))


@functools.lru_cache(maxsize=None)
def case_table():
    cases = []
    # 1. heights: Hv = 1, 4R - 1, 4R, 4R + 1 visited rows for R = 8, 16, 32 at strides 1, 2, 3, on the 2-D table (S ~ 14) and on the
    # row-vector table (S >= 48); widths 63, 65, 130, 193 in turn, i.e. last column tiles of 63, 1, 2 and 1 pixels
    widths = [63, 65, 130, 193]
    for s in (1, 2, 3):
        for i, Hv in enumerate([1, 31, 32, 33, 63, 64, 65, 127, 128, 129]):
            H = Hv * s
            W = widths[(i + s) % 4]
            if H * W < 64:
                W = 65                                  # (S < 8 would be the generic kernel's)
            cases.append(mk("h2d_s%d_hv%d_%dx%d" % (s, Hv, H, W), "AB"[i % 2], H, W, K_for(H, W, 8) if H * W < 1600 else K_for(H, W, 14),
                            stride=s, max_iter=(10, 4, 2)[i % 3], table="2d"))
            if H * W < 2500:                            # the smallest frame that has S >= 48 with this height (K = 1)
                W = (2500 // H) // 64 * 64 + 65 if H < 31 else 79
            cases.append(mk("hrv_s%d_hv%d_%dx%d" % (s, Hv, H, W), "BA"[i % 2], H, W, K_for(H, W, 49),
                            stride=s, max_iter=(4, 10, 3)[i % 3], table="rowvec"))
    # 2. one-block frames (every pass is ONE eight-row block, so the launch size is the scale itself) and two-block frames: the cases that
    # pin each rule at its value
    for s in (1, 2, 3):
        cases.append(mk("pin2d_s%d_32x63" % s, "A", 32, 63, K_for(32, 63, 12), stride=s, table="2d", want=("pin",)))
        # (K = 1 and S >= 48, 45 at stride 3: the fused passes at strides 2 and 3 are one block, and at stride 3 the full pass too)
        cases.append(mk("pinrv_s%d" % s, "B", 32 if s == 3 else 37, 64 if s == 3 else 63, 1, stride=s, table="rowvec", want=("pin",)))
    # 3. either side of the cut between the two tables (the 2-D table's bytes crossing 12288): S = 44 | 45 at stride 3, 47 | 48 below
    for s, S_lo in ((3, 44), (2, 47), (1, 47)):
        for S in (S_lo, S_lo + 1):
            H, W = 2 * S + 1, 3 * S + 2
            K = next(k for k in range(1, 64) if orc.S_of(H, W, k) == S)
            cases.append(mk("cut_s%d_S%d_%dx%d" % (s, S, H, W), "A", H, W, K, stride=s, max_iter=3, table="2d" if S == S_lo else "rowvec", want=("cut",)))
    # 4. parameters: compactness 1 and 80, the Euclidean patch, stride 5 (the 32-bit kernel), max_iter 0, 1, 2
    cases += [
        mk("c1_2d_97x130", "A", 97, 130, K_for(97, 130, 16), compactness=1.0, table="2d"),
        mk("c1_rv_129x193", "B", 129, 193, K_for(129, 193, 50), compactness=1.0, stride=2, table="rowvec"),
        mk("c80_manh_97x130", "A", 97, 130, K_for(97, 130, 16), compactness=80.0, table="k32"),
        # (the Euclidean patch stays below the packed kernel's distance limit at compactness 80, sqrt(2) S against the Manhattan 2 S)
        mk("c80_eucl_97x130", "B", 97, 130, K_for(97, 130, 16), compactness=80.0, manhattan=False, stride=2, table="2d"),
        mk("c120_eucl_97x130", "B", 97, 130, K_for(97, 130, 16), compactness=120.0, manhattan=False, stride=2, table="k32"),
        mk("c120_eucl_33x63", "B", 33, 63, K_for(33, 63, 12), compactness=120.0, manhattan=False, stride=1, table="k32"),
        mk("eucl_2d_65x193", "A", 65, 193, K_for(65, 193, 14), manhattan=False, table="2d"),
        mk("s5_2d_131x130", "A", 131, 130, K_for(131, 130, 14), stride=5, table="k32"),
        mk("s5_rv_161x193", "B", 161, 193, K_for(161, 193, 50), stride=5, max_iter=7, table="k32"),
        mk("s5_eucl_131x65", "A", 131, 65, K_for(131, 65, 14), stride=5, manhattan=False, table="k32"),
        mk("it0_2d_33x65", "A", 33, 65, K_for(33, 65, 12), max_iter=0, table="2d"),
        mk("it0_rv_97x130", "B", 97, 130, K_for(97, 130, 50), max_iter=0, table="rowvec"),
        mk("it1_2d_65x130", "A", 65, 130, K_for(65, 130, 14), max_iter=1, table="2d"),
        mk("it1_rv_129x130", "B", 129, 130, K_for(129, 130, 50), max_iter=1, stride=2, table="rowvec"),
        mk("it2_2d_63x63", "B", 63, 63, K_for(63, 63, 14), max_iter=2, stride=1, table="2d"),
        # a height below the stride: the passes of the residues >= H visit nothing (group.cpp, every_pass_has_rows)
        mk("short_2x130", "A", 2, 130, 1, stride=3, max_iter=5, table="2d"),
        mk("short_1x193", "B", 1, 193, 1, stride=2, max_iter=4, table="2d"),
        # K = 1 on a frame the single window covers, and S < 8: the generic kernel; debug_mode: its recording form
        mk("k1_31x33", "A", 31, 33, 1, stride=2, table="2d"),
        mk("generic_40x63", "A", 40, 63, 100, table="generic"),
        mk("record_40x65", "B", 40, 65, 20, max_iter=3, debug=True, table="generic"),
        # S of 412 .. 419 at stride 1: the full pass's row-vector table is the 16-row one alone (tables.cpp, rows32); at stride 3 the
        # subsampled table no longer fits and the 32-bit kernel takes the frame, as it does from S = 420 on at every stride
        mk("S415_353x488", "A", 353, 488, 1, max_iter=2, stride=1, table="rowvec412"),
        mk("S415_s3_353x488", "A", 353, 488, 1, max_iter=2, stride=3, table="k32"),
        mk("S425_361x501", "B", 361, 501, 1, max_iter=2, stride=2, table="k32"),
    ]
    # 5. a K whose last grid row of centres lies on the last image row
    for H, W in ((97, 130), (131, 193)):
        K = next(k for k in range(4, 400) if int(orc.initialize_clusters(variant("A", H, W), k)["y"].max()) == H - 1)
        cases.append(mk("lastrow_%dx%d_k%d" % (H, W, K), "A", H, W, K, stride=2, max_iter=4, table="2d", want=("lastrow",)))
    # 6. groups of two and three frames
    cases += [
        mk("group2_2d_65x130", "A", 65, 130, K_for(65, 130, 14), frames=2, table="2d"),
        mk("group3_rv_129x193", "B", 129, 193, K_for(129, 193, 50), frames=3, stride=2, max_iter=4, table="rowvec"),
        mk("group3_2d_33x193", "A", 33, 193, K_for(33, 193, 12), frames=3, stride=1, max_iter=3, table="2d"),
    ]
    # 7. centres scattered at random leave visited pixels outside every window: redone with storing passes, one per table form and stride
    for s in (1, 2, 3):
        cases.append(mk("scat2d_s%d" % s, "A", 97 + s, 130 + s, K_for(97 + s, 130 + s, 14), stride=s, max_iter=4, scatter=40 + s, table="2d"))
        cases.append(mk("scatrv_s%d" % s, "B", 129 + s, 193 + s, K_for(129 + s, 193 + s, 50), stride=s, max_iter=4, scatter=50 + s, table="rowvec"))
    cases.append(mk("scat415", "A", 353, 489, 1, max_iter=2, stride=1, scatter=60, table="rowvec412"))
    # 8. the preemptive mode: the fixtures of the unmodified reference
    fx = np.load(os.path.join(ROOT, "tests", "golden", "preemptive_form_cases.npz"), allow_pickle=False)
    for name in sorted({k.split("/")[0] for k in fx.files}):
        H, W, K = (int(v) for v in fx[name + "/shape"])
        kw = json.loads(str(fx[name + "/kwargs"]))
        cases.append(mk(name, str(fx[name + "/variant"]), H, W, K, stride=kw.get("subsample_stride", 3), max_iter=kw.get("max_iter", 10),
                        compactness=kw.get("compactness", 10.0), pre=float(fx[name + "/thres"]),
                        table="rowvec" if "rowvec" in name else "2d" if "_2d_" in name else "generic"))
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


@functools.lru_cache(maxsize=None)
def references():
    """name -> (per-frame inputs, expected results, whether some pass visits a pixel no window covers); computed once, never modified."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "preemptive_form_cases.npz"), allow_pickle=False)
    out = {}
    for c in case_table():
        frames = []
        for z in range(c["frames"]):
            if c["pre"] is not None:
                img = np.ascontiguousarray(variant(c["kind"], c["H"], c["W"]))       # (the fixture's input)
            else:
                img = np.ascontiguousarray(variant("AB"[("AB".index(c["kind"]) + z) & 1], c["H"], c["W"], seed=11 + z))
            cl0 = orc.initialize_clusters(img, c["K"])
            if c["scatter"] is not None:
                rng = np.random.RandomState(c["scatter"] + z)
                cl0["y"] = rng.randint(0, c["H"], c["K"]).astype(np.float32)
                cl0["x"] = rng.randint(0, c["W"], c["K"]).astype(np.float32)
            if c["pre"] is not None:
                labels, cl, pre = fx[c["name"] + "/labels"], fx[c["name"] + "/clusters"], fx[c["name"] + "/prelabels"]
                unc = False
            else:
                labels, cl, _, pre = orc.slic_iterate(img, cl0.copy(), stages=True, max_iter=c["max_iter"], compactness=c["compactness"],
                                                      subsample_stride=c["stride"], manhattan=c["manhattan"])
                unc = uncovered_in_some_pass(img, cl0, c["stride"], c["max_iter"]) if c["compactness"] == 10.0 and c["manhattan"] else None
            frames.append((img, cl0, labels, cl, pre, unc))
        out[c["name"]] = frames
    return out


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("assign_forms") / "cases.npz")
    arrays = {"names": np.array(json.dumps([c["name"] for c in case_table()]))}
    for c in case_table():
        for z, (img, cl0, labels, cl, pre, _) in enumerate(references()[c["name"]]):
            arrays["%s/image%d" % (c["name"], z)] = img
            arrays["%s/cl0_%d" % (c["name"], z)] = np.frombuffer(cl0.tobytes(), np.uint8)
            arrays["%s/labels%d" % (c["name"], z)] = labels
            arrays["%s/clusters%d" % (c["name"], z)] = np.frombuffer(cl.tobytes(), np.uint8)
            arrays["%s/prelabels%d" % (c["name"], z)] = pre
        arrays[c["name"] + "/meta"] = np.array(json.dumps(dict(
            frames=c["frames"], max_iter=c["max_iter"], compactness=c["compactness"], stride=c["stride"], manhattan=c["manhattan"],
            preemptive=c["pre"] is not None, thres=c["pre"] or 0.05, debug=c["debug"], own_engine=c["scatter"] is not None or c["name"] in TWICE,
            twice=c["name"] in TWICE)))
    np.savez(path, **arrays)
    return path


# run twice on a slot of their own: a covered frame whose 16-row blocks overflow their candidate lists, and a scattered one for contrast
OVERFLOWING, TWICE = "h2d_s2_hv129_258x193", ("h2d_s2_hv129_258x193", "scat2d_s2")
_results = {}


def child(setting, cases_file):
    """The child of one switch setting, run once (a timeout of its own)."""
    if setting not in _results:
        scale, fusebin = setting
        env = dict(os.environ, FSLIC_BLOCKS_SCALE=str(scale), FSLIC_GRAPH="0")
        env.pop("FSLIC_FUSEBIN", None)
        if fusebin is not None:
            env["FSLIC_FUSEBIN"] = str(fusebin)
        out = cases_file[:-4] + "." + setting_id(setting) + ".json"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "assign_forms_child.py"), cases_file, out], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):      # killed by a signal: nothing more is started on the GPU
            pytest.exit("%s: the child ended with %d\n%s" % (setting_id(setting), r.returncode, r.stdout.decode()[-3000:]), returncode=3)
        assert r.returncode == 0, "%s: exit %d\n%s" % (setting_id(setting), r.returncode, r.stdout.decode()[-3000:])
        with open(out) as f:
            _results[setting] = json.load(f)
    return _results[setting]


# ---- the forms a case was written for ---------------------------------------------------------------------------------------------------
def blocks8(c, Hv):
    return c["frames"] * ((c["W"] + 63) // 64) * ((Hv + 31) // 32)


def has_tabs16(S, stride):
    """tables.cpp keeps the subsampled stride's 2-D table for 16 rows per wavefront (`tabs16`) while it is at most 16 KB."""
    return ((S + 2) * ((2 * (S + 15 * stride) + 1) | 1) * 4 + 15) // 16 * 16 <= 16384


def written_for(c, setting):
    """Forms an integer-SLIC case on the block kernel must have recorded under the setting, at every scale: the size of each of its
    passes is the library's measure (eight-row blocks of the pass, times the scale), what each side of a rule selects is the design's
    statement ("The form record"), and the record is the library's.  A scale equal to a rule's value puts a one-block pass
    exactly on the rule's low side.  Other cases (32-bit and generic kernels, preemptive, recording, scattered centres) assert their
    family in the test below."""
    scale, fusebin = setting
    if c["table"] not in ("2d", "rowvec") or c["pre"] is not None or c["debug"] or c["scatter"] is not None:
        return set()
    s, S, rv = c["stride"], orc.S_of(c["H"], c["W"], c["K"]), c["table"] == "rowvec"
    rows = [(c["H"] - rem + s - 1) // s for rem in range(min(s, c["max_iter"]))]
    fused = {blocks8(c, hv) * scale for hv in rows if hv > 0}      # (a height below the stride: the passes of the other residues launch nothing)
    full = blocks8(c, c["H"]) * scale
    first = blocks8(c, (c["H"] + s - 1) // s) * scale
    # the cluster pass rides on the assign launches of small groups (or all, FSLIC_FUSEBIN=2) whose every pass has rows; the other
    # groups run label-free when they have a subsampled pass at all
    bin_pass = (fusebin == 2 or (fusebin is None and first <= 640)) and c["H"] >= s
    nolab = not bin_pass and c["max_iter"] >= 1
    rows_full = 32 if rv and full > 24576 else 16 if full > 3072 else 8
    want = {"blk r%d full s1 %s %s" % (rows_full, "rowvec" if rows_full == 32 else "rowvec16" if rv else "2d", "nolab" if nolab else "lab")}
    for b in fused:
        if bin_pass:
            if rv:
                want.add("bin r%d fused s%d rowvec lab" % (16 if b > 3072 else 8, s))
            else:
                want.add("bin r4 fused s3 2d lab" if s == 3 and b <= 384 else "bin r8 fused s%d 2d lab" % s)
        elif rv:
            want.add("blk r%d fused s%d rowvec nolab" % (16 if b > 3072 else 8, s))
        else:
            want.add("blk r16 fused s%d tabs16 nolab" % s if b > 2048 and has_tabs16(S, s) else "blk r8 fused s%d 2d nolab" % s)
    return want


@pytest.mark.parametrize("setting", SETTINGS, ids=setting_id)
def test_every_case_is_bit_equal_and_takes_the_form_it_was_written_for(setting, cases_file):
    res = child(setting, cases_file)
    bad = ["%s: %s" % (n, v["msg"]) for n, v in res["cases"].items() if not v["ok"]]
    assert not bad, "%s\n%s" % (setting_id(setting), "\n".join(bad)[:6000])
    wrong = []
    for c in case_table():
        got = set(res["cases"][c["name"]]["forms"])
        want = written_for(c, setting)
        refs = references()[c["name"]]
        print("%-28s S=%-3d %s" % (c["name"], orc.S_of(c["H"], c["W"], c["K"]), sorted(got)))
        if c["scatter"] is None and not (want <= got):
            wrong.append("%s: written for %s, recorded %s" % (c["name"], sorted(want - got), sorted(got)))
        # the families: every pass of a preemptive call, of a recording call and of a frame with S < 8 is of its own family
        fams = {f.split()[0] for f in got}
        if c["H"] < c["stride"]:
            assert "bin" not in fams, (c["name"], got)      # (group.cpp, every_pass_has_rows: no cluster pass can ride on a pass without rows)
        if c["pre"] is not None:
            assert "preempt_update" in fams and fams <= {"pre", "generic", "blk", "preempt_update"}, (c["name"], got)
            if c["table"] != "generic":
                assert any(f.startswith("pre r8 fused s%d %s" % (c["stride"], c["table"])) for f in got), (c["name"], got)
            else:
                assert ("preempt_update lists" in got) == (c["K"] <= 8192) and ("preempt_update allpairs" in got) == (c["K"] > 8192), (c["name"], got)
        elif c["debug"]:
            assert "generic_rec fused srt notab lab" in got, (c["name"], got)
        elif c["table"] == "generic":
            assert fams == {"generic"}, (c["name"], got)
        elif c["table"] == "k32":
            assert "k32" in fams, (c["name"], got)
        elif c["table"] == "rowvec412":
            assert any(f.startswith("blk") and f.split()[2] == "full" and f.split()[4] == "rowvec" and f.split()[1] != "r32" for f in got), (c["name"], got)
        # label-free passes: a covered input is never redone; an uncovered one is, with storing passes, exactly when its passes were label-free
        unc = [r[5] for r in refs]
        nolab_fused = any(f.split()[-1] == "nolab" for f in got)
        if all(u is False for u in unc):      # (also where a candidate list overflowed and the frame was redone generically)
            assert res["cases"][c["name"]]["redos"] == 0, (c["name"], got)
        if c["table"] != "generic" and "generic" in fams:
            continue      # (an overflow -- 64 rows of a block at S = 14 see more than 64 centres: the generic redo is not the storing one)
        if nolab_fused and all(u is not None for u in unc):
            assert res["cases"][c["name"]]["redos"] == sum(unc), (c["name"], unc, got)
            if any(unc) and c["max_iter"] >= 1:
                assert any(f.startswith("blk") and f.split()[2] == "fused" and f.split()[-1] == "lab" for f in got), (c["name"], got)
    assert not wrong, "%s\n%s" % (setting_id(setting), "\n".join(wrong))
    if setting[1] == 0 or (setting[1] is None and setting[0] > 640):
        covered_nolab = [c["name"] for c in case_table() if any(f.endswith("fused s%d %s nolab" % (c["stride"], t)) for f in res["cases"][c["name"]]["forms"] for t in ("2d", "tabs16", "rowvec"))
                         and res["cases"][c["name"]]["redos"] == 0]
        assert len(covered_nolab) >= 40, "too few covered inputs took the label-free passes: %s" % covered_nolab


def test_the_cut_between_the_tables_is_where_the_record_says(cases_file):
    """S on both sides of the row-vector cut-over, the table read from the record (scale 1, the cluster pass separate)."""
    res = child((1, 0), cases_file)
    for c in case_table():
        if "cut" in c["want"]:
            tabs = {f.split()[4] for f in res["cases"][c["name"]]["forms"] if f.split()[2] == "fused"}
            assert tabs == {c["table"]}, (c["name"], res["cases"][c["name"]]["forms"])


def test_scattered_inputs_are_redone_with_storing_passes(cases_file):
    res = child((1, 0), cases_file)
    for c in case_table():
        if c["scatter"] is not None:
            v = res["cases"][c["name"]]
            assert any(r[5] for r in references()[c["name"]]), c["name"] + ": the input was meant to leave uncovered pixels"
            assert v["redos"] > 0 and any(f.split()[-1] == "nolab" for f in v["forms"]) and any(f.split()[2] == "fused" and f.split()[-1] == "lab" for f in v["forms"]), (c["name"], v)


def test_an_overflowing_covered_frame_is_not_an_uncovered_redo(cases_file):
    """A block whose candidate list overflows assigns nothing, so the rest of that attempt may well meet uncovered pixels; the frame is
    redone with the generic kernel, which is neither an uncovered redo nor a reason to put the slot on the storing passes (group.cpp,
    group_finish).  16-row blocks at stride 2 and S = 14 overflow on a covered 258x193 frame; a scattered frame for contrast."""
    res = child((3072, 0), cases_file)
    assert not any(r[5] for r in references()[OVERFLOWING]), "the input was meant to cover every pixel"
    v = res["cases"][OVERFLOWING]
    assert v["ok"], v["msg"]
    assert "generic fused srt notab lab" in v["forms"] and "blk r16 fused s2 tabs16 nolab" in v["forms"], v["forms"]      # it did overflow
    assert v["redos"] == 0 and v["redos2"] == 0, v
    assert "blk r16 fused s2 tabs16 nolab" in v["forms2"] and not any(f.startswith("blk") and f.endswith(" lab") and " fused " in f for f in v["forms2"]), v["forms2"]
    # (8-row blocks, scale 1) the storing redo is counted once and sticks: the second call stores from the start
    w = child((1, 0), cases_file)["cases"]["scat2d_s2"]
    assert w["ok"] and w["redos"] == 1 and w["redos2"] == 0, w
    assert any(f.endswith("nolab") for f in w["forms"]) and not any(f.endswith("nolab") for f in w["forms2"]), w


def test_census_every_listed_form_ran(cases_file):
    """The union of the forms recorded over all children is the library's complete list: no form is left out, none is unlisted."""
    seen, everything = set(), None
    where = {}
    for setting in SETTINGS:
        res = child(setting, cases_file)
        everything = set(res["all"]) if everything is None else everything
        assert set(res["all"]) == everything
        for n, v in res["cases"].items():
            for f in v["forms"]:
                seen.add(f)
                where.setdefault(f, "%s under %s" % (n, setting_id(setting)))
    for f in sorted(where):
        print("%-40s first: %s" % (f, where[f]))
    assert everything == set(B.forms_all())
    assert seen == everything, "never run: %s; not listed: %s" % (sorted(everything - seen), sorted(seen - everything))
