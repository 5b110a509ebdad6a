"""One interpreter of tests/test_gpu_assign_forms.py: the library reads FSLIC_BLOCKS_SCALE / FSLIC_FUSEBIN / FSLIC_GRAPH when it is
loaded, so every switch setting runs the whole case table in a process of its own.

    python tests/assign_forms_child.py <cases.npz> <result.json>

cases.npz holds, per case, the inputs and the expected results (the plain-C oracle's, or the reference fixtures of the preemptive mode),
written once by the parent.  Every call clears the form record first, so what is read back afterwards is that call's (FSLIC_GRAPH=0: no
replay).  result.json: per case whether labels, pre-connectivity labels and every Cluster byte were equal, the forms the call
recorded and by how much Engine.uncovered_redos moved; for the cases marked `twice` the same of a second call of the same work.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fast_slic_amd import _binding as B  # noqa: E402
from fast_slic_amd import Engine, make_params  # noqa: E402
from util import describe_mismatch, cluster_fields_equal  # noqa: E402


def run_case(eng, name, c):
    meta = json.loads(str(c[name + "/meta"]))
    n = meta["frames"]
    imgs = [np.ascontiguousarray(c["%s/image%d" % (name, i)]) for i in range(n)]
    H, W = imgs[0].shape[:2]
    cls = [c["%s/cl0_%d" % (name, i)].copy().view(B.CLUSTER_DTYPE) for i in range(n)]
    p = make_params(meta["max_iter"], meta["compactness"], 0.25, meta["stride"], True, meta["manhattan"],
                    preemptive=meta["preemptive"], preemptive_thres=meta["thres"], debug_mode=meta["debug"])
    before = eng.uncovered_redos()
    B.forms_seen(clear=True)
    if n == 1:
        labels = [eng.iterate(imgs[0], cls[0], p)]
        pre = eng.last_prelabels(H, W)
    else:
        labels = [np.zeros((H, W), np.uint16) for _ in range(n)]
        eng.iterate_batch([im.ctypes.data for im in imgs], cls, [o.ctypes.data for o in labels], H, W, p, False)
        pre = None                      # (the plane the library hands out is that of the group's first frame: checked on single frames)
    forms = sorted(B.forms_seen(clear=True))
    msgs = []
    for i in range(n):
        exp_labels, exp_cl = c["%s/labels%d" % (name, i)], c["%s/clusters%d" % (name, i)]
        if not np.array_equal(labels[i], exp_labels):
            msgs.append(describe_mismatch("%s/labels of frame %d" % (name, i), labels[i], exp_labels))
        if cls[i].tobytes() != exp_cl.tobytes():
            msgs.append("%s frame %d clusters: %s" % (name, i, "; ".join(cluster_fields_equal(cls[i], exp_cl)) or "bytes differ"))
    if pre is not None and not np.array_equal(pre, c[name + "/prelabels0"]):
        msgs.append(describe_mismatch(name + "/prelabels", pre, c[name + "/prelabels0"]))
    out = {"ok": not msgs, "msg": "\n".join(msgs)[:2000], "forms": forms, "redos": eng.uncovered_redos() - before}
    if meta["twice"] and n == 1:        # the same work once more on the same slot: has the slot been put on the storing passes?
        again = eng.uncovered_redos()
        cl2 = c[name + "/cl0_0"].copy().view(B.CLUSTER_DTYPE)
        labels2 = eng.iterate(imgs[0], cl2, p)
        out["forms2"] = sorted(B.forms_seen(clear=True))
        out["redos2"] = eng.uncovered_redos() - again
        if not np.array_equal(labels2, c[name + "/labels0"]) or cl2.tobytes() != c[name + "/clusters0"].tobytes():
            out["ok"], out["msg"] = False, out["msg"] + "\n%s: the second call of the same work differs" % name
    return out


def main():
    cases_path, out_path = sys.argv[1], sys.argv[2]
    c = np.load(cases_path, allow_pickle=False)
    names = json.loads(str(c["names"]))
    out = {"all": B.forms_all(), "cases": {}}
    eng = Engine(0, 1)
    try:
        for name in names:
            meta = json.loads(str(c[name + "/meta"]))
            if meta["own_engine"]:      # a frame that is redone leaves its slot on the storing passes for that work: a slot of its own
                e2 = Engine(0, 1)
                try:
                    out["cases"][name] = run_case(e2, name, c)
                finally:
                    e2.close()
            else:
                out["cases"][name] = run_case(eng, name, c)
    finally:
        eng.close()
    with open(out_path, "w") as f:
        json.dump(out, f)
    print("cases", len(names), "failed", sum(not v["ok"] for v in out["cases"].values()))


if __name__ == "__main__":
    main()
