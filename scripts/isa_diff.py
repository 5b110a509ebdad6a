#!/usr/bin/env python
"""CPU only: do two versions of the library's kernels compile to the same gfx950 code?

    python scripts/isa_diff.py <A> <B> ['k_rd_assign_rec<true>=k_rd_assign<true, true>' ...]

A and B are trees (every fast_slic_amd/csrc/*.hip is compiled with the Makefile's flags plus --cuda-device-only -S) or directories of
such listings (<unit>.s).  Per unit and kernel (demangled name without namespace and argument list; an `old=new` argument renames a
kernel of A) the instruction streams are compared with comments, directives and the function number of the local labels stripped:
IDENTICAL or the number of differing lines, then the VGPR / SGPR / LDS / scratch / kernarg figures of the kernel descriptor where
they differ.  The exit status is the number of kernels whose code differs or that exist on one side only."""
import difflib, glob, os, re, subprocess, sys, tempfile

META = {"next_free_vgpr": "VGPR", "next_free_sgpr": "SGPR", "group_segment_fixed_size": "LDS", "private_segment_fixed_size": "scratch",
        "kernarg_size": "kernarg"}


def listings(root):      # {unit: text of its -S listing}
    csrc = os.path.join(root, "fast_slic_amd", "csrc")
    if not os.path.isdir(csrc):
        return {os.path.basename(p)[:-2]: open(p).read() for p in sorted(glob.glob(os.path.join(root, "*.s")))}
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^FLAGS := (.*)$", mk, re.M).group(1).replace("$(LABFLAG)", "").split()
    extra = {u: f.split() for u, f in re.findall(r"^\$\(OBJDIR\)/(\w+)\.o: FLAGS \+= (.*)$", mk, re.M)}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
            unit = os.path.basename(src)[:-4]
            lst = os.path.join(tmp, unit + ".s")
            subprocess.run(["/opt/rocm/bin/hipcc"] + flags + extra.get(unit, []) + ["--cuda-device-only", "-S", "-o", lst, src],
                           check=True, stderr=subprocess.DEVNULL)
            out[unit] = open(lst).read()
    return out


def short(demangled):      # 'void fslic::k<1, true>(fslic::FrameDev, int)' -> 'k<1, true>'
    depth, i = 0, len(demangled)
    while i > 0:                                     # the '(' that opens the argument list
        i -= 1
        depth += {")": 1, "(": -1}.get(demangled[i], 0)
        if depth == 0 and demangled[i] == "(":
            break
    return re.sub(r"^void ", "", demangled[:i] if i else demangled).replace("fslic::", "")


def kernels(text, rename):      # {name: (instruction lines, {figure: value})} of one listing
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
            for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.M | re.S)}
    syms = sorted(desc)
    names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for sym, dem in zip(syms, names):
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(sym), text, re.M | re.S).group(1)
        code = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()) for l in body.split("\n")]
        code = [l for l in code if l and (not l.startswith(".") or l.startswith(".LBB_"))]
        name = short(dem)
        out[rename.get(name, name)] = (code, {v: desc[sym].get(k) for k, v in META.items()})
    return out


def main():
    rename = dict(a.split("=", 1) for a in sys.argv[3:])
    A, B = listings(sys.argv[1]), listings(sys.argv[2])
    bad = 0
    for unit in sorted(set(A) | set(B)):
        ka, kb = kernels(A.get(unit, ""), rename), kernels(B.get(unit, ""), {})
        for name in sorted(set(ka) | set(kb)):
            if name not in ka or name not in kb:
                verdict = "ONLY IN " + ("A" if name in ka else "B")
            else:
                n = sum(1 for l in difflib.unified_diff(ka[name][0], kb[name][0], n=0, lineterm="") if l[0] in "+-" and l[:3] not in ("+++", "---"))
                verdict = "IDENTICAL" if n == 0 else "%d lines differ" % n
                verdict += "".join("  [%s %s -> %s]" % (k, v, kb[name][1][k]) for k, v in ka[name][1].items() if v != kb[name][1][k])
            bad += not verdict.startswith("IDENTICAL")
            print("%-9s %-64s %s" % (unit, name, verdict))
    print("%d kernels differ" % bad)
    return bad


if __name__ == "__main__":
    sys.exit(main())
