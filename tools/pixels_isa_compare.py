"""pixels_kernel, parent against new: are the plain (STATS == false)
instantiations the parent's kernels instruction for instruction, and what do
the STATS ones cost in registers?

    hipcc <Makefile flags> -Rpass-analysis=kernel-resource-usage -c -o /dev/null csrc/smallpt.hip 2> RU.txt
    hipcc <Makefile flags> --cuda-device-only -S -o smallpt.s csrc/smallpt.hip
    python tools/pixels_isa_compare.py PARENT.s NEW.s NEW_RU.txt

A kernel's body is its instructions with operands, in order; block labels are
renumbered by first appearance, since a label carries the function's index in
the file.  The parent's pixels_kernel<GEO, DL> is matched with the new
pixels_kernel<GEO, DL, false>.  Then the resource table of all sixteen new
instantiations.  Exits non-zero if a plain kernel differs, or a kernel uses
scratch or spills VGPRs.
"""
import re
import sys


def bodies(path):
    """{(geo, dl, stats or None): [instruction lines]} of every pixels_kernel."""
    lines = open(path).read().split("\n")
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^(_ZN2rt7smallpt13pixels_kernelILi(\d)ELb(\d)E(?:Lb(\d)E)?E\w*):", lines[i])
        if not m:
            i += 1
            continue
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        labels, body = {}, []

        def norm(tok):
            return labels.setdefault(tok.group(0), "L%d" % len(labels))
        for l in lines[i + 1:end]:
            s = l.split(";")[0].strip()
            if not s or s.startswith("//") or (s.startswith(".") and not s.startswith(".LBB")):
                continue
            body.append(re.sub(r"\.LBB\d+_\d+", norm, s))
        out[(int(m.group(2)), int(m.group(3)), None if m.group(4) is None else int(m.group(4)))] = body
        i = end
    return out


def remarks(path):
    out, cur = {}, None
    for l in open(path):
        m = re.search(r"Function Name: _ZN2rt7smallpt13pixels_kernelILi(\d)ELb(\d)ELb(\d)E", l)
        if m:
            cur = out.setdefault(tuple(int(g) for g in m.groups()), {})
            continue
        if "Function Name:" in l:
            cur = None
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def main(parent_s, new_s, new_ru):
    old, new = bodies(parent_s), bodies(new_s)
    assert len(old) == 8 and len(new) == 16, (sorted(old), sorted(new))
    bad = 0
    print("# plain kernels against the parent's, instruction for instruction (labels renumbered)")
    for (geo, dl, _), a in sorted(old.items()):
        b = new[(geo, dl, 0)]
        same = a == b
        first = next((k for k, (p, q) in enumerate(zip(a, b)) if p != q), min(len(a), len(b)))
        print("pixels_kernel<%d, %s>: parent %d lines, new <.., false> %d lines: %s" % (
            geo, "true" if dl else "false", len(a), len(b), "identical" if same else "DIFFER at line %d" % first))
        bad += not same
    ru = remarks(new_ru)
    print("# resources of the new instantiations <GEO, DL, STATS>; instructions: lines of the body above")
    print("%-34s %5s %5s %11s %11s %8s %9s %13s" % ("kernel", "VGPR", "SGPR", "SGPR spill", "VGPR spill", "scratch",
                                                    "occupancy", "instructions"))
    for key in sorted(new):
        r = ru[key]
        n = sum(1 for s in new[key] if not s.endswith(":"))
        print("%-34s %5s %5s %11s %11s %8s %9s %13d" % (
            "pixels_kernel<%d, %s, %s>" % (key[0], "true" if key[1] else "false", "true" if key[2] else "false"),
            r["VGPRs"], r["TotalSGPRs"], r["SGPRs Spill"], r["VGPRs Spill"], r["ScratchSize"],
            r["Occupancy"], n))
        bad += r["VGPRs Spill"] != "0" or r["ScratchSize"].split()[0] != "0"
    print("%d problems" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
