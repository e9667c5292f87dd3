"""Per-kernel resource guard of a change to smallpt.hip: registers, scratch,
occupancy and scalar spills from hipcc's kernel-resource-usage remarks, and
static VALU / SALU, f64 VALU, v_readlane / v_writelane (inside loops and
outside) and scratch instructions from the device assembly, parent against new.

    hipcc <Makefile flags> -Rpass-analysis=kernel-resource-usage -c -o /dev/null csrc/smallpt.hip 2> RU.txt
    hipcc <Makefile flags> --cuda-device-only -S -o smallpt.s csrc/smallpt.hip
    python tools/resource_guard.py PARENT.s PARENT_RU.txt NEW.s NEW_RU.txt

One block per kernel that differs; a line starting with "GUARD" for every
kernel that gains scratch, loses occupancy or gains a lane copy inside a loop
(the rule of profiles/r12 and r17), and a last line with their count.
"""
import collections
import re
import sys


def remarks(path):
    out, cur = {}, None
    for l in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", l)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def kernels(path):
    """{kernel: Counter} of static instruction classes; lane copies split by loop depth."""
    lines = open(path).read().split("\n")
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        ops, label_pos, branches = [], {}, []
        for l in lines[i + 1:end]:
            s = l.strip()
            if not s or s.startswith(";") or s.startswith("//"):
                continue
            lm = re.match(r"^(\.LBB\w+):", s)
            if lm:
                label_pos[lm.group(1)] = len(ops)
                continue
            if s.startswith(".") or s.endswith(":"):
                continue
            op = s.split()[0]
            if op.startswith("s_cbranch") or op.startswith("s_branch"):
                branches.append((len(ops), s.split()[-1]))
            ops.append(op)
        inloop = [False] * len(ops)
        for bi, tgt in branches:
            if tgt in label_pos and label_pos[tgt] <= bi:
                for k in range(label_pos[tgt], bi + 1):
                    inloop[k] = True
        c = collections.Counter()
        for k, op in enumerate(ops):
            if op.startswith("v_readlane") or op.startswith("v_writelane"):
                c[op[:10].rstrip("_") + (" in-loop" if inloop[k] else " out")] += 1
            elif op.startswith("scratch_"):
                c["scratch"] += 1
            elif op.startswith("v_"):
                c["valu"] += 1
                if op.endswith("_f64") or "_f64_" in op:
                    c["f64"] += 1
            elif op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch")):
                c["salu"] += 1
        out[name] = c
        i = end
    return out


def main():
    pa, pr, na, nr = sys.argv[1:5]
    A, B = kernels(pa), kernels(na)
    RA, RB = remarks(pr), remarks(nr)
    names = [k for k in A if k in B]
    print("%d kernels in both; only in parent: %d, only in new: %d" % (len(names), len(set(A) - set(B)), len(set(B) - set(A))))
    same, broken = 0, 0
    for k in names:
        a, b, ra, rb = A[k], B[k], RA.get(k, {}), RB.get(k, {})
        if a == b and ra == rb:
            same += 1
            continue
        short = re.sub(r"^_ZN2rt7smallpt", "", k)[:60]
        print("%s\n     v %d->%d  f64 %d->%d  s %d->%d  readlane in-loop %d->%d out %d->%d | writelane in-loop %d->%d out %d->%d | scratch %d->%d"
              % (short, a["valu"], b["valu"], a["f64"], b["f64"], a["salu"], b["salu"],
                 a["v_readlane in-loop"], b["v_readlane in-loop"], a["v_readlane out"], b["v_readlane out"],
                 a["v_writelan in-loop"], b["v_writelan in-loop"], a["v_writelan out"], b["v_writelan out"],
                 a["scratch"], b["scratch"]))
        keys = ["TotalSGPRs", "VGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill"]
        print("     " + "  ".join("%s %s->%s" % (q, ra.get(q, "?"), rb.get(q, "?")) for q in keys))
        why = []
        if int(rb.get("ScratchSize", 0)) > int(ra.get("ScratchSize", 0)) or b["scratch"] > a["scratch"]:
            why.append("scratch")
        if int(rb.get("Occupancy", 0)) < int(ra.get("Occupancy", 0)):
            why.append("occupancy")
        if b["v_readlane in-loop"] > a["v_readlane in-loop"] or b["v_writelan in-loop"] > a["v_writelan in-loop"]:
            why.append("lane copies inside a loop")
        if why:
            broken += 1
            print("GUARD %s: %s" % (short, ", ".join(why)))
    print("%d kernels identical in counts and resources; %d kernels break the guard" % (same, broken))


if __name__ == "__main__":
    main()
