"""Resource table of every kernel in hipcc -S listings, and a comparison of two sets of listings (before / after a refactor).

    hipcc <the build's flags> --cuda-device-only -S file.hip -o dir/file.s          (one listing per source, both trees)
    python tools/debug/kernel_resources.py before_dir after_dir

Per kernel: registers, spills, private segment, static LDS, kernel-argument layout (all from the code object's metadata) and the
instruction classes of isa_count.py plus barriers.  `same` = every figure equal; `stream` = the instruction streams are equal line
for line once labels and comments are dropped.  Exit status 1 if a kernel differs in a figure or exists on one side only.
"""
import collections
import glob
import os
import re
import sys

META = [("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("vspill", ".vgpr_spill_count"),
        ("sspill", ".sgpr_spill_count"), ("priv", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size"),
        ("kernarg", ".kernarg_segment_size"), ("wg", ".max_flat_workgroup_size")]
CLASSES = ["mfma", "ds", "vmem", "scratch", "barrier", "wait"]


def classify(op):
    if op.startswith(("v_mfma", "v_smfma")):
        return "mfma"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("s_barrier"):
        return "barrier"
    if op.startswith("s_waitcnt"):
        return "wait"
    return None


def kernels(path):
    """{kernel symbol: (figures dict, argument layout string, normalised instruction stream)}"""
    text = open(path).read()
    lines = text.split("\n")
    out = {}
    # the metadata: one yaml map per kernel under amdhsa.kernels, each starting with "  - .agpr_count:" or "  - .args:"
    meta = text[text.find("amdhsa.kernels:"):]
    for entry in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"\.symbol:\s+(\S+)\.kd", entry)
        if not m:
            continue
        fig = {}
        for key, field in META:
            v = re.search(r"%s:\s+(\d+)" % re.escape(field), entry)
            fig[key] = int(v.group(1)) if v else -1
        args = " ".join("%s@%s" % (s, o) for o, s in re.findall(r"\.offset:\s+(\d+)\s+\.size:\s+(\d+)", entry))
        out[m.group(1)] = [fig, args, None]
    for sym in out:
        start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith((".Lfunc_end", "\t.section")))
        body, cnt = [], collections.Counter()
        for l in lines[start + 1:end]:
            t = l.split(";")[0].strip()
            if not t or t.startswith("."):
                continue
            t = re.sub(r"\.LBB\d+_", ".LBB_", t)
            body.append(t)
            c = classify(t.split()[0])
            if c:
                cnt[c] += 1
        for c in CLASSES:
            out[sym][0][c] = cnt[c]
        out[sym][2] = body
    return out


def short(sym):
    m = re.match(r"_ZL?(\d+)", sym)
    if not m:
        return sym
    name, rest = sym[m.end():m.end() + int(m.group(1))], sym[m.end() + int(m.group(1)):]
    targs = re.findall(r"L[ib](\d+)E", rest.split("EvP")[0]) if rest.startswith("I") else []
    return name + ("<" + ",".join(targs) + ">" if targs else "")


def main():
    before, after = sys.argv[1], sys.argv[2]
    keys = [k for k, _ in META] + CLASSES
    bad = 0
    for pb in sorted(glob.glob(os.path.join(before, "*.s"))):
        pa = os.path.join(after, os.path.basename(pb))
        kb, ka = kernels(pb), kernels(pa)
        print("== " + os.path.basename(pb))
        print("%-28s %s  same stream args" % ("kernel", " ".join("%7s" % k for k in keys)))
        for sym in sorted(set(kb) | set(ka)):
            if sym not in kb or sym not in ka:
                print("%-28s only in %s" % (short(sym), "before" if sym in kb else "after"))
                bad += 1
                continue
            fb, fa = kb[sym][0], ka[sym][0]
            same = all(fb[k] == fa[k] for k in keys if k != "wait") and kb[sym][1] == ka[sym][1]
            bad += not same
            print("%-28s %s  %-4s %-6s %s" % (short(sym), " ".join("%7d" % fa[k] for k in keys), "yes" if same else "NO",
                                               "yes" if kb[sym][2] == ka[sym][2] else "no", "yes" if kb[sym][1] == ka[sym][1] else "NO"))
            if not same or fb["wait"] != fa["wait"]:
                print("%-28s %s  (before)" % ("", " ".join("%7d" % fb[k] for k in keys)))
    print("kernels that differ in a required figure: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
