"""Compare the gfx950 instruction text of the tied kernels of two builds, kernel by kernel, and count what the fused kernel's
backward per-state pass issues.

    python profiles/full_layout/compare_isa.py PARENT_DIR THIS_DIR > profiles/full_layout/kernel_isa.txt

Each directory holds den_tied_kernel.s, den_tied_mitm.s, den_tied_split.s, den_tied_planes.s, den_tied_pair.s and
den_general_owner.s, made with the Makefile's flags plus ``--cuda-device-only -S``.  A kernel's text is its instructions, as
profiles/last_pass/compare_isa.py takes them.  Every kernel of the parent must have the same text in this build (its
general instantiations: den_tied_kernel<...> of the parent meets <..., false> here) and no kernel may have static LDS; the
exit status says whether that holds.

The per-state stretch of a den_tied_kernel instantiation with a backward phase: the kernel's text holds the forward frame
loop, the backward frame loop and the peeled backward frame 0, each with one ``s_setprio 0`` behind its walk; the stretch runs
from the second of them (the backward loop's) to the next ``s_barrier`` (the reduction's), in the order of the text.
"""
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "last_pass"))
from compare_isa import kernels  # noqa: E402

FILES = ("den_tied_kernel.s", "den_tied_mitm.s", "den_tied_split.s", "den_tied_planes.s", "den_tied_pair.s", "den_general_owner.s")
HOT = "den_tied_kernel<2, 1, true, false, true, 4, 4, false, %s>"


def canonical(pretty):
    name = re.sub(r"^void ", "", pretty).replace("tc::(anonymous namespace)::", "").replace("tc::", "")
    name = re.sub(r"\((DenParams|tc::DenParams).*$", "", name)
    m = re.match(r"den_tied_kernel<(.*)>$", name)
    if m:
        args = [a.strip() for a in m.group(1).split(",")]
        args += ["false"] * (9 - len(args))  # RAGGED, FULL
        name = "den_tied_kernel<%s>" % ", ".join(args)
    return name


def load(d):
    ks = {}
    for f in FILES:
        for name, v in kernels("%s/%s" % (d, f)).items():
            ks[(f, name)] = v
    names = [n for _, n in ks]
    pretty = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    return {(f, canonical(p)): ks[(f, n)] for (f, n), p in zip(ks, pretty)}


def kind(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("buffer_", "global_", "scratch_")):
        return "VMEM"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    return "other"


def stretch(ins):
    """the backward loop's per-state pass: second ``s_setprio 0`` -> next ``s_barrier``"""
    at = [i for i, line in enumerate(ins) if line == "s_setprio 0"]
    if len(at) < 3:
        return None
    end = next(i for i in range(at[1], len(ins)) if ins[i].startswith("s_barrier"))
    c = collections.Counter()
    for line in ins[at[1] + 1:end]:
        op = line.split()[0]
        c[kind(op)] += 1
        if op.startswith("v_mov"):
            c["v_mov"] += 1
        if op.startswith("v_pk_"):
            c["v_pk"] += 1
        if op.startswith("v_readlane"):
            c["v_readlane"] += 1
    return c


def main():
    parent, this = load(sys.argv[1]), load(sys.argv[2])
    same = [k for k in sorted(parent) if k in this and parent[k][0] == this[k][0]]
    print("%d of %d kernels of the parent have the same instruction text in this build" % (len(same), len(parent)))
    for f in FILES:
        ks = [k for k in sorted(parent) if k[0] == f]
        bad = [k for k in ks if k not in same]
        print("  %-22s %3d kernels, %d differ%s" % (f, len(ks), len(bad), "".join("\n      " + k[1] for k in bad)))
    print()
    print("kernels this build adds: instructions, VGPRs, SGPRs, spills (SGPR / VGPR), scratch bytes, v_readlane in the whole text")
    for k in sorted(this):
        if k not in parent:
            ins, st = this[k]
            print("  %5d instructions  vgpr %3d  sgpr %3d  spill %d / %d  scratch %d  readlane %d  %s" % (
                len(ins), st["vgpr"], st["sgpr"], st["sgpr_spill"], st["vgpr_spill"], st["scratch"],
                sum(1 for i in ins if i.startswith("v_readlane")), k[1]))
    print()
    print("whole kernel, hot instantiation: VGPRs, spills (SGPR / VGPR), scratch bytes, v_readlane in the text")
    for label, table, name in (("parent", parent, HOT % "false"), ("general", this, HOT % "false"), ("FULL", this, HOT % "true")):
        ins, st = table[("den_tied_kernel.s", name)]
        print("  %-8s vgpr %d  spill %d / %d  scratch %d  v_readlane %d" % (
            label, st["vgpr"], st["sgpr_spill"], st["vgpr_spill"], st["scratch"], sum(1 for i in ins if i.startswith("v_readlane"))))
    print()
    print("backward per-state pass of the FULL twins (backward loop's s_setprio 0 -> the reduction's s_barrier), static counts")
    print("(the general form's stretch is not one run of text: its guarded blocks lie out of line)")
    for k in sorted(this):
        if k[0] == "den_tied_kernel.s" and k[1].endswith(", true>"):
            c = stretch(this[k][0])
            print("  VALU %3d (v_mov %d, packed %d, v_readlane %d)  LDS %d  VMEM %d  branches %d  %s" % (
                c["VALU"], c["v_mov"], c["v_pk"], c["v_readlane"], c["LDS"], c["VMEM"], c["branch"], k[1]))
    # the frames address LDS from byte 0: no kernel may have static LDS of its own (a private array the compiler moved there)
    static = 0
    for f in FILES:
        try:
            sizes = re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", open("%s/%s" % (sys.argv[2], f)).read())
        except FileNotFoundError:
            continue
        static += sum(1 for x in sizes if int(x) != 0)
    print()
    print("kernels of this build with static LDS: %d" % static)
    return 0 if len(same) == len(parent) and static == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
