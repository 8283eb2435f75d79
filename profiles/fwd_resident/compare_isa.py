"""Compare the gfx950 instruction text of the tied kernels of two builds, kernel by kernel, and read the waits of the full-layout
twin's forward walk.

    python profiles/fwd_resident/compare_isa.py PARENT_DIR THIS_DIR > profiles/fwd_resident/kernel_isa.txt

Each directory holds den_tied_kernel.s, den_tied_mitm.s, den_tied_split.s, den_tied_planes.s, den_tied_pair.s and
den_general_owner.s, made with the Makefile's flags plus ``--cuda-device-only -S``.  A kernel's text is its instructions, as
profiles/last_pass/compare_isa.py takes them.  Every kernel of the parent must have the same text in this build except the two
full-layout twins (``den_tied_kernel<2, 1, true, ACCUM, true, RESF, 4, false, true>``), whose RESF goes from 4 to 6; the twins
must have no spilled VGPR, no scratch and no static LDS.  The exit status says whether all of that holds.

The forward walk of a den_tied_kernel instantiation: the kernel's text holds the forward frame loop, the backward frame loop and
the peeled backward frame 0, each with one ``s_setprio 0`` behind its walk and the ``s_setprio 1 / 2 / 3`` of the wave
generations in front of it (the first in line, the other two out of line behind the loop); the forward walk runs from the first
``s_setprio 1 / 2 / 3`` of the text to the first ``s_setprio 0``.  Its buffer loads, chunks (eight gathers) and ``s_waitcnt``
with a vmcnt field are listed in the order of the text: a wait that follows a streamed chunk's look-ahead loads must be counted
(vmcnt(3): the three loads just issued stay in flight), not vmcnt(0).
"""
import os
import re
import subprocess
import sys

import importlib.util


def sibling(directory):
    """profiles/<directory>/compare_isa.py as a module of its own name (the three scripts share a file name)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", directory, "compare_isa.py")
    spec = importlib.util.spec_from_file_location("compare_isa_" + directory, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


kernels = sibling("last_pass").kernels
FILES = ("den_tied_kernel.s", "den_tied_mitm.s", "den_tied_split.s", "den_tied_planes.s", "den_tied_pair.s", "den_general_owner.s")


def canonical(pretty):
    """a kernel's demangled name without namespaces and argument list; den_tied_kernel with all nine template arguments"""
    name = re.sub(r"^void ", "", pretty).replace("tc::(anonymous namespace)::", "").replace("tc::", "")
    name = re.sub(r"\((DenParams|tc::DenParams).*$", "", name)
    m = re.match(r"den_tied_kernel<(.*)>$", name)
    if m:
        args = [a.strip() for a in m.group(1).split(",")]
        args += ["false"] * (9 - len(args))  # RAGGED, FULL
        name = "den_tied_kernel<%s>" % ", ".join(args)
    return name


def load(d):
    """{(file, kernel name): (instruction lines, registers and spills)} of a directory"""
    ks = {}
    for f in FILES:
        for name, v in kernels("%s/%s" % (d, f)).items():
            ks[(f, name)] = v
    pretty = subprocess.run(["c++filt"], input="\n".join(n for _, n in ks), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    return {(f, canonical(p)): ks[(f, n)] for (f, n), p in zip(ks, pretty)}


TWIN = re.compile(r"den_tied_kernel<2, 1, true, (false|true), true, (\d+), 4, false, true>$")


def static_lds(d):
    """{(file, kernel name as load() spells it): bytes of static LDS} over the directory's files"""
    found = {}
    for f in FILES:
        try:
            text = open("%s/%s" % (d, f)).read()
        except FileNotFoundError:
            continue
        for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
            found[(f, m.group(1))] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
    pretty = subprocess.run(["c++filt"], input="\n".join(n for _, n in found), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    return {(f, canonical(p)): found[(f, n)] for (f, n), p in zip(found, pretty)}


def forward_walk(ins):
    """instruction lines of the forward walk (module docstring)"""
    start = next(i for i, line in enumerate(ins) if re.match(r"s_setprio [123]$", line))
    return ins[start + 1:ins.index("s_setprio 0")]


def walk_events(ins):
    """the forward walk as a line of events in the order of the text: ``load x N`` (buffer loads), ``chunk`` (the eight gathers of
    one chunk), and every s_waitcnt that has a vmcnt field"""
    out, loads, reads = [], 0, 0

    def flush():
        nonlocal loads
        if loads:
            out.append("load x %d" % loads)
            loads = 0

    for line in forward_walk(ins):
        if line.startswith("buffer_load"):
            loads += 1
        elif line.startswith("ds_read_b32"):
            flush()
            reads += 1
            if reads == 8:
                out.append("chunk")
                reads = 0
        elif line.startswith("s_waitcnt") and "vmcnt" in line:
            flush()
            out.append("[%s]" % line[len("s_waitcnt "):])
    flush()
    return out


def streamed_waits(events):
    """the waits in front of streamed chunks: every wait behind the first ``load`` of the walk"""
    first = next((i for i, e in enumerate(events) if e.startswith("load")), len(events))
    return [e for e in events[first:] if e.startswith("[")]


def main():
    parent, this = load(sys.argv[1]), load(sys.argv[2])
    same = [k for k in sorted(parent) if k in this and parent[k][0] == this[k][0]]
    moved = [k for k in sorted(parent) if k not in same]
    print("%d of %d kernels of the parent have the same instruction text in this build" % (len(same), len(parent)))
    for f in FILES:
        ks = [k for k in sorted(parent) if k[0] == f]
        bad = [k for k in ks if k not in same]
        print("  %-22s %3d kernels, %d differ%s" % (f, len(ks), len(bad), "".join("\n      " + k[1] for k in bad)))
    only_twins = all(k[0] == "den_tied_kernel.s" and TWIN.match(k[1]) for k in moved) and len(moved) == 2
    added = [k for k in sorted(this) if k not in parent]
    print("kernels of this build that the parent does not have:%s" % "".join("\n      " + k[1] for k in added))
    only_twins = only_twins and len(added) == 2 and all(TWIN.match(k[1]) for k in added)
    print("the kernels that differ are the two full-layout twins and nothing else: %s" % ("yes" if only_twins else "NO"))
    print()

    clean = True
    print("the full-layout twins: instructions, VGPRs, spills (SGPR / VGPR), scratch bytes, static LDS bytes")
    for label, table, d in (("parent", parent, sys.argv[1]), ("this", this, sys.argv[2])):
        lds = static_lds(d)
        for k in sorted(table):
            if k[0] != "den_tied_kernel.s" or not TWIN.match(k[1]):
                continue
            ins, st = table[k]
            print("  %-6s %5d instructions  vgpr %3d  spill %d / %d  scratch %d  static LDS %d  %s" % (
                label, len(ins), st["vgpr"], st["sgpr_spill"], st["vgpr_spill"], st["scratch"], lds[k], k[1]))
            if label == "this" and (st["vgpr_spill"] or st["scratch"] or lds[k]):
                clean = False
        if label == "this" and any(lds.values()):
            print("  kernels of this build with static LDS: %d" % sum(1 for v in lds.values() if v))
            clean = False
    print()
    print("the forward walk in the order of the text (first s_setprio 1 / 2 / 3 -> first s_setprio 0): resident chunks, the loop's two")
    print("chunks, the single peeled chunk, the peeled pair.  The waits in front of the resident chunks bind in frame 1 only (the")
    print("prologue's loads); the single peeled chunk and the pair's second chunk have no load behind them to count.  ``load x 1``")
    print("between the loop and the single chunk is the frame's row of y on the out-of-line entry of wave generations 1 and 2.")
    counted = True
    for label, table in (("parent", parent), ("this", this)):
        for k in sorted(table):
            if k[0] == "den_tied_kernel.s" and TWIN.match(k[1]):
                ev = walk_events(table[k][0])
                print("  %-6s %s" % (label, k[1]))
                print("         " + " ".join(ev))
                print("         waits of the streamed part: " + " ".join(streamed_waits(ev)))
                # behind a chunk's three look-ahead loads a wait must leave them in flight (``load x 1``: the frame's row of y, on the
                # out-of-line path of the wave generations 1 and 2)
                for i, e in enumerate(ev):
                    if e == "load x 3" and i + 1 < len(ev) and ev[i + 1].startswith("[") and "vmcnt(0)" in ev[i + 1] and label == "this":
                        counted = False
    print("every wait of this build's twins that follows a chunk's look-ahead loads is counted: %s" % ("yes" if counted else "NO"))
    ok = len(same) + 2 == len(parent) and only_twins and clean and counted
    print()
    print("verdict: %s" % ("ok" if ok else "FAILED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
