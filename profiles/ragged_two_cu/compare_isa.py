"""Compare the gfx950 instruction text of the two meet-in-the-middle kernel files, parent build against this one.

    python profiles/ragged_two_cu/compare_isa.py PARENT_DIR THIS_DIR > profiles/ragged_two_cu/kernel_isa.txt

Each directory holds den_tied_mitm.s and den_tied_planes.s, made with the Makefile's flags plus ``--cuda-device-only -S``.
The reading of an assembly file is profiles/ragged/compare_isa.py's (``kernels``: a kernel's text is its instructions,
labels, directives and comments dropped).  A kernel is named by its demangled name with the template arguments padded to this
build's count: ``RAGGED`` = false is the new last argument of ``den_tied_mitm_kernel`` (7) and of
``den_tied_planes_mitm_kernel`` (4, behind a defaulted ``SPLIT``); ``den_tied_planes_kernel`` keeps its five.
Exit status 0: every kernel of the parent is in this build with identical instructions.
"""
import importlib.util
import os
import re
import sys

_spec = importlib.util.spec_from_file_location(
    "ragged_compare_isa", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ragged", "compare_isa.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

FILES = ("den_tied_mitm.s", "den_tied_planes.s")
ARGS = {"den_tied_mitm_kernel": 7, "den_tied_planes_kernel": 5, "den_tied_planes_mitm_kernel": 4}
NEW = ("den_tied_mitm_kernel", "den_tied_planes_mitm_kernel")  # the kernels whose RAGGED instantiation is this commit's


def canonical(pretty):
    m = re.match(r"void tc::(?:\(anonymous namespace\)::)?(\w+)<(.*)>\(", pretty)
    name, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    args += ["false"] * (ARGS[name] - len(args))
    return "%s<%s>" % (name, ", ".join(args)), name in NEW and args[-1] == "true"


def load(d):
    out = {}
    for f in FILES:
        ks = base.kernels("%s/%s" % (d, f))
        pretty = base.demangle(list(ks))
        for mangled, (ins, stats) in ks.items():
            key, ragged = canonical(pretty[mangled])
            out[key] = (ins, stats, ragged)
    return out


def main():
    parent, this = load(sys.argv[1]), load(sys.argv[2])
    same = [k for k in sorted(parent) if k in this and parent[k][0] == this[k][0]]
    print("%d of %d kernels of the parent identical in this build (instruction text, uniform instantiations)" % (len(same), len(parent)))
    for k in sorted(parent):
        state = "identical" if k in same else ("MISSING" if k not in this else "DIFFERS")
        st = this.get(k, parent[k])[1]
        print("  %-9s %6d instructions  vgpr %3d  sgpr %3d  %s" % (state, len(parent[k][0]), st["vgpr"], st["sgpr"], k))
    print()
    print("RAGGED two-workgroup instantiations of this build against their uniform twins: instructions (uniform -> ragged), VGPRs, "
          "SGPRs, spills (SGPR / VGPR; the twin's in brackets), scratch bytes")
    for k in sorted(this):
        ins, st, ragged = this[k]
        if not ragged:
            continue
        twin = this[re.sub(r"true>$", "false>", k)]
        print("  %6d -> %6d  vgpr %3d -> %3d  sgpr %3d -> %3d  spill %d / %d (%d / %d)  scratch %d -> %d  %s" %
              (len(twin[0]), len(ins), twin[1]["vgpr"], st["vgpr"], twin[1]["sgpr"], st["sgpr"], st["sgpr_spill"], st["vgpr_spill"],
               twin[1]["sgpr_spill"], twin[1]["vgpr_spill"], twin[1]["scratch"], st["scratch"], k))
    return 0 if len(same) == len(parent) else 1


if __name__ == "__main__":
    sys.exit(main())
