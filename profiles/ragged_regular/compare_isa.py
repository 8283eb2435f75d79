"""Compare the gfx950 instruction text of the two regular numerator kernel files, parent build against this one.

    python profiles/ragged_regular/compare_isa.py PARENT_DIR THIS_DIR > profiles/ragged_regular/kernel_isa.txt

Each directory holds num_kernels.s and num_windowed_kernels.s, made with the Makefile's flags plus ``--cuda-device-only -S``.
The reading of an assembly file is profiles/ragged/compare_isa.py's (``kernels``: a kernel's text is its instructions,
labels, directives and comments dropped).  A kernel is named by its demangled name with the template arguments padded to this
build's count: ``RAGGED`` = false is the new last argument of ``num_fwd_bwd_kernel`` (3) and of ``num_windowed_kernel`` (2);
``num_scatter_kernel`` keeps its one, and the kernels of num_kernels.hip that are no templates (the scalar epilogue and its
kin) are compared under their plain names.
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

FILES = ("num_kernels.s", "num_windowed_kernels.s")
ARGS = {"num_fwd_bwd_kernel": 3, "num_windowed_kernel": 2, "num_scatter_kernel": 1}
NEW = ("num_fwd_bwd_kernel", "num_windowed_kernel")  # the kernels whose RAGGED instantiation is this commit's


def canonical(pretty):
    m = re.match(r"void tc::(?:\(anonymous namespace\)::)?(\w+)<(.*)>\(", pretty)
    if not m:  # not a template
        return re.match(r"(?:void )?tc::(?:\(anonymous namespace\)::)?(\w+)\(", pretty).group(1), False
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
    print("RAGGED instantiations of this build against their uniform twins: instructions (uniform -> ragged), VGPRs, SGPRs, "
          "spills (SGPR / VGPR; the twin's in brackets), scratch bytes, vector compares (v_cmp*)")
    for k in sorted(this):
        ins, st, ragged = this[k]
        if not ragged:
            continue
        twin = this[re.sub(r"true>$", "false>", k)]
        vcmp = lambda lines: sum(1 for line in lines if line.startswith("v_cmp"))  # noqa: E731
        print("  %6d -> %6d  vgpr %3d -> %3d  sgpr %3d -> %3d  spill %d / %d (%d / %d)  scratch %d  v_cmp %d -> %d  %s" %
              (len(twin[0]), len(ins), twin[1]["vgpr"], st["vgpr"], twin[1]["sgpr"], st["sgpr"], st["sgpr_spill"], st["vgpr_spill"],
               twin[1]["sgpr_spill"], twin[1]["vgpr_spill"], st["scratch"], vcmp(twin[0]), vcmp(ins), k))
    return 0 if len(same) == len(parent) else 1


if __name__ == "__main__":
    sys.exit(main())
