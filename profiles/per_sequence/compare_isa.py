"""Compare the gfx950 instruction text of every kernel of the library, parent build against this one.

    python profiles/per_sequence/compare_isa.py PARENT_DIR THIS_DIR > profiles/per_sequence/kernel_isa.txt

Each directory holds one assembly file ``<stem>.s`` per ``csrc/<stem>.hip``, made with the Makefile's flags plus
``--cuda-device-only -S`` (or the device half of ``-save-temps``, renamed).  The reading of an assembly file is
profiles/ragged/compare_isa.py's (``kernels``: a kernel's text is its instructions, labels, directives and comments dropped).
No kernel of the parent changed its signature in this commit, so kernels meet under their mangled names; the kernels this
commit adds are listed behind.
Exit status 0: every kernel of the parent is in this build with identical instructions.
"""
import importlib.util
import os
import sys

_spec = importlib.util.spec_from_file_location(
    "ragged_compare_isa", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ragged", "compare_isa.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

STEMS = ("den_kernels", "den_general_owner", "den_tied_kernel", "den_tied_planes", "den_tied_split", "den_tied_pair",
         "den_tied_mitm", "den_slab_kernel", "num_kernels", "num_windowed_kernels", "num_e2e_kernels", "num_best_path_kernels",
         "layout_kernels", "layout_rows_kernels")


def short(pretty):
    return pretty.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]


def load(d):
    out = {}
    for stem in STEMS:
        for mangled, (ins, stats) in base.kernels(os.path.join(d, stem + ".s")).items():
            out[(stem, mangled)] = (ins, stats)
    return out


def main():
    parent, this = load(sys.argv[1]), load(sys.argv[2])
    pretty = base.demangle(sorted({k[1] for k in list(parent) + list(this)}))
    same = [k for k in sorted(parent) if k in this and parent[k][0] == this[k][0]]
    print("%d of %d kernels of the parent identical in this build (instruction text)" % (len(same), len(parent)))
    for stem in STEMS:
        keys = [k for k in sorted(parent) if k[0] == stem]
        bad = [k for k in keys if k not in same]
        print("  %-22s %3d kernels, %3d identical, %6d instructions in all" % (stem, len(keys), len(keys) - len(bad),
                                                                             sum(len(parent[k][0]) for k in keys)))
        for k in bad:
            print("    %s %s" % ("MISSING" if k not in this else "DIFFERS", pretty[k[1]]))
    print()
    for name in ("finalize_kernel", "zero_on_fail_kernel", "zero_padding_kernel"):
        for k in sorted(parent):
            if ("tc::" + name) in pretty[k[1]] or ("::" + name + "<") in pretty[k[1]]:
                st = this[k][1]
                print("  %-9s %6d instructions  vgpr %3d  sgpr %3d  %s" % ("identical" if k in same else "DIFFERS", len(parent[k][0]),
                                                                          st["vgpr"], st["sgpr"], short(pretty[k[1]])))
    print()
    print("kernels this build adds:")
    for k in sorted(this):
        if k not in parent:
            ins, st = this[k]
            print("  %6d instructions  vgpr %3d  sgpr %3d  spill %d / %d  scratch %d  %s" % (
                len(ins), st["vgpr"], st["sgpr"], st["sgpr_spill"], st["vgpr_spill"], st["scratch"], short(pretty[k[1]])))
    return 0 if len(same) == len(parent) else 1


if __name__ == "__main__":
    sys.exit(main())
