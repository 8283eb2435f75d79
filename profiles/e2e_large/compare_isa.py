"""Compare the gfx950 instruction text of the end-to-end numerator kernels of two builds, function by function.

    python profiles/e2e_large/compare_isa.py PARENT_DIR THIS_DIR > profiles/e2e_large/kernel_isa.txt

Each directory holds num_e2e_kernels.s and num_best_path_kernels.s (and, for this build, num_e2e_large_kernels.s), made with
the Makefile's flags plus ``--cuda-device-only -S``.  A kernel's text is its instructions, as profiles/last_pass/compare_isa.py
takes them: labels, directives and comments are dropped.  The resident kernels (num_e2e_kernel, num_e2e_scatter_kernel) must
be the parent's: the exit status says whether they are.  The best path's kernels are listed too; its end-to-end kernel lays
its LDS out per sequence since this change, so its text differs.
"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "last_pass"))
from compare_isa import kernels  # noqa: E402

FILES = ("num_e2e_kernels.s", "num_best_path_kernels.s", "num_e2e_large_kernels.s")


def load(d):
    ks = {}
    for f in FILES:
        ks.update(kernels("%s/%s" % (d, f)))
    names = list(ks)
    pretty = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    return {p.split("(tc::NumParams")[0].replace("void ", ""): ks[n] for n, p in zip(names, pretty)}


def main():
    parent, this = load(sys.argv[1]), load(sys.argv[2])
    same = [k for k in sorted(parent) if k in this and parent[k][0] == this[k][0]]
    print("%d of %d kernels of the parent have the same instruction text in this build" % (len(same), len(parent)))
    for k in sorted(parent):
        print("  %-9s %5d instructions  %s" % ("identical" if k in same else ("MISSING" if k not in this else "DIFFERS"), len(parent[k][0]), k))
    print()
    print("kernels this build adds: instructions, VGPRs, SGPRs, spills (SGPR / VGPR), scratch bytes")
    for k in sorted(this):
        if k not in parent:
            ins, st = this[k]
            print("  %5d instructions  vgpr %3d  sgpr %3d  spill %d / %d  scratch %d  %s"
                  % (len(ins), st["vgpr"], st["sgpr"], st["sgpr_spill"], st["vgpr_spill"], st["scratch"], k))
    resident = [k for k in parent if k.startswith(("tc::num_e2e_kernel<", "tc::num_e2e_scatter_kernel<"))]
    print()
    print("resident end-to-end kernels (num_e2e_kernel, num_e2e_scatter_kernel): %d of %d identical" % (
        len([k for k in resident if k in same]), len(resident)))
    return 0 if resident and all(k in same for k in resident) else 1


if __name__ == "__main__":
    sys.exit(main())
