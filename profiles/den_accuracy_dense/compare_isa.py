"""Compare the gfx950 instruction text of the expected-accuracy kernels of two builds, kernel by kernel.

    python profiles/den_accuracy_dense/compare_isa.py PARENT_DIR THIS_DIR > profiles/den_accuracy_dense/kernel_isa.txt

Each directory holds den_accuracy_kernels.s, made with the Makefile's flags plus ``--cuda-device-only -S``.  A kernel's text is
its instructions, as profiles/last_pass/compare_isa.py takes them, to the kernel's end.  Every kernel of the parent -- the hard-reference form --
must have the same text in this build, where it is the DENSE = false instantiation: ``den_accuracy_rows_kernel`` of the parent
meets ``den_accuracy_rows_kernel<false>``, ``den_accuracy_grad_kernel<R, L>`` meets ``<R, L, false>``.  No gradient kernel may
have static LDS and the row kernels keep the parent's 64 bytes; the exit status says whether all of that holds.
"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "last_pass"))
from compare_isa import kernels as to_first_endpgm  # noqa: E402

FILE = "den_accuracy_kernels.s"


def canonical(pretty):
    name = re.sub(r"^void ", "", pretty).replace("tc::", "")
    name = re.sub(r"\((DenAcc\w+Params)( const)?\)$", "", name)
    m = re.match(r"(den_accuracy_\w+_kernel)(?:<(.*)>)?$", name)
    args = [a.strip() for a in m.group(2).split(",")] if m.group(2) else []
    args += ["false"] * ({"den_accuracy_rows_kernel": 1, "den_accuracy_grad_kernel": 3}[m.group(1)] - len(args))  # DENSE
    return "%s<%s>" % (m.group(1), ", ".join(args))


def kernels(path):
    """as profiles/last_pass/compare_isa.py's, with a kernel's WHOLE text: the gradient kernel leaves early for a sequence that
    is not finite, so its first s_endpgm is not its end"""
    found = to_first_endpgm(path)
    text = open(path).read()
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\s*\.section", text, re.S | re.M):
        if m.group(1) not in found:
            continue
        ins = []
        for line in m.group(2).splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            ins.append(re.sub(r"\s+", " ", re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)))
        found[m.group(1)] = (ins, found[m.group(1)][1])
    return found


def load(d):
    path = "%s/%s" % (d, FILE)
    ks = kernels(path)
    pretty = subprocess.run(["c++filt"], input="\n".join(ks), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    text = open(path).read()
    lds = {}
    for m in re.finditer(r"\.amdhsa_kernel (\w+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        lds[m.group(1)] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2)).group(1))
    return {canonical(p): ks[n] + (lds[n],) for n, p in zip(ks, pretty)}


def main():
    parent, this = load(sys.argv[1]), load(sys.argv[2])
    same = [k for k in sorted(parent) if k in this and parent[k][0] == this[k][0]]
    print("%d of %d kernels of the parent have the same instruction text in this build" % (len(same), len(parent)))
    for k in sorted(parent):
        print("  %-9s %5d instructions  %s" % ("identical" if k in same else ("MISSING" if k not in this else "DIFFERS"),
                                               len(parent[k][0]), k))
    print()
    print("every kernel of this build: instructions, VGPRs, SGPRs, spills (SGPR / VGPR), scratch bytes, static LDS bytes")
    ok = len(same) == len(parent)
    for k in sorted(this):
        ins, st, lds = this[k]
        print("  %5d instructions  vgpr %3d  sgpr %3d  spill %d / %d  scratch %d  lds %d  %s" % (
            len(ins), st["vgpr"], st["sgpr"], st["sgpr_spill"], st["vgpr_spill"], st["scratch"], lds, k))
        ok = ok and lds == (64 if k.startswith("den_accuracy_rows_kernel") else 0) and st["scratch"] == 0
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
