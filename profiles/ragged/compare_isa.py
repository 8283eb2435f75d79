"""Compare the gfx950 instruction text of the kernels that gained a RAGGED instantiation, parent build against this one.

    python profiles/ragged/compare_isa.py PARENT_DIR THIS_DIR > profiles/ragged/kernel_isa.txt

Each directory holds den_kernels.s, den_general_owner.s, den_tied_kernel.s, den_tied_planes.s and num_e2e_kernels.s, made with
the Makefile's flags plus ``--cuda-device-only -S``.  A kernel's text is its instructions: labels, directives and comments
are dropped (as profiles/last_pass/compare_isa.py does).  A kernel is named by its demangled name without the template
arguments this commit appended (``RAGGED`` = false is the last argument of the uniform instantiations), so that
``den_tied_kernel<2, 1, true, false, true, 4, 4>`` of the parent meets ``<2, 1, true, false, true, 4, 4, false>``.
Exit status 0: every kernel of the parent is in this build with identical instructions.
"""
import re
import subprocess
import sys

FILES = ("den_kernels.s", "den_general_owner.s", "den_tied_kernel.s", "den_tied_planes.s", "num_e2e_kernels.s")
# template arguments of each kernel in this build (the parent's lists are shorter by the trailing RAGGED, the plane-wise
# kernel's also by a defaulted SPLIT that the compiler prints)
ARGS = {"den_fwd_bwd_kernel": 6, "den_general_owner_kernel": 4, "den_tied_kernel": 8, "den_tied_planes_kernel": 5,
        "den_tied_planes_mitm_kernel": 3, "num_e2e_kernel": 2, "num_e2e_scatter_kernel": 2}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def kernels(path):
    """{mangled name: (instruction lines, stats)} of every kernel in an assembly file"""
    text = open(path).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        code = body.split("s_endpgm")[0]
        ins = []
        for line in code.splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)  # (a label carries its function's number in the file)
            ins.append(re.sub(r"\s+", " ", line))
        found[name] = (ins, {})
    for entry in text[text.find("amdhsa.kernels:"):].split("\n  - ")[1:]:
        f = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", entry, re.M))
        if f.get("name") in found:
            found[f["name"]][1].update(vgpr=int(f["vgpr_count"]), sgpr=int(f["sgpr_count"]), sgpr_spill=int(f["sgpr_spill_count"]),
                                       vgpr_spill=int(f["vgpr_spill_count"]), scratch=int(f["private_segment_fixed_size"]))
    return found


def canonical(pretty):
    """(kernel<arguments padded with false to this build's count>, is a RAGGED instantiation)"""
    m = re.match(r"void tc::(?:\(anonymous namespace\)::)?(\w+)<(.*)>\(", pretty)
    name, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    args += ["false"] * (ARGS[name] - len(args))
    ragged = name != "den_tied_planes_mitm_kernel" and args[-1] == "true"
    return "%s<%s>" % (name, ", ".join(args)), ragged


def load(d):
    out = {}
    for f in FILES:
        ks = kernels("%s/%s" % (d, f))
        pretty = demangle(list(ks))
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
          "spills (SGPR / VGPR), scratch bytes")
    for k in sorted(this):
        ins, st, ragged = this[k]
        if not ragged:
            continue
        twin = this[re.sub(r"true>$", "false>", k)]
        print("  %6d -> %6d  vgpr %3d -> %3d  sgpr %3d -> %3d  spill %d / %d  scratch %d  %s" %
              (len(twin[0]), len(ins), twin[1]["vgpr"], st["vgpr"], twin[1]["sgpr"], st["sgpr"], st["sgpr_spill"], st["vgpr_spill"],
               st["scratch"], k))
    return 0 if len(same) == len(parent) else 1


if __name__ == "__main__":
    sys.exit(main())
