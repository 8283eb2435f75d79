"""Compare the gfx950 instruction text of the layout kernels of two builds, function by function.

    python profiles/last_pass/compare_isa.py PARENT_DIR THIS_DIR > profiles/last_pass/kernel_isa.txt

Each directory holds layout_kernels.s and layout_rows_kernels.s (and, for the parent, penalty_kernels.s), made with the
Makefile's flags plus ``--cuda-device-only -S``.  A kernel's text is its instructions: labels, directives and comments are
dropped, and a mangled name that occurs in an operand is replaced by its demangled form without the trailing template
defaults, so that ``layout_kernel<false, true, float, false>`` of the parent meets ``<false, true, float, false, false>``.
"""
import re
import subprocess
import sys

FILES = ("layout_kernels.s", "layout_rows_kernels.s", "penalty_kernels.s")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def kernels(path):
    """{mangled name: (instruction lines, {vgpr, sgpr, sgpr_spill, vgpr_spill, scratch})} of every kernel in an assembly file"""
    try:
        text = open(path).read()
    except FileNotFoundError:
        return {}
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
    # registers and spills: the code object's metadata, one entry per kernel
    for entry in text[text.find("amdhsa.kernels:"):].split("\n  - ")[1:]:
        f = dict(re.findall(r"^\s*\.(\w+):\s+(\S+)\s*$", entry, re.M))
        if f.get("name") in found:
            found[f["name"]][1].update(vgpr=int(f["vgpr_count"]), sgpr=int(f["sgpr_count"]), sgpr_spill=int(f["sgpr_spill_count"]),
                                       vgpr_spill=int(f["vgpr_spill_count"]), scratch=int(f["private_segment_fixed_size"]))
    return found


def canonical(pretty):
    """the kernel's name without the tc::(anonymous namespace):: prefix, the argument list and the penalty's false"""
    m = re.match(r"void tc::\(anonymous namespace\)::(\w+)<(.*?)>\(", pretty)
    name, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    args = [{"(tc::ScatterMode)0": "0", "(tc::ScatterMode)1": "1", "(tc::ScatterMode)2": "2"}.get(a, a) for a in args]
    full = {"layout_kernel": 5, "round_kernel": 4, "scale_rows_kernel": 3}
    defaults = {"layout_kernel": ["", "", "float", "false", "false"], "round_kernel": ["", "", "false", "false"],
                "scale_rows_kernel": ["", "true", "false"]}
    if name in full:
        args += defaults[name][len(args):]
    return "%s<%s>" % (name, ", ".join(args))


def load(d):
    ks = {}
    for f in FILES:
        ks.update(kernels("%s/%s" % (d, f)))
    pretty = demangle(list(ks))
    out = {}
    for mangled, (ins, stats) in ks.items():
        if "trace_" in mangled:
            continue
        ins = [re.sub(r"_Z\w+", lambda mm: canonical(pretty[mm.group(0)]) if mm.group(0) in pretty else mm.group(0), i) for i in ins]
        out[canonical(pretty[mangled])] = (ins, stats)
    return out


FMA = re.compile(r"v_(pk_)?(fma|fmac|fmamk|fmaak|mad|mac|madmk|madak)(_legacy)?_(f32|f16)(_e32|_e64|_dpp|_sdwa)?\b|v_fma_mix|v_dot")


def float_fmas(ins):
    """(all, outside a division): float FMAs of a kernel, and those of them that are not part of the reciprocal refinement
    of an integer division (the row index i / cols, r / B), which lies within a dozen instructions of its v_rcp"""
    at = [i for i, line in enumerate(ins) if FMA.match(line)]
    out = [i for i in at if not any(x.startswith("v_rcp_") for x in ins[max(0, i - 12):i + 12])]
    return len(at), len(out)


def main():
    parent, this = load(sys.argv[1]), load(sys.argv[2])
    plain = [k for k in sorted(parent) if "penalized" not in k and "penalize_rows" not in k]
    same = [k for k in plain if k in this and parent[k][0] == this[k][0]]
    print("%d of %d identical (kernels of the parent, instruction text, against this build's PEN = false instantiations)" % (len(same), len(plain)))
    for k in plain:
        print("  %-9s %5d instructions  %s" % ("identical" if k in same else ("MISSING" if k not in this else "DIFFERS"), len(parent[k][0]), k))
    print()
    print("penalised instantiations of this build: VGPRs, SGPRs, spills (SGPR / VGPR), scratch bytes, float FMAs (all / outside an integer division)")
    for k in sorted(this):
        if k in parent and k in plain:
            continue
        ins, st = this[k]
        print("  vgpr %3d  sgpr %3d  spill %d / %d  scratch %d  fma %d / %d  %s" % ((st["vgpr"], st["sgpr"], st["sgpr_spill"], st["vgpr_spill"], st["scratch"]) + float_fmas(ins) + (k,)))
    return 0 if len(same) == len(plain) else 1


if __name__ == "__main__":
    sys.exit(main())
