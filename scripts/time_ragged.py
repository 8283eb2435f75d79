"""What ragged (unequal sequence lengths) end-to-end minibatches cost and buy, on C3's and C2's denominator graphs.

Two kinds of child process take turns, ``--rounds`` of each: ``parent`` (another checkout of this repository, ``--parent-root``,
built there) and ``this``.  Two builds of the library cannot share a process, hence the children; the process that starts
them never opens the GPU.  Every case is ``--warmup`` untimed and ``--iters`` event-timed calls; the report gives per case and
kind the median over the rounds of each round's median and the spread (max - min) of the rounds' medians -- the spread of a
kind is its run-to-run noise.

    den_c3_uniform / den_c2_uniform          tc_den_forward_backward, 256 x 150 / 64 x 150 (both kinds; SHA-1 of the derivative)
    den_c3_ragged_equal / den_c2_ragged_equal tc_den_forward_backward_ragged, all lengths 150 (this): what the route costs at
                                             C3 (the fused kernel and one scalar load), what it loses at C2 (the uniform call
                                             takes the meet-in-the-middle form there)
    step_c3_regular                          chain_loss + backward, C3's regular supervision, (B, C, T) (both; SHA-1 of the gradient)
    step_ragged_256                          chain_loss + backward on ONE ragged end-to-end minibatch: 256 sequences of eight
                                             lengths between 75 and 150, 32 of each (this)
    step_8x32_uniform                        the same sequences as EIGHT uniform steps of 32 (both): the only correct way before
    step_padded_256x150                      the uniform step on the padded (256, C, 150) tensor (both): a wrong objective, but
                                             the time a user pays who pads

    python scripts/time_ragged.py [--parent-root DIR] [--rounds 3] [--iters 20] [--warmup 5]

``--suite two_cu``: ragged batches of 8 sequences up to half the chip on two workgroups per sequence (DESIGN.md 4.12,
profiles/ragged_two_cu/README.md); every case in both kinds unless it says otherwise.

    den_c2_uniform / den_c3_uniform / den_r4_64_uniform   tc_den_forward_backward, 64 x 150 / 256 x 150 / R4's graph at 64 x 150
                                             (SHA-1 of the derivative): the uniform calls do not move
    den_c2_ragged_equal                      C2's batch as a ragged call, all lengths 150 (SHA-1): what the route costs against
                                             den_c2_uniform of the same process; the parent's is the fused kernel
    den_<g>_ragged_<S> / step_<g>_ragged_<S> the denominator alone / chain_loss + backward on S sequences of the eight lengths
                                             below, S / 8 of each: C2's graph at 64 and 128, R4's at 64 (parent: one workgroup a
                                             sequence)
    den_c2_ragged_<S>_two_cu / _one_wg       this only, S = 8, 16, 32: the two-workgroup route against ``no_phase_split``
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (150, 139, 129, 118, 107, 97, 86, 75)  # eight distinct lengths, 32 sequences of each, longest first


def phones_fst(num_pdfs, rng, phones=20):
    """A left-to-right end-to-end FST: ``phones`` states, each entered by an arc of its forward pdf and kept by a self-loop
    of its self-loop pdf; the last one final.  Feasible for every length >= phones."""
    n = phones + 1
    arc_begin, ilabel, cost, nxt = [0], [], [], []
    for i in range(n):
        if i > 0:  # self-loop
            ilabel.append(int(rng.integers(1, num_pdfs + 1)))
            cost.append(float(rng.uniform(0, 1)))
            nxt.append(i)
        if i + 1 < n:
            ilabel.append(int(rng.integers(1, num_pdfs + 1)))
            cost.append(float(rng.uniform(0, 1)))
            nxt.append(i + 1)
        arc_begin.append(len(ilabel))
    final = np.full(n, np.inf, np.float32)
    final[-1] = 0.0
    return (0, np.asarray(arc_begin, np.int32), np.asarray(ilabel, np.int32), np.asarray(cost, np.float32),
            np.asarray(nxt, np.int32), final)


def child(args):
    sys.path.insert(0, args.root)
    import torch

    from torchain_amd import io, synth
    from torchain_amd._lib import check, lib
    from torchain_amd.functions import chain_loss

    dev = "cuda:0"
    this = args.kind == "this"

    def timed(name, step, digest=None, extra=None):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        times.sort()
        row = dict(kind=args.kind, case=name, iters=args.iters, median_ms=round(times[len(times) // 2], 4), min_ms=round(times[0], 4))
        if digest is not None and args.hash:
            row["sha1"] = hashlib.sha1(digest().contiguous().view(torch.int32).cpu().numpy().tobytes()).hexdigest()
        if extra:
            row.update(extra())
        print(json.dumps(row), flush=True)

    if args.suite == "two_cu":
        return two_cu_cases(args, timed)

    for config in ("C3", "C2"):
        cfg = synth.CONFIGS[config]
        S, T, P = cfg["S"], cfg["T"], cfg["P"]
        graph = io.DenominatorGraph(synth.config_den_fst(config), P).prepare(dev)
        gen = torch.Generator(device=dev).manual_seed(4)
        y = torch.randn(S * T, P, device=dev, generator=gen)
        deriv = torch.empty_like(y)
        nbytes = lib.tc_chain_workspace_bytes(graph.ptr, S, T)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        lp = torch.zeros(1, dtype=torch.float64, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        frames = torch.full((S,), T, dtype=torch.int32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (graph.ptr, S, C.c_void_p(y.data_ptr()), S * T, P, P, cfg["leaky"], -1.0, cfg["l2"], 0, C.c_void_p(deriv.data_ptr()), P)
        tail = (C.c_void_p(lp.data_ptr()), C.c_void_p(st.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, 0, stream)
        timed("den_%s_uniform" % config.lower(), lambda: check(lib.tc_den_forward_backward(*head, *tail), "den"), lambda: deriv)
        if this:
            timed("den_%s_ragged_equal" % config.lower(),
                  lambda: check(lib.tc_den_forward_backward_ragged(*head, C.c_void_p(frames.data_ptr()), T, *tail), "den ragged"),
                  lambda: deriv)
        if config == "C2":
            continue
        kw = dict(l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"])

        def stepper(x, sup):
            def step():
                x.grad = None
                loss, _ = chain_loss(x, graph, sup, **kw)
                loss.backward()
            return step

        x = y.view(T, S, P).permute(1, 2, 0).contiguous().requires_grad_(True)
        rsup = io.Supervision.from_synth(synth.random_supervision(synth.config_den_fst(config), S, T, 3, seed=3))
        timed("step_c3_regular", stepper(x, rsup), lambda: x.grad)
        rng = np.random.default_rng(11)
        fsts = [phones_fst(P, rng) for _ in range(S)]
        per = S // len(LENGTHS)
        lens = [t for t in LENGTHS for _ in range(per)]
        timed("step_padded_256x150", stepper(x, io.Supervision.from_e2e_fsts(1.0, T, P, fsts)))
        parts = []
        for k, t in enumerate(LENGTHS):
            xs = x.detach()[k * per:(k + 1) * per, :, :t].contiguous().requires_grad_(True)
            parts.append(stepper(xs, io.Supervision.from_e2e_fsts(1.0, t, P, fsts[k * per:(k + 1) * per])))
        timed("step_8x32_uniform", lambda: [p() for p in parts])
        if this:
            timed("step_ragged_256", stepper(x, io.Supervision.from_e2e_fsts(1.0, lens, P, fsts)))
        del x, parts


def two_cu_cases(args, timed):
    """The cases of ``--suite two_cu`` (module docstring), in one child process."""
    import torch

    from torchain_amd import io, synth
    from torchain_amd._lib import check, lib
    from torchain_amd.functions import chain_loss

    dev = "cuda:0"
    this = args.kind == "this"
    T = 150
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def den_call(graph, cfg, S, P, lens=None):
        """(step, derivative) of tc_den_forward_backward on S x T, or -- lens given -- of the ragged entry"""
        gen = torch.Generator(device=dev).manual_seed(4)
        y = torch.randn(S * T, P, device=dev, generator=gen)
        deriv = torch.empty_like(y)
        nbytes = lib.tc_chain_workspace_bytes(graph.ptr, S, T)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        lp = torch.zeros(1, dtype=torch.float64, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        head = (graph.ptr, S, C.c_void_p(y.data_ptr()), S * T, P, P, cfg["leaky"], -1.0, cfg["l2"], 0, C.c_void_p(deriv.data_ptr()), P)
        tail = (C.c_void_p(lp.data_ptr()), C.c_void_p(st.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, 0, stream)
        keep = (y, ws, lp, st)
        if lens is None:
            return (lambda: check(lib.tc_den_forward_backward(*head, *tail), "den")), deriv, keep
        frames = torch.tensor(list(lens), dtype=torch.int32, device=dev)
        return (lambda: check(lib.tc_den_forward_backward_ragged(*head, C.c_void_p(frames.data_ptr()), T, *tail), "den ragged")), deriv, (keep, frames)

    def two_cu_count():
        n = int(lib.tc_debug_counter(b"ragged_two_cu_launches"))
        return {} if n < 0 else {"ragged_two_cu_launches": n}

    def step_call(graph, cfg, S, P, lens, seed):
        rng = np.random.default_rng(seed)
        sup = io.Supervision.from_e2e_fsts(1.0, list(lens), P, [phones_fst(P, rng) for _ in range(S)])
        gen = torch.Generator(device=dev).manual_seed(5)
        x = torch.randn(S, P, T, device=dev, generator=gen).requires_grad_(True)

        def step():
            x.grad = None
            loss, _ = chain_loss(x, graph, sup, l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"])
            loss.backward()
        return step, x

    def eight_lengths(S):
        return [t for t in LENGTHS for _ in range(S // len(LENGTHS))]

    for config, sizes in (("C2", (64, 128)), ("C3", ()), ("R4", (64,))):
        cfg = synth.CONFIGS[config]
        P = cfg["P"]
        graph = io.DenominatorGraph(synth.config_den_fst(config), P).prepare(dev)
        S = 64 if config == "R4" else cfg["S"]
        name = "den_%s_uniform" % ("r4_64" if config == "R4" else config.lower())
        step, deriv, keep = den_call(graph, cfg, S, P)
        timed(name, step, lambda: deriv)
        if config == "C2":
            step, deriv, keep = den_call(graph, cfg, S, P, [T] * S)
            timed("den_c2_ragged_equal", step, lambda: deriv, two_cu_count)
        for S in sizes:
            step, deriv, keep = den_call(graph, cfg, S, P, eight_lengths(S))
            timed("den_%s_ragged_%d" % (config.lower(), S), step, None, two_cu_count)
            step, x = step_call(graph, cfg, S, P, eight_lengths(S), seed=11)
            timed("step_%s_ragged_%d" % (config.lower(), S), step, None, two_cu_count)
            del x
        if config == "C2" and this:
            for S in (8, 16, 32):
                step, deriv, keep = den_call(graph, cfg, S, P, eight_lengths(S))
                timed("den_c2_ragged_%d_two_cu" % S, step, None, two_cu_count)
                check(lib.tc_debug_set(b"no_phase_split", 1), "no_phase_split")
                timed("den_c2_ragged_%d_one_wg" % S, step, None, two_cu_count)
                check(lib.tc_debug_set(b"no_phase_split", 0), "no_phase_split")
        del graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit to compare with (kind 'parent')")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--suite", default="ragged", choices=("ragged", "two_cu"), help="which set of cases (module docstring)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kind", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--hash", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.join(HERE, ".."), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    roots = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", os.path.abspath(args.root))]
    rows, hashes = {}, {}
    for rnd in range(args.rounds):
        for kind, root in roots:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--kind", kind, "--root", root, "--iters", str(args.iters),
                   "--warmup", str(args.warmup), "--suite", args.suite] + (["--hash"] if rnd == 0 else [])
            # (a child that fails or hangs ends the run: nothing more is started on the GPU behind it)
            out = subprocess.run(cmd, check=True, timeout=args.timeout, stdout=subprocess.PIPE, text=True, cwd=root).stdout
            for line in out.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    r["round"] = rnd
                    print(json.dumps(r), flush=True)
                    rows.setdefault((r["case"], kind), []).append(r["median_ms"])
                    if "sha1" in r:
                        hashes[(r["case"], kind)] = r["sha1"]
    print("# case kind: median over %d rounds of the rounds' medians (ms), spread max - min, the rounds" % args.rounds)
    for key, v in sorted(rows.items()):
        s = sorted(v)
        print("# %-22s %-6s %.3f  spread %.3f  %s" % (key[0], key[1], s[len(s) // 2], s[-1] - s[0], " ".join("%.3f" % x for x in v)))
    print("# SHA-1 of the outputs (derivative of the denominator call, gradient of the step):")
    for (case, kind), h in sorted(hashes.items()):
        if kind == "this" and (case, "parent") in hashes:
            print("# %-22s this == parent: %s" % (case, "identical" if h == hashes[(case, "parent")] else "DIFFERENT"))
    for config in ("c3", "c2"):
        a, b = hashes.get(("den_%s_uniform" % config, "this")), hashes.get(("den_%s_ragged_equal" % config, "this"))
        if a and b:
            print("# den_%s ragged (all lengths equal) == uniform, this build: %s" % (config, "identical" if a == b else "different"))
    if args.suite == "two_cu" and ("den_c2_uniform", "this") in rows:
        # what the route costs: per round, the ragged call with all lengths equal minus the uniform call of the same process,
        # against the spread of the uniform call's rounds
        u, r = rows[("den_c2_uniform", "this")], rows.get(("den_c2_ragged_equal", "this"), [])
        diffs = [b - a for a, b in zip(u, r)]
        if diffs:
            print("# den_c2 ragged_equal - uniform, this build, per round: %s  (spread of the uniform call %.3f)" %
                  (" ".join("%+.3f" % d for d in diffs), max(u) - min(u)))


if __name__ == "__main__":
    main()
