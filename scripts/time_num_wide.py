"""What the wide-level numerator kernel (csrc/num_wide_kernels.hip) costs, and that nothing else moved.  Three parts, each a
child process; the process that starts them never opens the GPU.

  wide12k   this checkout: the numerator alone (``tc_num_forward_backward`` with a derivative) and the training step
            (``chain_loss`` + backward, (B, C, T) float32) on C3's denominator graph at C3's shape (256 x 150), on a batch every
            sequence of which has three levels of 12000 states (frames 25, 75 and 125; 2-11 states elsewhere) -- refused by
            every kernel before this one.  Four different sequences, each 64 times, through ``from_sequences(any_width=True)``.
            The LDS form, and the slot form forced (``tc_debug_set("force_num_wide_streamed", 1)``).
  forced    this checkout: the numerator alone on ``lattice_wide`` and ``lattice_bursty`` of tests/wide_supervisions.py, by the
            windowed kernel (``force_num_windowed``) and by the wide kernel (``force_num_wide``) on handles of the same FST in
            the same process, taking turns; their results compared byte for byte.
  step      the C3 training step on a resident handle (trie3) and a windowed one (trie64) of scripts/time_num_windowed.py, by
            this checkout and by another built checkout of the repository (``--parent-root``), ``--rounds`` children of each
            taking turns: the parent's spread over its rounds is the run-to-run noise the difference is read against.

Every figure is the median of ``--iters`` calls between two device events after ``--warmup`` calls.

    python scripts/time_num_wide.py [--parent-root DIR] [--rounds 3] [--iters 20] [--warmup 5] [--cache-dir DIR]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import time_num_windowed as tw  # noqa: E402  (the C3 supervisions and their cache)

STEP_CASES = ("trie3", "trie64")


def timed(torch, fns, iters, warmup):
    """{key: median ms} of the callables, taking turns."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: round(sorted(v)[len(v) // 2], 4) for k, v in times.items()}


def child(args):
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(args.root, "tests"))
    import torch

    from torchain_amd import io, synth
    from torchain_amd._lib import check, lib
    from torchain_amd.functions import chain_loss

    dev = "cuda:0"
    stream = torch.cuda.current_stream().cuda_stream

    def numerator(sup, y2d):
        S = sup.n_batch
        nbytes = 256 * ((S * 8 + 255) // 256) + 256
        deriv, ws_ = torch.zeros_like(y2d), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        lp = torch.zeros(1, dtype=torch.float64, device=dev)

        def num():
            check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y2d.data_ptr()), y2d.shape[0], y2d.shape[1], y2d.stride(0),
                                              C.c_void_p(deriv.data_ptr()), y2d.shape[1], C.c_void_p(lp.data_ptr()),
                                              C.c_void_p(ws_.data_ptr()), nbytes, torch.cuda.current_device(),
                                              C.c_void_p(stream)), "tc_num_forward_backward")
        return num, deriv, lp

    def report(**kw):
        print(json.dumps(dict(kind=args.kind, **kw)), flush=True)

    if args.kind == "forced":
        import wide_supervisions as ws
        for name in ("lattice_wide", "lattice_bursty"):
            y = torch.from_numpy(ws.nnet_output(name)).to(dev)
            fns, results = {}, {}
            for kernel, switch in (("windowed", b"force_num_windowed"), ("wide", b"force_num_wide")):
                sup = io.Supervision.from_synth(ws.supervision(name), any_width=True)
                num, deriv, lp = numerator(sup, y)

                def run(num=num, switch=switch):  # (the switch is read when the handle is staged and at every launch)
                    check(lib.tc_debug_set(switch, 1), "tc_debug_set")
                    num()
                    check(lib.tc_debug_set(switch, 0), "tc_debug_set")
                run()
                torch.cuda.synchronize()
                results[kernel] = (deriv.cpu().numpy().tobytes(), lp.cpu().numpy().tobytes())
                fns[kernel] = run
            st = io.Supervision.from_synth(ws.supervision(name)).stats()
            report(case=name, what="num", level_states=st["max_level_states"], level_arcs=st["max_level_arcs"],
                   same_bits=results["windowed"] == results["wide"], **timed(torch, fns, args.iters, args.warmup))
        report(num_wide_launches=int(lib.tc_debug_counter(b"num_wide_launches")),
               num_windowed_launches=int(lib.tc_debug_counter(b"num_windowed_launches")))
        return

    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    graph = io.DenominatorGraph(synth.config_den_fst(args.config), P).prepare(dev)
    y2d = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)

    def step_of(sup):
        x = y2d.view(T, S, P).permute(1, 2, 0).contiguous().requires_grad_(True)

        def step():
            x.grad = None
            loss, _ = chain_loss(x, graph, sup, l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"])
            loss.backward()
        return step

    if args.kind == "wide12k":
        import wide_supervisions as ws
        pieces = [ws.lattice_supervision(1, T, P, lambda q, t, r: 12000 if t % 50 == 25 else r.integers(2, 12), 1, seed=70 + i,
                                         final_weights=True) for i in range(4)]
        for form, streamed in (("lds", 0), ("slot", 1)):
            check(lib.tc_debug_set(b"force_num_wide_streamed", streamed), "tc_debug_set")
            sup = io.Supervision.from_sequences([pieces[i % 4] for i in range(S)], any_width=True)
            st = sup.stats()
            assert st["kernel"] == "wide" and sup.wide_stats()["form"] == form, (st, sup.wide_stats())
            fns = dict(num_ms=numerator(sup, y2d)[0], step_ms=step_of(sup))
            report(case="wide12k", form=form, states=st["max_states"], arcs=st["max_arcs"], scratch_bytes=sup.wide_stats()["scratch_bytes"],
                   history_bytes=st["history_bytes"], **timed(torch, fns, args.iters, args.warmup))
            del sup, fns
        report(num_wide_launches=int(lib.tc_debug_counter(b"num_wide_launches")))
        return

    # kind "step-this" / "step-parent": the C3 step on a resident and on a windowed handle
    fns = {case: step_of(io.Supervision.from_synth(tw.load_supervision(synth, args.config, args.cache_dir, case))) for case in STEP_CASES}
    for case, ms in timed(torch, fns, args.iters, args.warmup).items():
        report(case=case, what="step", median_ms=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit to compare with (part 'step')")
    ap.add_argument("--cache-dir", default=None, help="where the C3 supervisions are kept (default: a temporary directory)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kind", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.join(HERE, ".."), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    this = os.path.abspath(args.root)
    cache = os.path.abspath(args.cache_dir) if args.cache_dir else tempfile.mkdtemp(prefix="time_num_wide_")
    os.makedirs(cache, exist_ok=True)
    tw.make_supervisions(args.config, cache)
    steps = ([("step-parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("step-this", this)]
    runs = [("wide12k", this), ("forced", this)] + steps * args.rounds
    rows = {}
    for kind, root in runs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--kind", kind, "--root", root, "--config", args.config,
               "--iters", str(args.iters), "--warmup", str(args.warmup), "--cache-dir", cache]
        # (a child that fails or hangs ends the run: nothing more is started on the GPU behind it)
        out = subprocess.run(cmd, check=True, timeout=args.timeout, stdout=subprocess.PIPE, text=True, cwd=root).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                r = json.loads(line)
                if r.get("what") == "step":
                    rows.setdefault((r["case"], r["kind"]), []).append(r["median_ms"])
    print("# C3 step, case kind: median over the rounds of the rounds' medians (ms), spread max - min, the rounds")
    for (case, kind), v in sorted(rows.items()):
        s = sorted(v)
        print("# %-7s %-11s %.3f  spread %.3f  %s" % (case, kind, s[len(s) // 2], s[-1] - s[0], " ".join("%.3f" % x for x in v)))


if __name__ == "__main__":
    main()
