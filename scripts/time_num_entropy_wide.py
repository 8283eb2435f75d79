"""What the wide-level entropy kernel (``csrc/num_entropy_wide_kernels.hip``) costs, at C3's shape (256 x 150, 4096 pdfs), 2-D
float32 outputs.  Two parts, each a child process; the process that starts them never opens the GPU.

  wide12k   the batch of ``scripts/time_num_wide.py``: every sequence has three levels of 12000 states (four different sequences,
            each 64 times, ``from_sequences(any_width=True)``).  The entropy's value alone and the value with its gradient,
            beside the wide-level numerator's forward-backward (``tc_num_forward_backward`` with a derivative) on the same handle.
            A 12000-state level is beyond the entropy kernel's LDS form: this is its slot form.
  forced    the three supervisions of ``scripts/time_num_entropy_regular.py`` (three paths, forty paths, lattice-like): the
            level-windowed entropy kernel and the wide-level one (``force_num_entropy_wide``) on the same handle, taking turns,
            their outputs compared byte for byte.  ``--regular-only`` times the level-windowed kernel alone: run on this checkout
            and on the parent's, alternated, it shows whether that kernel moved.

Every figure is the median of ``--rounds`` rounds' medians of ``--iters`` calls between two device events, the entries taking
turns, after ``--warmup`` calls; the smallest and the largest round beside it.

    python scripts/time_num_entropy_wide.py [--rounds 5] [--iters 10] [--warmup 5] [--cache DIR] [--regular-only] [--build-only]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import time_num_entropy_regular as tr  # noqa: E402  (the three C3 supervisions and their cache)


def child(args):
    sys.path.insert(0, os.path.join(tr.ROOT, "tests"))
    import torch

    from torchain_amd import egs, io, synth
    from torchain_amd._lib import check, lib

    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    dev, device = "cuda:0", torch.cuda.current_device()
    stream = torch.cuda.current_stream().cuda_stream
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    out = torch.zeros_like(y)
    lp = torch.zeros(1, dtype=torch.float64, device=dev)
    num_bytes = 256 * ((S * 8 + 255) // 256) + 256
    query = lib.tc_supervision_path_entropy_regular_workspace_bytes

    def rounds_of(calls):
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in calls}
        for _ in range(args.rounds):
            times = {k: [] for k in calls}
            for _ in range(args.iters):
                for k, fn in calls.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    times[k].append(a.elapsed_time(b))
            for k, v in times.items():
                rounds[k].append(sorted(v)[len(v) // 2])
        return {k + "_ms": [round(sorted(v)[len(v) // 2], 4), round(min(v), 4), round(max(v), 4)] for k, v in rounds.items()}

    def entropy_of(sup, ws, force, grad):
        ent, elp = (torch.zeros(S, dtype=torch.float64, device=dev) for _ in range(2))

        def run():  # (the switch is read at every call)
            check(lib.tc_debug_set(b"force_num_entropy_wide", force), "tc_debug_set")
            check(lib.tc_supervision_path_entropy_regular(
                sup.ptr, C.c_void_p(y.data_ptr()), 0, 0, S * T, P, y.stride(0), C.c_void_p(ent.data_ptr()), C.c_void_p(elp.data_ptr()),
                C.c_void_p(out.data_ptr()) if grad else None, P, None, C.c_void_p(ws.data_ptr()), ws.numel(), device,
                C.c_void_p(stream)), "tc_supervision_path_entropy_regular")
            check(lib.tc_debug_set(b"force_num_entropy_wide", 0), "tc_debug_set")
        return run, ent, elp

    def workspace(sup, force):
        check(lib.tc_debug_set(b"force_num_entropy_wide", force), "tc_debug_set")
        need = [int(query(sup.ptr, g)) for g in (0, 1)]
        kernel = sup.path_entropy_regular_kernel()
        check(lib.tc_debug_set(b"force_num_entropy_wide", 0), "tc_debug_set")
        check(min(need + [0]), "tc_supervision_path_entropy_regular_workspace_bytes")
        return torch.empty(max(need + [num_bytes]), dtype=torch.uint8, device=dev), need, kernel

    if args.kind == "wide12k":
        import wide_supervisions as ws_
        pieces = [ws_.lattice_supervision(1, T, P, lambda q, t, r: 12000 if t % 50 == 25 else r.integers(2, 12), 1, seed=70 + i,
                                          final_weights=True) for i in range(4)]
        sup = io.Supervision.from_sequences([pieces[i % 4] for i in range(S)], any_width=True)
        ws, need, kernel = workspace(sup, 0)

        def numerator():
            check(lib.tc_num_forward_backward(sup.ptr, C.c_void_p(y.data_ptr()), S * T, P, y.stride(0), C.c_void_p(out.data_ptr()), P,
                                              C.c_void_p(lp.data_ptr()), C.c_void_p(ws.data_ptr()), num_bytes, device,
                                              C.c_void_p(stream)), "tc_num_forward_backward")
        value, ent, elp = entropy_of(sup, ws, 0, False)
        calls = dict(numerator=numerator, entropy_value=value, entropy_value_grad=entropy_of(sup, ws, 0, True)[0])
        row = rounds_of(calls)
        numerator()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ent).all()) and abs(float(elp.sum()) - float(lp[0])) <= 1e-9 * abs(float(lp[0]))
        print(json.dumps(dict(kind="wide12k", numerator_kernel=sup.stats()["kernel"], entropy_kernel=kernel, workspace_value_mb=round(need[0] / 2 ** 20, 1),
                              workspace_grad_mb=round(need[1] / 2 ** 20, 1), mean_entropy=round(float(ent.mean()), 3), **row)), flush=True)
    else:
        for case in tr.CASES:
            sup = io.Supervision.from_synth(egs.append_supervisions(tr.pieces(synth, args.config, args.cache, case)))
            calls, outs = {}, {}
            for name, force in (("regular", 0),) + ((("wide", 1),) if not args.regular_only else ()):
                ws, need, kernel = workspace(sup, force)
                assert kernel == force
                for grad in (False, True):
                    run, ent, elp = entropy_of(sup, ws, force, grad)
                    calls["%s_value%s" % (name, "_grad" if grad else "")] = run
                run()
                torch.cuda.synchronize()
                outs[name] = (out.cpu().numpy().tobytes(), ent.cpu().numpy().tobytes(), elp.cpu().numpy().tobytes())
            same = None if args.regular_only else outs["regular"] == outs["wide"]
            print(json.dumps(dict(kind="forced", case=case, same_bits=same, **rounds_of(calls))), flush=True)
    print(json.dumps({k: int(lib.tc_debug_counter(k.encode())) for k in ("num_entropy_regular_launches", "num_entropy_wide_launches")}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cache", default=os.path.join(tr.ROOT, "build", "time_num_entropy_regular"))
    ap.add_argument("--regular-only", action="store_true")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--timeout", type=int, default=400, help="seconds a child may take")
    ap.add_argument("--kind", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kind:
        return child(args)
    from torchain_amd import synth
    for case in tr.CASES:
        tr.pieces(synth, args.config, args.cache, case)
    if args.build_only:
        return
    for kind in ("forced",) if args.regular_only else ("wide12k", "forced"):
        cmd = [sys.executable, os.path.abspath(__file__), "--kind", kind] + sys.argv[1:]
        # (a child that fails or hangs ends the run: nothing more is started on the GPU behind it)
        subprocess.run(cmd, check=True, timeout=args.timeout, cwd=tr.ROOT)


if __name__ == "__main__":
    main()
