"""Training and evaluation step at C3 with the cross-entropy branch (kaldi_way=True), the head's log-softmax taken three ways:

    torch  the route callers took before the option: ``chain_loss(y, ..., xent_input=F.log_softmax(xe, dim=1))``, the
           log-softmax and its backward INSIDE the timed step;
    fused  ``chain_loss(y, ..., xent_input=xe, xent_log_softmax=True)`` (tc_chain_step_log_softmax);
    off    ``chain_loss(y, ..., xent_input=xe)``: no log-softmax anywhere -- the step as it was, for the cost of the option off.

Forms of the two network outputs: (B, C, T) float32 and bfloat16, 2-D float32 rows, a batch-first (B, T, C) float32 view.
Every way runs in child processes of its own that take turns, ``--rounds`` times; a child times ``--iters`` steps per form with
CUDA events and reports the median and ``torch.cuda.max_memory_allocated``.  The parent prints, per form and step, the median
over the rounds of every way and the spread (min .. max of the rounds' medians) of the torch route, which is the yardstick.

    python scripts/time_xent_log_softmax.py [--config C3] [--rounds 3] [--iters 20] [--warmup 5] [--forms ...] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
WAYS = ("torch", "fused", "off")
FORMS = ("bct_f32", "bct_bf16", "2d_f32", "batch_first_f32")


def child(args):
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ROOT)
    from torchain_amd import io, synth
    from torchain_amd.functions import chain_loss

    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    dev = "cuda:0"
    fst = synth.config_den_fst(args.config)
    graph = io.DenominatorGraph(fst, P).prepare(dev)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=3, initial_probs=graph.initial_probs()))
    y2d = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    xe2d = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=5, scale=3.0)).to(dev)
    make = {
        "bct_f32": lambda t: t.view(T, S, P).permute(1, 2, 0).contiguous(),
        "bct_bf16": lambda t: t.view(T, S, P).permute(1, 2, 0).contiguous().to(torch.bfloat16),
        "2d_f32": lambda t: t.clone(),
        "batch_first_f32": lambda t: t.view(T, S, P).permute(1, 0, 2).contiguous().permute(0, 2, 1),
    }
    kw = dict(l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"], xent_regularize=0.1, kaldi_way=True)
    if args.way == "fused":
        kw["xent_log_softmax"] = True
    for form in args.forms.split(","):
        x = make[form](y2d).detach().requires_grad_(True)
        xi = make[form](xe2d).detach().requires_grad_(True)

        def train():
            x.grad = None
            xi.grad = None
            loss, _ = chain_loss(x, graph, sup, xent_input=F.log_softmax(xi, dim=1) if args.way == "torch" else xi, **kw)
            loss.backward()

        def evaluate():
            with torch.no_grad():
                chain_loss(x, graph, sup, xent_input=F.log_softmax(xi, dim=1) if args.way == "torch" else xi, **kw)

        for step_name, step in (("train", train), ("eval", evaluate)):
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            times = []
            for _ in range(args.iters):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
            times.sort()
            print(json.dumps(dict(config=args.config, S=S, T=T, P=P, form=form, step=step_name, way=args.way, iters=args.iters,
                                  median_ms=round(times[len(times) // 2], 4), min_ms=round(times[0], 4),
                                  peak_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
                                  resident_mb=round(base / 2 ** 20, 1))), flush=True)
        del x, xi
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--ways", default=",".join(WAYS))
    ap.add_argument("--way", default=None, help="(a child's: the one way it times)")
    ap.add_argument("--out", default=None, help="file that receives every child's raw lines")
    args = ap.parse_args()
    if args.way:
        return child(args)
    ways = [w for w in WAYS if w in args.ways.split(",")]
    rows = []
    for rnd in range(args.rounds):
        for way in ways:  # (the ways take turns, a fresh process each: clock and allocator state hit them alike)
            cmd = [sys.executable, os.path.abspath(__file__), "--config", args.config, "--iters", str(args.iters), "--warmup",
                   str(args.warmup), "--forms", args.forms, "--way", way]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
            if done.returncode != 0:
                print("child %s of round %d ended with %d: stopping" % (way, rnd, done.returncode), flush=True)
                return done.returncode
            for line in done.stdout.splitlines():
                if line.startswith("{"):
                    rows.append(dict(json.loads(line), round=rnd))
                    print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    print("\n%-16s %-5s | %s | torch spread (min .. max) | peak MB %s" % ("form", "step", " ".join("%9s" % w for w in ways),
                                                                      " ".join("%9s" % w for w in ways)))
    for form in args.forms.split(","):
        for step in ("train", "eval"):
            sel = lambda w: [r for r in rows if r["form"] == form and r["step"] == step and r["way"] == w]  # noqa: E731
            ms = {w: med([r["median_ms"] for r in sel(w)]) for w in ways if sel(w)}
            mem = {w: max(r["peak_mb"] for r in sel(w)) for w in ways if sel(w)}
            t = [r["median_ms"] for r in sel("torch")] or [float("nan")]
            print("%-16s %-5s | %s | %9.4f .. %9.4f    | %s" % (form, step, " ".join("%9.4f" % ms.get(w, float("nan")) for w in ways),
                                                              min(t), max(t), " ".join("%9.1f" % mem.get(w, float("nan")) for w in ways)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
