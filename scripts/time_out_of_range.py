"""Training step (chain_loss + backward) at C3 with the out-of-range penalty, in three forms of the network output --
(B, C, T) float32, (B, C, T) bfloat16 and 2-D float32 -- and five ways each:

    parent   the step of another checkout of this repository (``--parent-root``, built there): the commit before the penalty
    alone    this checkout, the keyword left out (c = 0), in a child process that times nothing else -- as ``parent`` is timed
    zero     the same, taking turns with the three ways below
    clean    ``out_of_range_regularize=c`` on N(0, 1) outputs: nothing out of range
    sparse   the same with about 1 % of the elements at +-(30 + U(0.5, 20))
    hook     c = 0 and the workaround: a gradient hook on the output that adds the same term with torch ops (sparse outputs)

Two builds of the library cannot share a process, so the script starts one child process per checkout and round, parent and
this checkout (``alone``, then the other four ways) taking turns, ``--rounds`` of each; inside a child the ways of a form take
turns step by step.  Each child prints
the median and min wall time of a step (CUDA events) per form and way; the parent process never opens the GPU and prints, per
form and way, the median over the rounds and their spread (max - min of the rounds' medians): the spread of the repeated
``parent`` runs is the run-to-run noise that ``alone`` has to stay within.

    python scripts/time_out_of_range.py [--parent-root DIR] [--rounds 3] [--iters 20] [--warmup 5] [--config C3]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = ("bct_f32", "bct_bf16", "2d_f32")
WAYS = ("zero", "clean", "sparse", "hook")
C_REG, LIMIT = 0.01, 30.0


def child(args):
    sys.path.insert(0, args.root)
    import torch

    from torchain_amd import io, synth
    from torchain_amd.functions import chain_loss

    ways = [args.only] if args.only else list(WAYS)
    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    dev = "cuda:0"
    fst = synth.config_den_fst(args.config)
    graph = io.DenominatorGraph(fst, P).prepare(dev)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=3))
    clean = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    mask = torch.rand(clean.shape, device=dev, generator=g) < 0.01
    sign = torch.where(torch.rand(clean.shape, device=dev, generator=g) < 0.5, -1.0, 1.0)
    sparse = torch.where(mask, sign * (30.5 + 19.5 * torch.rand(clean.shape, device=dev, generator=g)), clean)
    del mask, sign
    to3d = lambda t: t.view(T, S, P).permute(1, 2, 0).contiguous()  # noqa: E731
    forms = {"bct_f32": lambda t: to3d(t), "bct_bf16": lambda t: to3d(t).to(torch.bfloat16), "2d_f32": lambda t: t.clone()}

    def make_step(make, way):
        x = make(clean if way in ("parent", "alone", "zero", "clean") else sparse).requires_grad_(True)
        kw = dict(l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"])
        if way in ("clean", "sparse"):
            kw.update(out_of_range_regularize=C_REG)

        def add_term(grad):  # (the library's statement with torch ops, as a caller without the option would write it)
            y = x.detach().float()
            p = torch.where(y > LIMIT, y - LIMIT, torch.where(y < -LIMIT, y + LIMIT, torch.zeros_like(y)))
            return (grad.float() + p * (2.0 * C_REG)).to(grad.dtype)

        def step():
            x.grad = None
            out = x
            if way == "hook":
                out = x.view_as(x)
                out.register_hook(add_term)
            loss, _ = chain_loss(out, graph, sup, **kw)
            loss.backward()

        return step

    for name in args.forms.split(","):
        steps = {way: make_step(forms[name], way) for way in ways}
        for _ in range(args.warmup):
            for way in ways:
                steps[way]()
        torch.cuda.synchronize()
        times = {way: [] for way in ways}
        for _ in range(args.iters):
            for way in ways:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                steps[way]()
                b.record()
                b.synchronize()
                times[way].append(a.elapsed_time(b))
        for way in ways:
            t = sorted(times[way])
            print(json.dumps(dict(config=args.config, form=name, way=way, iters=args.iters, median_ms=round(t[len(t) // 2], 4),
                                  min_ms=round(t[0], 4))), flush=True)
        del steps
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit to compare with (way 'parent')")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--only", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.join(HERE, ".."), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    this = os.path.abspath(args.root)
    roots = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("alone", this), (None, this)]
    rows = {}
    for rnd in range(args.rounds):
        for who, root in roots:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--config", args.config, "--iters",
                   str(args.iters), "--warmup", str(args.warmup), "--forms", args.forms] + (["--only", who] if who else [])
            # (a child that fails or hangs ends the run: nothing more is started on the GPU behind it)
            out = subprocess.run(cmd, check=True, timeout=args.timeout, stdout=subprocess.PIPE, text=True, cwd=root).stdout
            for line in out.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    r["round"] = rnd
                    print(json.dumps(r), flush=True)
                    rows.setdefault((r["form"], r["way"]), []).append(r["median_ms"])
    print("# form way: median over %d rounds of the rounds' medians (ms), spread max - min" % args.rounds)
    for (form, way), v in rows.items():
        s = sorted(v)
        print("# %-9s %-7s %.3f  spread %.3f  %s" % (form, way, s[len(s) // 2], s[-1] - s[0], " ".join("%.3f" % x for x in v)))


if __name__ == "__main__":
    main()
