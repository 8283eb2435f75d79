"""Training step (chain_loss + backward) at C3 on its tied graph, (B, C, T) float32 and 2-D float32, four ways:

    parent    the step of another checkout of this repository (``--parent-root``, built there): the commit before the
              per-sequence entry
    alone     this checkout with the defaults (``tc_chain_step_strided``), in a child process that times nothing else -- as
              ``parent`` is timed
    default   the same, taking turns with the two ways below
    report    ``per_sequence=True``: the sibling epilogue and the (S, 6) buffer, nothing else
    isolate   ``on_failure="sequence"`` with nothing failing: the report plus the zeroing launch on a uniform handle

Two builds of the library cannot share a process, so the script starts one child process per checkout and round, parent and
this checkout (``alone``, then the other three ways) taking turns, ``--rounds`` of each; inside a child the ways of a form take
turns step by step.  Each child prints the median and min wall time of a step (CUDA events) per form and way; the parent
process never opens the GPU and prints, per form and way, the median over the rounds and their spread (max - min of the
rounds' medians): the spread of the repeated ``parent`` runs is the run-to-run noise that ``alone`` has to stay within, and
``isolate - default`` is the cost of the switch.

    python scripts/time_per_sequence.py [--parent-root DIR] [--rounds 3] [--iters 20] [--warmup 5] [--config C3]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = ("bct_f32", "2d_f32")
WAYS = ("default", "report", "isolate")
OPTIONS = {"report": dict(per_sequence=True), "isolate": dict(on_failure="sequence")}


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
    assert graph.stats()["tied"] == 1
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=3))
    clean = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    forms = {"bct_f32": lambda t: t.view(T, S, P).permute(1, 2, 0).contiguous(), "2d_f32": lambda t: t.clone()}

    def make_step(make, way):
        x = make(clean).requires_grad_(True)
        kw = dict(l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"], **OPTIONS.get(way, {}))

        def step():
            x.grad = None
            loss, _ = chain_loss(x, graph, sup, **kw)
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
        print("# %-9s %-8s %.3f  spread %.3f  %s" % (form, way, s[len(s) // 2], s[-1] - s[0], " ".join("%.3f" % x for x in v)))


if __name__ == "__main__":
    main()
