"""What boosted LF-MMI costs over the plain step, at C3's shape (S = 256, T = 150).

Times ``chain_loss`` + backward -- the plain step, the hard boost (``boost_ref``, without classes) and the dense boost
(``boost_accuracy``) -- for ``(B, C, T)`` float32 and bfloat16 and for 2-D float32, with C3's l2 (the l2 fix-up runs) and
with l2 = 0 (the pass alone).  Medians of device times between events, after a warm-up.

``--parent DIR``: a built checkout of the parent commit.  The plain step is then timed there and here in alternation
(``--rounds`` child processes each, ``--plain-only``), so that the two sides see the same box in the same minutes; the table
gives every round, the medians and each side's own spread.

    python scripts/time_boost.py [--parent DIR] [--rounds 5] [--iters 30] [--warmup 8]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = (("bct", "float32"), ("bct", "bfloat16"), ("rows", "float32"))


def _workload():
    import torch
    from torchain_amd import io, synth

    S, T = 256, 150
    cfg = synth.CONFIGS["C3"]
    fst = synth.config_den_fst("C3")
    graph = io.DenominatorGraph(fst, cfg["P"]).prepare("cuda:0")
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=5))
    y = torch.from_numpy(synth.random_nnet_output(S, T, cfg["P"], seed=6)).to("cuda:0")
    return S, T, cfg, graph, sup, y


def _time(fn, iters, warmup):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def measure(iters, warmup, plain_only):
    import torch
    from torchain_amd.functions import chain_loss

    S, T, cfg, graph, sup, y = _workload()
    P = cfg["P"]
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    ref = torch.randint(0, P, (S, T), device="cuda:0", dtype=torch.int32, generator=gen)
    acc = torch.rand(S * T, P, device="cuda:0", generator=gen)
    out = {}
    for layout, dtype in CONFIGS:
        x = y.to(getattr(torch, dtype))
        x = x.view(T, S, P).permute(1, 2, 0).contiguous() if layout == "bct" else x.clone()
        x.requires_grad_(True)
        for l2 in ((cfg["l2"],) if plain_only else (cfg["l2"], 0.0)):
            variants = {"plain": {}}
            if not plain_only:
                variants["hard"] = dict(boost=1.0, boost_ref=ref)
                variants["dense"] = dict(boost=1.0, boost_accuracy=acc)
            for name, kw in variants.items():
                def step():
                    loss, _ = chain_loss(x, graph, sup, l2_regularize=l2, leaky_hmm_coefficient=cfg["leaky"], **kw)
                    torch.autograd.grad(loss, x)

                out["%s %s l2=%g %s" % (layout, dtype, l2, name)] = _time(step, iters, warmup)
    return out


def _child(root, args):
    env = dict(os.environ, PYTHONPATH=root)
    cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--json", "--iters", str(args.iters), "--warmup", str(args.warmup)]
    res = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise SystemExit("child in %s failed:\n%s" % (root, res.stderr[-2000:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if args.plain_only:
        sys.path.insert(0, os.environ.get("PYTHONPATH", HERE).split(os.pathsep)[0])
        out = measure(args.iters, args.warmup, True)
        print(json.dumps(out) if args.json else "\n".join("%-40s %.3f ms" % kv for kv in out.items()))
        return
    if args.parent:
        rounds = {"parent": [], "this": []}
        for _ in range(args.rounds):  # alternated: parent, this, parent, this, ...
            rounds["parent"].append(_child(os.path.abspath(args.parent), args))
            rounds["this"].append(_child(HERE, args))
        print("plain step (chain_loss + backward), ms, alternated rounds: parent | this commit")
        for key in rounds["this"][0]:
            p, t = [r[key] for r in rounds["parent"]], [r[key] for r in rounds["this"]]
            print("%-28s parent %s  median %.3f  spread %.3f | this %s  median %.3f  spread %.3f" % (
                key, " ".join("%.3f" % v for v in p), statistics.median(p), max(p) - min(p),
                " ".join("%.3f" % v for v in t), statistics.median(t), max(t) - min(t)))
        print()
    sys.path.insert(0, HERE)
    out = measure(args.iters, args.warmup, False)
    print("chain_loss + backward at C3's shape (S = 256, T = 150), ms, median of %d" % args.iters)
    for key, ms in out.items():
        base = out[key.rsplit(" ", 1)[0] + " plain"]
        print("%-40s %.3f ms  (%+.3f over plain)" % (key, ms, ms - base))


if __name__ == "__main__":
    main()
