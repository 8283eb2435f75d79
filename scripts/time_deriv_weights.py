"""Training step (chain_loss + backward) at C3 with Kaldi's per-frame derivative weights, in three forms of the network
output -- (B, C, T) float32, (B, C, T) bfloat16 and 2-D float32 -- and three ways each: without weights, with
``deriv_weights=w`` (tc_chain_step_weighted) and with the workaround of a gradient hook on the output
(``out.register_hook(lambda g: g * w_in_layout)``, one more pass and allocation per gradient).  Without and with the
cross-entropy branch (kaldi_way=True).  Prints one line per case: median and min wall time of a step over the timed
iterations (CUDA events; the ways of a form take turns step by step).

    python scripts/time_deriv_weights.py [--config C3] [--iters 20] [--warmup 5] [--forms bct_f32,bct_bf16,2d_f32] [--xent 0,1]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from torchain_amd import io, synth  # noqa: E402
from torchain_amd.functions import chain_loss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--forms", default="bct_f32,bct_bf16,2d_f32", help="comma-separated subset of the forms")
    ap.add_argument("--xent", default="0,1", help="comma-separated: 0 without, 1 with the cross-entropy branch")
    ap.add_argument("--ways", default=",".join(WAYS), help="comma-separated subset of the ways")
    args = ap.parse_args()
    ways = [v for v in WAYS if v in args.ways.split(",")]
    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    dev = "cuda:0"
    fst = synth.config_den_fst(args.config)
    graph = io.DenominatorGraph(fst, P).prepare(dev)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=3, initial_probs=graph.initial_probs()))
    y2d = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
    xe2d = torch.log_softmax(y2d, dim=1)
    # <DW>-like weights: mostly 1, below 1 on some frames, some 0
    w = torch.from_numpy(np.random.default_rng(5).choice(np.array([0.0, 0.5, 0.75, 1.0, 1.0, 1.0], np.float32), S * T)).to(dev)
    to3d = lambda t: t.view(T, S, P).permute(1, 2, 0).contiguous()  # noqa: E731
    forms = {
        "bct_f32": (lambda t: to3d(t), torch.float32, w.view(T, S).t().unsqueeze(1)),
        "bct_bf16": (lambda t: to3d(t).to(torch.bfloat16), torch.bfloat16, w.view(T, S).t().unsqueeze(1)),
        "2d_f32": (lambda t: t.clone(), torch.float32, w.unsqueeze(1)),
    }
    for xent in [bool(int(v)) for v in args.xent.split(",")]:
        for name, (make, dtype, w_layout) in forms.items():
            if name not in args.forms.split(","):
                continue
            w_hook = w_layout.to(dtype)
            steps = {way: make_step(make, y2d, xe2d, xent, way, w, w_hook, cfg, graph, sup) for way in ways}
            for _ in range(args.warmup):
                for way in ways:
                    steps[way]()
            torch.cuda.synchronize()
            times = {way: [] for way in ways}
            for _ in range(args.iters):  # (the three ways interleaved: clock and allocator drift hit them alike)
                for way in ways:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    steps[way]()
                    b.record()
                    b.synchronize()
                    times[way].append(a.elapsed_time(b))
            for way in ways:
                t = sorted(times[way])
                print(json.dumps(dict(config=args.config, S=S, T=T, P=P, xent=xent, form=name, way=way, iters=args.iters,
                                      median_ms=round(t[len(t) // 2], 4), min_ms=round(t[0], 4))), flush=True)
            del steps


WAYS = ("none", "weighted", "hook")


def make_step(make, y2d, xe2d, xent, way, w, w_hook, cfg, graph, sup):
    x = make(y2d).requires_grad_(True)
    xi = make(xe2d).requires_grad_(True) if xent else None
    kw = dict(l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"])
    if xent:
        kw.update(xent_regularize=0.1, xent_input=xi, kaldi_way=True)
    if way == "weighted":
        kw.update(deriv_weights=w)

    def step():
        x.grad = None
        out = x
        if xent:
            xi.grad = None
        if way == "hook":  # (what a caller has to do without deriv_weights: a view to hang the hook on)
            out = x.view_as(x)
            out.register_hook(lambda g: g * w_hook)
            if xent:
                xo = xi.view_as(xi)
                xo.register_hook(lambda g: g * w_hook)
                kw["xent_input"] = xo
        loss, _ = chain_loss(out, graph, sup, **kw)
        loss.backward()

    return step


if __name__ == "__main__":
    main()
