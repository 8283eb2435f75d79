"""Training step (chain_loss + backward) at C3 on a (B, C, T) network output in three forms: float32 input, bfloat16 input
taken as it is (tc_chain_step_typed), and bfloat16 through ``out.float()`` (the up-cast and autograd's cast of the
gradient back to bfloat16 around the float32 step).  Without and with the cross-entropy branch (kaldi_way=True).
Prints one line per case: median and min wall time of a step over the timed iterations (CUDA events).

    python scripts/time_half_step.py [--config C3] [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from torchain_amd import io, synth  # noqa: E402
from torchain_amd.functions import chain_loss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    dev = "cuda:0"
    fst = synth.config_den_fst(args.config)
    graph = io.DenominatorGraph(fst, P).prepare(dev)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=3, initial_probs=graph.initial_probs()))
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev).view(T, S, P).permute(1, 2, 0).contiguous()
    xe = torch.log_softmax(y, dim=1)
    forms = {
        "f32": lambda t: t,
        "bf16_native": lambda t: t,
        "bf16_via_float": lambda t: t.float(),
    }
    for xent in (False, True):
        for name, prep in forms.items():
            dtype = torch.float32 if name == "f32" else torch.bfloat16
            x = y.to(dtype, copy=True).requires_grad_(True)
            xi = xe.to(dtype, copy=True).requires_grad_(True) if xent else None
            kw = dict(l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"])
            if xent:
                kw.update(xent_regularize=0.1, xent_input=xi, kaldi_way=True)

            def step():
                x.grad = None
                if xent:
                    xi.grad = None
                    kw["xent_input"] = prep(xi)
                loss, _ = chain_loss(prep(x), graph, sup, **kw)
                loss.backward()

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
            print(json.dumps(dict(config=args.config, S=S, T=T, P=P, xent=xent, form=name, iters=args.iters,
                                  median_ms=round(times[len(times) // 2], 4), min_ms=round(times[0], 4))), flush=True)
            del x, xi


if __name__ == "__main__":
    main()
