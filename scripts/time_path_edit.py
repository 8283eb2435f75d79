"""What scoring sampled paths by edit distance costs on the device (``tc_paths_edit_distance``) beside the Python loop it
replaces, and what the fused gradient of ``sampled_risk_surrogate`` (``tc_sampled_risk_grad``) does to a sampled step:

    device_edit      path_edit_distance on K = 8 sampled paths a sequence (collapse mode; and start mode)
    loop_edit        the same paths through the host: .cpu(), a Python token rule and a two-row Levenshtein per path,
                     torch.tensor(...).to(device) -- the route of the docstring this entry replaces, its two copies included
    step_loop_torch    den_sample_paths -> loop_edit   -> sampled_risk_surrogate(...).sum().backward()
    step_device_torch  den_sample_paths -> device_edit -> sampled_risk_surrogate(...).sum().backward()
    step_device_fused  den_sample_paths -> device_edit -> sampled_risk_surrogate(..., fused=True).sum().backward()
    surrogate_torch / surrogate_fused   the surrogate's forward and backward alone, on fixed paths and risks

    C3      256 x 150 frames, 4096 pdfs, 8192 states / 65536 arcs; references of 30 .. 50 tokens over 41 phones

pdf ``j`` belongs to phone ``(j // 2) % 42``, phone 0 being silence; an even pdf starts its phone.  Device events around every
call (each ends in a synchronise); the host loop is timed by the same events, which span it.  ``--iters`` timed calls after
``--warmup``, the two routes through the host ``--loop-iters`` after one; per case one JSON line with medians, minima and
quartiles.  The values' checks are tests/test_gpu_path_edit.py's; here only that both routes give the same distances.

    python scripts/time_path_edit.py [--iters 10] [--warmup 2] [--loop-iters 3] [--configs C3:256]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def phones_of(pdfs, phone_of_pdf):
    out, before = [], -1
    for q in pdfs:
        c = phone_of_pdf[q]
        if c >= 0 and c != before:
            out.append(c)
        before = c
    return out


def edit_distance(h, r):
    prev = list(range(len(r) + 1))
    for i, a in enumerate(h, 1):
        cur = [i] + [0] * len(r)
        for j, b in enumerate(r, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a != b))
        prev = cur
    return prev[len(r)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--configs", default="C3:256")
    args = ap.parse_args()

    import numpy as np
    import torch

    from torchain_amd import io, synth
    from torchain_amd.functions import den_sample_paths, path_edit_distance, sampled_risk_surrogate

    if not torch.cuda.is_available():
        raise SystemExit("time_path_edit.py measures on the GPU: none is available")
    dev = "cuda:0"
    K = 8
    for item in args.configs.split(","):
        config, S = item.split(":")[0], int(item.split(":")[1])
        cfg = synth.CONFIGS[config]
        T, P, leaky = cfg["T"], cfg["P"], cfg["leaky"]
        t0 = time.time()
        fst = synth.config_den_fst(config)
        graph = io.DenominatorGraph(fst, P).prepare(dev)
        print("# %s: %d states, %d arcs, ready in %.1f s" % (config, graph.num_states, graph.num_arcs, time.time() - t0), flush=True)
        rng = np.random.default_rng(3)
        phone_np = ((np.arange(P) // 2) % 42 - 1).astype(np.int32)
        phone_list = phone_np.tolist()
        lengths = rng.integers(30, 51, S).astype(np.int32)
        refs_np = np.full((S, 50), -1, np.int32)
        for b, m in enumerate(lengths):
            refs_np[b, :m] = rng.integers(0, 41, m)
        ref_lists = [refs_np[b, :m].tolist() for b, m in enumerate(lengths)]
        phone_of_pdf = torch.from_numpy(phone_np).to(dev)
        starts = torch.from_numpy((np.arange(P) % 2 == 0).astype(np.uint8)).to(dev)
        refs, ref_lengths = torch.from_numpy(refs_np).to(dev), torch.from_numpy(lengths).to(dev)
        y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=4)).to(dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        fixed = den_sample_paths(y, graph, K, n_batch=S, leaky_hmm_coefficient=leaky, generator=gen)

        def device_edit(pdfs=fixed, st=None):
            return path_edit_distance(pdfs, phone_of_pdf, refs, ref_lengths, starts=st)[0]

        def loop_edit(pdfs=fixed):
            return torch.tensor([[edit_distance(phones_of(p, phone_list), ref_lists[b]) for p in pdfs[b].tolist()]
                                 for b in range(S)]).to(dev)

        fixed_risks = device_edit()

        def step(risks_of, fused):
            x = y.detach().requires_grad_(True)
            pdfs = den_sample_paths(x, graph, K, n_batch=S, leaky_hmm_coefficient=leaky, generator=gen)
            sampled_risk_surrogate(x, pdfs, risks_of(pdfs), fused=fused).sum().backward()
            return x.grad

        def surrogate(fused):
            x = y.detach().requires_grad_(True)
            sampled_risk_surrogate(x, fixed, fixed_risks, fused=fused).sum().backward()
            return x.grad

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        quick = {"device_edit": device_edit, "device_edit_start_mode": lambda: device_edit(st=starts),
                 "step_device_torch": lambda: step(device_edit, False), "step_device_fused": lambda: step(device_edit, True),
                 "surrogate_torch": lambda: surrogate(False), "surrogate_fused": lambda: surrogate(True)}
        slow = {"loop_edit": loop_edit, "step_loop_torch": lambda: step(loop_edit, False)}
        assert torch.equal(loop_edit().to(torch.int32), fixed_risks) and int(fixed_risks.min()) >= 0, config
        for _ in range(args.warmup):
            for fn in quick.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in list(quick) + list(slow)}
        for _ in range(args.iters):  # (they take turns)
            for k, fn in quick.items():
                times[k].append(timed(fn))
        for _ in range(args.loop_iters):
            for k, fn in slow.items():
                times[k].append(timed(fn))
        row = dict(config=config, S=S, K=K, T=T, pdfs=P, iters=args.iters, loop_iters=args.loop_iters,
                   mean_ref_tokens=round(float(lengths.mean()), 2),
                   mean_hyp_tokens=round(float(path_edit_distance(fixed, phone_of_pdf, refs, ref_lengths)[1].float().mean()), 2),
                   mean_distance=round(float(fixed_risks.float().mean()), 2))
        for k, v in times.items():
            v = sorted(v)
            row.update({k + "_median_ms": round(v[len(v) // 2], 4), k + "_min_ms": round(v[0], 4),
                        k + "_q1_ms": round(v[len(v) // 4], 4), k + "_q3_ms": round(v[(3 * len(v)) // 4], 4)})
        row["loop_over_device_edit"] = round(row["loop_edit_median_ms"] / row["device_edit_median_ms"], 1)
        row["step_loop_over_step_fused"] = round(row["step_loop_torch_median_ms"] / row["step_device_fused_median_ms"], 2)
        print(json.dumps(row), flush=True)
        del y, fixed


if __name__ == "__main__":
    main()
