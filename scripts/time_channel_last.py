"""What a channel-last network output costs ``chain_loss``: the training step (``chain_loss`` + backward through a leaf) at
C3's shape (256 x 150 x 4096) on C3's denominator graph, float32 and bfloat16, without and with the cross-entropy branch
(``kaldi_way=True``), for five forms of the same values:

    bct          contiguous (B, C, T), the reference's layout
    rows         2-D frame-major (T*B, C)
    batch_first  (B, T, C).transpose(1, 2): a batch-first LSTM / Transformer output
    joint_head   the halves of one (B, T, 2C) leaf: [..., :C] is the chain output, [..., C:] the xent output
    time_major   (T, B, C).permute(1, 2, 0): PyTorch's default recurrent layout

and two kinds of child process, taking turns, ``--rounds`` of each: ``parent`` (another checkout of this repository,
``--parent-root``, built there: it runs the same Python calls through its fallback routes) and ``this``.  Two builds of the
library cannot share a process, hence the children; the process that starts them never opens the GPU.  It prints per case and
kind the median over the rounds of each round's median and the spread (max - min) of the rounds' medians -- the spread of
``parent`` is the run-to-run noise -- and compares the SHA-1 of every case's gradients (in (B, C, T) order) between the kinds.

    python scripts/time_channel_last.py [--parent-root DIR] [--rounds 3] [--iters 20] [--warmup 5] [--only form,form]
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = ("bct", "rows", "batch_first", "joint_head", "time_major")
FIELDS = ("weight", "num_sequences", "frames_per_sequence", "label_dim", "num_states", "arc_begin", "ilabel", "arc_weight",
          "nextstate", "final")


def make_supervision(config, path):
    sys.path.insert(0, os.path.join(HERE, ".."))
    from torchain_amd import synth
    cfg = synth.CONFIGS[config]
    sup = synth.random_supervision(synth.config_den_fst(config), cfg["S"], cfg["T"], 3, seed=3)
    np.savez_compressed(path, **dict(zip(FIELDS, sup)))


def child(args):
    sys.path.insert(0, args.root)
    import torch

    from torchain_amd import io, synth
    from torchain_amd.functions import chain_loss

    cfg = synth.CONFIGS[args.config]
    S, T, P = cfg["S"], cfg["T"], cfg["P"]
    dev = "cuda:0"
    graph = io.DenominatorGraph(synth.config_den_fst(args.config), P).prepare(dev)
    own_tmp = None
    if args.supervision is None:  # (a child started by hand, e.g. under a profiler)
        own_tmp = tempfile.mkdtemp(prefix="time_channel_last_")
        args.supervision = os.path.join(own_tmp, "supervision.npz")
        make_supervision(args.config, args.supervision)
    with np.load(args.supervision) as z:
        sup = io.Supervision.from_synth(synth.SupFst(float(z["weight"]), int(z["num_sequences"]), int(z["frames_per_sequence"]),
                                                     int(z["label_dim"]), int(z["num_states"]), z["arc_begin"], z["ilabel"],
                                                     z["arc_weight"], z["nextstate"], z["final"]))
    if own_tmp:
        shutil.rmtree(own_tmp, ignore_errors=True)
    gen = torch.Generator(device=dev).manual_seed(4)
    y_btc = torch.randn(S, T, P, device=dev, generator=gen)           # the values, batch-first
    xe_btc = torch.log_softmax(torch.randn(S, T, P, device=dev, generator=gen), dim=2)

    def build(form, dtype, xent):
        """(input, xent_input or None, leaves, grads()): grads() -> the gradients in (B, C, T) order, contiguous"""
        a, b = y_btc.to(dtype), xe_btc.to(dtype)
        if form == "joint_head":
            leaf = torch.cat([a, b], dim=2).requires_grad_(True)
            x, xe = leaf[..., :P].transpose(1, 2), leaf[..., P:].transpose(1, 2)
            return x, (xe if xent else None), [leaf], lambda: [leaf.grad[..., :P].transpose(1, 2)] + ([leaf.grad[..., P:].transpose(1, 2)] if xent else [])
        view = {"bct": lambda t: t.transpose(1, 2).contiguous(), "rows": lambda t: t.transpose(0, 1).reshape(T * S, P).contiguous(),
                "batch_first": lambda t: t.clone(), "time_major": lambda t: t.transpose(0, 1).contiguous()}[form]
        back = {"bct": lambda g: g, "rows": lambda g: g.view(T, S, P).permute(1, 2, 0), "batch_first": lambda g: g.transpose(1, 2),
                "time_major": lambda g: g.permute(1, 2, 0)}[form]
        use = {"bct": lambda t: t, "rows": lambda t: t, "batch_first": lambda t: t.transpose(1, 2),
               "time_major": lambda t: t.permute(1, 2, 0)}[form]
        leaves = [view(a).requires_grad_(True)] + ([view(b).requires_grad_(True)] if xent else [])
        return use(leaves[0]), (use(leaves[1]) if xent else None), leaves, lambda: [back(t.grad) for t in leaves]

    forms = [f for f in FORMS if not args.only or f in args.only.split(",")]
    for dtype in (torch.float32, torch.bfloat16):
        for xent in (False, True):
            for form in forms:
                x, xe, leaves, grads = build(form, dtype, xent)
                kw = dict(l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"])
                if xent:
                    kw.update(xent_regularize=0.1, xent_input=xe, kaldi_way=True)

                def step():
                    for t in leaves:
                        t.grad = None
                    loss, _ = chain_loss(x, graph, sup, **kw)
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
                row = dict(config=args.config, kind=args.kind, dtype=str(dtype).split(".")[1], xent=xent, form=form,
                           iters=args.iters, median_ms=round(times[len(times) // 2], 4), min_ms=round(times[0], 4))
                if args.hash:
                    h = hashlib.sha1()
                    for g in grads():
                        h.update(g.contiguous().view(torch.int16 if dtype == torch.bfloat16 else torch.int32).cpu().numpy().tobytes())
                    row["grad_sha1"] = h.hexdigest()
                print(json.dumps(row), flush=True)
                del x, xe, leaves, grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated forms (default: all five)")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit to compare with (kind 'parent')")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kind", default="this", help=argparse.SUPPRESS)
    ap.add_argument("--hash", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--supervision", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.join(HERE, ".."), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    this = os.path.abspath(args.root)
    tmp = tempfile.mkdtemp(prefix="time_channel_last_")
    try:
        report(args, this, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def report(args, this, tmp):
    sup_path = os.path.join(tmp, "supervision.npz")
    make_supervision(args.config, sup_path)
    roots = ([("parent", os.path.abspath(args.parent_root))] if args.parent_root else []) + [("this", this)]
    rows, hashes = {}, {}
    for rnd in range(args.rounds):
        for kind, root in roots:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--kind", kind, "--root", root, "--config", args.config,
                   "--iters", str(args.iters), "--warmup", str(args.warmup), "--supervision", sup_path, "--only", args.only]
            cmd += ["--hash"] if rnd == 0 else []
            # (a child that fails or hangs ends the run: nothing more is started on the GPU behind it)
            out = subprocess.run(cmd, check=True, timeout=args.timeout, stdout=subprocess.PIPE, text=True, cwd=root).stdout
            for line in out.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    r["round"] = rnd
                    print(json.dumps(r), flush=True)
                    key = (r["dtype"], r["xent"], r["form"])
                    rows.setdefault(key + (kind,), []).append(r["median_ms"])
                    if "grad_sha1" in r:
                        hashes[key + (kind,)] = r["grad_sha1"]
    print("# dtype xent form kind: median over %d rounds of the rounds' medians (ms), spread max - min" % args.rounds)
    for key, v in sorted(rows.items()):
        s = sorted(v)
        print("# %-8s %-5s %-11s %-6s %.3f  spread %.3f  %s" % (key[0], key[1], key[2], key[3], s[len(s) // 2], s[-1] - s[0],
                                                                " ".join("%.3f" % x for x in v)))
    print("# gradients (SHA-1 of the bytes in (B, C, T) order):")
    for (dtype, xent, form, kind), h in sorted(hashes.items()):
        if kind != "this":
            continue
        line = "# %-8s %-5s %-11s" % (dtype, xent, form)
        ref = hashes.get((dtype, xent, "bct", "this"))
        line += "  this == this bct: %s" % ("identical" if h == ref else "DIFFERENT")
        if (dtype, xent, form, "parent") in hashes:
            line += "  this == parent: %s" % ("identical" if h == hashes[(dtype, xent, form, "parent")] else "DIFFERENT")
        print(line)


if __name__ == "__main__":
    main()
