"""Launch census of the training step: what one ``chain_loss`` (plus ``backward``) enqueues, as the change of every
``tc_debug_counter`` key, for layout x dtype x cross-entropy branch x mode.  The table is the structural statement of "the same
launches": a change to the step's host code that adds, drops or re-routes a pass moves a count.  It uses nothing but
``chain_loss`` and ``tc_debug_counter``, so the same file runs on any earlier commit that has both.

Shapes: P = 20, B = 3, T = 5.  The supervision has been used before the census starts, so the staging pool's counters stand
still unless a step stages again."""
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, B, T = 20, 3, 5
KEYS = ("den_launches", "den_backward_launches", "num_launches", "num_backward_launches", "layout_launches",
        "den_long_utterance_launches", "num_e2e_staged_launches", "num_windowed_launches", "channel_last_steps",
        "pool_device_allocs", "pool_reuses")
LAYOUTS = ("rows", "padded rows", "bct", "batch-first", "time-major")
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}
XENT = {"no xent": None, "kaldi way": True, "reference way": False}
MODES = ("train", "train, weights and penalty", "eval")

# (layout, dtype, xent, mode) -> the change of each of KEYS, in that order
EXPECTED = {
    ('rows', 'float32', 'no xent', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'float32', 'no xent', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'float32', 'no xent', 'eval'): (1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'float32', 'kaldi way', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'float32', 'kaldi way', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'float32', 'kaldi way', 'eval'): (1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'float32', 'reference way', 'train'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'float32', 'reference way', 'train, weights and penalty'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'float32', 'reference way', 'eval'): (1, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'bfloat16', 'no xent', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'bfloat16', 'no xent', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'bfloat16', 'no xent', 'eval'): (1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'bfloat16', 'kaldi way', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'bfloat16', 'kaldi way', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'bfloat16', 'kaldi way', 'eval'): (1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'bfloat16', 'reference way', 'train'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'bfloat16', 'reference way', 'train, weights and penalty'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('rows', 'bfloat16', 'reference way', 'eval'): (1, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'float32', 'no xent', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'float32', 'no xent', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'float32', 'no xent', 'eval'): (1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'float32', 'kaldi way', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'float32', 'kaldi way', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'float32', 'kaldi way', 'eval'): (1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'float32', 'reference way', 'train'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'float32', 'reference way', 'train, weights and penalty'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'float32', 'reference way', 'eval'): (1, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'bfloat16', 'no xent', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'bfloat16', 'no xent', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'bfloat16', 'no xent', 'eval'): (1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'bfloat16', 'kaldi way', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'bfloat16', 'kaldi way', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'bfloat16', 'kaldi way', 'eval'): (1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'bfloat16', 'reference way', 'train'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'bfloat16', 'reference way', 'train, weights and penalty'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('padded rows', 'bfloat16', 'reference way', 'eval'): (1, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0),
    ('bct', 'float32', 'no xent', 'train'): (1, 1, 1, 1, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'float32', 'no xent', 'train, weights and penalty'): (1, 1, 1, 1, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'float32', 'no xent', 'eval'): (1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0),
    ('bct', 'float32', 'kaldi way', 'train'): (1, 1, 1, 1, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'float32', 'kaldi way', 'train, weights and penalty'): (1, 1, 1, 1, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'float32', 'kaldi way', 'eval'): (1, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0),
    ('bct', 'float32', 'reference way', 'train'): (1, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'float32', 'reference way', 'train, weights and penalty'): (1, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'float32', 'reference way', 'eval'): (1, 0, 2, 1, 1, 0, 0, 0, 0, 0, 0),
    ('bct', 'bfloat16', 'no xent', 'train'): (1, 1, 1, 1, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'bfloat16', 'no xent', 'train, weights and penalty'): (1, 1, 1, 1, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'bfloat16', 'no xent', 'eval'): (1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0),
    ('bct', 'bfloat16', 'kaldi way', 'train'): (1, 1, 1, 1, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'bfloat16', 'kaldi way', 'train, weights and penalty'): (1, 1, 1, 1, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'bfloat16', 'kaldi way', 'eval'): (1, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0),
    ('bct', 'bfloat16', 'reference way', 'train'): (1, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'bfloat16', 'reference way', 'train, weights and penalty'): (1, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0),
    ('bct', 'bfloat16', 'reference way', 'eval'): (1, 0, 2, 1, 1, 0, 0, 0, 0, 0, 0),
    ('batch-first', 'float32', 'no xent', 'train'): (1, 1, 1, 1, 2, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'float32', 'no xent', 'train, weights and penalty'): (1, 1, 1, 1, 2, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'float32', 'no xent', 'eval'): (1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'float32', 'kaldi way', 'train'): (1, 1, 1, 1, 4, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'float32', 'kaldi way', 'train, weights and penalty'): (1, 1, 1, 1, 4, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'float32', 'kaldi way', 'eval'): (1, 0, 1, 1, 2, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'float32', 'reference way', 'train'): (1, 1, 2, 2, 4, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'float32', 'reference way', 'train, weights and penalty'): (1, 1, 2, 2, 4, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'float32', 'reference way', 'eval'): (1, 0, 2, 1, 2, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'bfloat16', 'no xent', 'train'): (1, 1, 1, 1, 2, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'bfloat16', 'no xent', 'train, weights and penalty'): (1, 1, 1, 1, 2, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'bfloat16', 'no xent', 'eval'): (1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'bfloat16', 'kaldi way', 'train'): (1, 1, 1, 1, 4, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'bfloat16', 'kaldi way', 'train, weights and penalty'): (1, 1, 1, 1, 4, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'bfloat16', 'kaldi way', 'eval'): (1, 0, 1, 1, 2, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'bfloat16', 'reference way', 'train'): (1, 1, 2, 2, 4, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'bfloat16', 'reference way', 'train, weights and penalty'): (1, 1, 2, 2, 4, 0, 0, 0, 1, 0, 0),
    ('batch-first', 'bfloat16', 'reference way', 'eval'): (1, 0, 2, 1, 2, 0, 0, 0, 1, 0, 0),
    ('time-major', 'float32', 'no xent', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'float32', 'no xent', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'float32', 'no xent', 'eval'): (1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'float32', 'kaldi way', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'float32', 'kaldi way', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'float32', 'kaldi way', 'eval'): (1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'float32', 'reference way', 'train'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'float32', 'reference way', 'train, weights and penalty'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'float32', 'reference way', 'eval'): (1, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'bfloat16', 'no xent', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'bfloat16', 'no xent', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'bfloat16', 'no xent', 'eval'): (1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'bfloat16', 'kaldi way', 'train'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'bfloat16', 'kaldi way', 'train, weights and penalty'): (1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'bfloat16', 'kaldi way', 'eval'): (1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'bfloat16', 'reference way', 'train'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'bfloat16', 'reference way', 'train, weights and penalty'): (1, 1, 2, 2, 0, 0, 0, 0, 0, 0, 0),
    ('time-major', 'bfloat16', 'reference way', 'eval'): (1, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0),
}


def _leaf(rows, layout, dtype):
    rows = rows.to(dtype)
    if layout == "rows":
        return rows.clone()
    if layout == "padded rows":
        wide = torch.zeros(T * B, P + 4, dtype=dtype, device=DEV)
        wide[:, :P] = rows
        return wide[:, :P]
    tbp = rows.view(T, B, P)
    if layout == "bct":
        return tbp.permute(1, 2, 0).contiguous()
    if layout == "batch-first":
        return tbp.permute(1, 0, 2).contiguous().transpose(1, 2)  # (B, T, C) seen as (B, C, T)
    assert layout == "time-major", layout
    return tbp.contiguous().permute(1, 2, 0)                      # (T, B, C) seen as (B, C, T)


def _counters():
    return [int(lib.tc_debug_counter(k.encode())) for k in KEYS]


def census():
    fst = synth.random_den_fst(40, 4, P, seed=6)
    graph = io.DenominatorGraph(fst, P).prepare(DEV)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, B, T, 2, seed=1))
    y = torch.from_numpy(synth.random_nnet_output(B, T, P, seed=1)).to(DEV)
    xe = torch.from_numpy(synth.random_nnet_output(B, T, P, seed=2)).to(DEV)
    w = torch.linspace(0.5, 1.5, T * B, device=DEV)
    chain_loss(y.clone().requires_grad_(True), graph, sup, 5e-4, 0.05)[0].backward()  # (stages the supervision)
    torch.cuda.synchronize()
    table = {}
    for layout in LAYOUTS:
        for dname, dtype in DTYPES.items():
            for xname, kaldi_way in XENT.items():
                for mode in MODES:
                    grad = mode != "eval"
                    x = _leaf(y, layout, dtype).requires_grad_(grad)
                    kw = dict(l2_regularize=5e-4, leaky_hmm_coefficient=0.05)
                    if kaldi_way is not None:
                        kw.update(xent_regularize=0.1, xent_input=_leaf(xe, layout, dtype).requires_grad_(grad), kaldi_way=kaldi_way)
                    if mode == "train, weights and penalty":
                        kw.update(deriv_weights=w, out_of_range_regularize=0.25)
                    before = _counters()
                    with torch.set_grad_enabled(grad):
                        loss, _ = chain_loss(x, graph, sup, **kw)
                    if grad:
                        loss.backward()
                    table[(layout, dname, xname, mode)] = tuple(b - a for a, b in zip(before, _counters()))
    torch.cuda.synchronize()
    return table


def test_launch_census():
    got = census()
    assert len(got) == len(LAYOUTS) * len(DTYPES) * len(XENT) * len(MODES) == 90
    wrong = {k: (got[k], EXPECTED.get(k)) for k in got if got[k] != EXPECTED.get(k)}
    assert not wrong, "\n".join("%s: got %s, expected %s" % (k, v[0], v[1]) for k, v in sorted(wrong.items()))
    assert set(EXPECTED) == set(got)
