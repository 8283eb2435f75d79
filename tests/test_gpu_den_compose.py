"""Supervisions that carry a denominator graph's weights (``io.DenominatorGraph.normalize_fsts``, the constructors'
``den_graph`` argument, ``Supervision.from_alignments``) run on the GPU: the objective's bound, ``chain_loss`` against float64
on the RESTATED composition (``den_compose_reference``), the flat-start hand-over, and the graph left as it was.
B = 5, ragged lengths 7 .. 12, leaky-HMM coefficient 1e-5, l2 = 0.  Cases and references: ``den_compose_cases``.

Tolerances are those of ``test_gpu_ragged_regular.py`` / ``test_gpu_e2e.py``, restated: objective and gradient within
``helpers.REL`` (the gradient matrix-wise on the scale of the supervision's weight), a numerator log-prob within
``num_elementwise_cases.REL_LOGPROB`` of its float64 value."""
import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss

import den_compose_cases as dc
import den_compose_reference as dr
import num_elementwise_cases as nc
from helpers import REL, from3d, rel_err, to3d

pytestmark = pytest.mark.gpu
LENS = dc.LENGTHS
S, T, P = len(LENS), max(LENS), dc.P
KW = dict(l2_regularize=dc.L2, leaky_hmm_coefficient=dc.LEAKY)
BOUND_SEED = 1       # of the bound test's supervisions: with it every float64 objf / T_s below is <= -0.05 (asserted)
MARGIN = -0.05

_graphs = {}


def _graph(name):
    if name not in _graphs:
        _graphs[name] = io.DenominatorGraph(dc.den_fst(name), P).prepare(0)
    return _graphs[name]


def _handle(fsts, e2e, **kw):
    if e2e:
        return io.Supervision.from_e2e_fsts(1.0, list(LENS), P, fsts, **kw)
    return io.Supervision.from_fsts(1.0, list(LENS), P, fsts, **kw)


def _loss(graph, sup, y, grad=False):
    """chain_loss on the (Tmax * S, P) matrix as a (B, C, T) tensor: (loss, results, per-sequence report, -gradient rows)"""
    x = to3d(np.ascontiguousarray(y), S, T, P).requires_grad_(grad)
    loss, res = chain_loss(x, graph, sup, per_sequence=True, **KW)
    g = None
    if grad:
        (gx,) = torch.autograd.grad(loss, x)
        g = -from3d(gx, S, T, P)
    torch.cuda.synchronize()
    return float(loss.detach()), res.data.numpy().copy(), res.per_sequence, g


# ---- the bound ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e2e", [False, True])
def test_normalized_supervisions_bound_the_objective(e2e):
    name = "phone_lm"
    g = _graph(name)
    fsts, paths = dc.bound_batch(name, e2e, BOUND_SEED)
    # the gap: without the graph's weights, outputs that favour the path outside the graph drive the objective above 0
    y = np.zeros((T * S, P), np.float32)
    for s, p in enumerate(paths):
        for t, lab in enumerate(p[2]):
            y[t * S + s, lab - 1] = 8.0
    _, _, seq, _ = _loss(g, _handle(fsts, e2e), y)
    print("un-normalized objf per sequence:", seq.objf.tolist())
    assert seq.status.tolist() == [0] * S and (seq.objf > 0).any()
    # ... with them it stays below 0, for those outputs and for ten draws of y ~ N(0, 1)
    sup = _handle(fsts, e2e, den_graph=g, normalization_scale=1.0)
    restated, status = dr.normalize(g, fsts, e2e=e2e)
    assert status == [0] * S
    for draw in [y] + [dc.nnet_output(1000 + k) for k in range(10)]:
        want = dc.reference(name, restated, LENS, draw, e2e=e2e)
        assert (want["objf"] / np.asarray(LENS) <= MARGIN).all(), want["objf"]  # rounding cannot decide the sign
        loss, _, seq, _ = _loss(g, sup, draw)
        print("objf per sequence %s (float64 %s)" % (seq.objf.tolist(), want["objf"].tolist()))
        assert np.isfinite(loss) and seq.status.tolist() == [0] * S
        assert (seq.objf < 0).all()


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
def _oracle_batch(name, e2e, seed):
    """Supervisions with arc and final costs of their own: unions of label paths (two in the graph, one outside), or
    end-to-end acceptors with self-loops and cycles cut out of the graph plus arcs it does not have."""
    rng = np.random.default_rng(seed)
    fst = dc.den_fst(name)
    if e2e:
        return [dc.e2e_fst(fst, rng, n=6, junk=3) for _ in LENS]
    return [dc.regular_fst(fst, rng, T=Ts, in_graph=2, junk=1)[0] for Ts in LENS]


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("name,e2e", [("random", False), ("phone_lm", False), ("random", True), ("phone_lm", True)])
def test_chain_loss_matches_float64_on_the_restated_composition(name, e2e, scale):
    g = _graph(name)
    fsts = _oracle_batch(name, e2e, seed=7 + e2e)
    restated, status = dr.normalize(g, fsts, e2e=e2e, scale=scale)
    assert status == [0] * S
    y = dc.nnet_output(77)
    want = dc.reference(name, restated, LENS, y, e2e=e2e)
    sup = _handle(fsts, e2e, den_graph=g, normalization_scale=scale)
    assert sup.is_e2e == e2e and list(sup.frames) == list(LENS)
    loss, r, seq, grad = _loss(g, sup, y, grad=True)
    print("%s e2e=%d scale=%g: objf %.9g (float64 %.9g), gradient rel %.2e, num_logprob rel %s" % (
        name, e2e, scale, r[0], want["total"], rel_err(grad, want["deriv"], floor=1.0),
        (np.abs(seq.num_logprob.numpy() - want["num_logprob"]) / np.abs(want["num_logprob"])).tolist()))
    assert seq.status.tolist() == [0] * S
    assert abs(r[0] - want["total"]) <= REL * abs(want["total"])
    assert r[2] == np.float32(sum(LENS))
    assert (np.abs(seq.objf.numpy() - want["objf"]) <= REL * np.abs(want["objf"])).all()
    assert (np.abs(seq.num_logprob.numpy() - want["num_logprob"]) <= nc.REL_LOGPROB * np.abs(want["num_logprob"])).all()
    assert rel_err(grad, want["deriv"], floor=1.0) <= REL
    pad = (np.arange(T)[:, None] >= np.asarray(LENS)[None, :]).reshape(T * S)
    assert not grad[pad].any()
    assert abs(loss + r[0] / r[2]) <= 1e-6 * abs(loss)


# ---- the flat-start hand-over ---------------------------------------------------------------------------------------------------
def test_flat_start_alignments_become_regular_supervisions():
    name = "phone_lm"
    g = _graph(name)
    fsts = _oracle_batch(name, True, seed=17)
    e2e = _handle(fsts, True, den_graph=g)
    y = dc.nnet_output(78, scale=2.0)
    x = to3d(y, S, T, P)
    pdfs, scores = e2e.best_path(x)
    torch.cuda.synchronize()
    ali = pdfs.cpu().numpy()
    assert np.isfinite(scores.cpu().numpy()).all()
    for s, Ts in enumerate(LENS):
        assert (ali[s, :Ts] >= 0).all() and (ali[s, Ts:] == -1).all()
    sup = io.Supervision.from_alignments(1.0, pdfs, P, den_graph=g)
    assert not sup.is_e2e and sup.is_ragged and list(sup.frames) == list(LENS)
    linear = [dr.union_of_paths([[int(p) + 1 for p in ali[s, :Ts]]]) for s, Ts in enumerate(LENS)]
    restated, status = dr.normalize(g, linear)
    assert status == [0] * S
    want = dc.reference(name, restated, LENS, y)
    assert (want["objf"] / np.asarray(LENS) <= MARGIN).all(), want["objf"]
    loss, r, seq, _ = _loss(g, sup, y)
    print("objf per sequence %s (float64 %s)" % (seq.objf.tolist(), want["objf"].tolist()))
    assert np.isfinite(loss) and seq.status.tolist() == [0] * S and (seq.objf < 0).all()
    assert (np.abs(seq.objf.numpy() - want["objf"]) <= REL * np.abs(want["objf"])).all()
    again, _ = sup.best_path(x)
    assert torch.equal(again, pdfs)
    # a sequence without a path of its length: best_path gives -1s, from_alignments names it
    broken = list(fsts)
    broken[3] = (0,) + dr.union_of_paths([dr.graph_path(dc.den_fst(name), LENS[3] + 1, np.random.default_rng(1))])
    pdfs, scores = _handle(broken, True).best_path(x)
    assert (pdfs[3] == -1).all() and scores[3].item() == float("-inf")
    with pytest.raises(ValueError, match=r"\[3\]"):
        io.Supervision.from_alignments(1.0, pdfs, P, frames=list(LENS), den_graph=g)


# ---- the graph is untouched -----------------------------------------------------------------------------------------------------
def test_a_training_step_gives_the_same_bits_after_normalize_fsts():
    fst = dc.den_fst("random")
    g = io.DenominatorGraph(fst, P).prepare(0)
    sup = synth.random_supervision(fst, 4, 9, 3, seed=3)
    y = synth.random_nnet_output(4, 9, P, seed=4)

    def step():
        x = to3d(y, 4, 9, P).requires_grad_(True)
        loss, res = chain_loss(x, g, io.Supervision.from_synth(sup), **KW)
        (gx,) = torch.autograd.grad(loss, x)
        torch.cuda.synchronize()
        return loss.detach().cpu().numpy().view(np.int32), res.data.numpy().view(np.int32).copy(), gx.cpu().numpy().view(np.int32)

    before, h = step(), int(lib.tc_den_graph_hash(g.ptr))
    outs, info = g.normalize_fsts([dr.strip_weights(synth.random_supervision(fst, 1, 9, 3, seed=5))])
    assert info["status"][0] == 0
    after = step()
    assert int(lib.tc_den_graph_hash(g.ptr)) == h
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
