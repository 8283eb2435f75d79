"""Boosted LF-MMI on the host: what the boost means path by path, that the two CPU compositions of
``boost_reference`` agree, the hard form as the dense form on the indicator, the shift by a constant accuracy, and that
``chain_loss`` refuses what it must before the library is touched.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import independent_f64 as ind
from torchain_amd import functions, io, synth

import boost_reference as br
from helpers import REL, rel_err


def _tiny_graph(seed):
    fst = synth.random_den_fst(4, 2, 3, seed=seed)
    return fst, synth.initial_probs_f64(fst)


@pytest.mark.parametrize("form", ["hard_classes", "dense"])
def test_boost_reweights_every_path_by_its_accuracy(form):
    """den_logprob(y - b * a) == log sum_paths exp(score(path) - b * A(path)), enumerated: 4 states, T = 4, leaky 0."""
    fst, pi = _tiny_graph(3)
    T, P, b = 4, fst.num_pdfs, 0.75
    rng = np.random.default_rng(5)
    y = rng.normal(size=(T, P))
    if form == "dense":
        a = rng.normal(size=(T, P))
    else:
        a = br.indicator(np.array([[0, 2, -1, 1]]), np.array([0, 1, 0]), P).astype(np.float64)
        assert a.sum() == 2 + 2 + 0 + 1  # (classes {0, 2} and {1}; the third frame scores nothing)
    want = br.enumerate_den_logprob(fst, pi, y, a, b)
    with np.errstate(divide="ignore"):
        got = float(ind.den_logprob(fst, pi, torch.from_numpy(y - b * a), 1, 0.0))
        plain = float(ind.den_logprob(fst, pi, torch.from_numpy(y), 1, 0.0))
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (got, want)
    assert abs(plain - br.enumerate_den_logprob(fst, pi, y, a, 0.0)) <= 1e-12 * max(1.0, abs(plain))
    assert abs(got - plain) > 1e-3  # (the boost did something on this case)


def test_the_float64_reference_is_the_enumeration():
    """boost_reference.float64 / boosted themselves, which every GPU comparison leans on: their boosted denominator is the
    enumerated sum.  y on a grid of 2^-10, a on a grid of 1/4 and b = 0.75 keep the two float32 roundings exact, so 1e-12
    holds; the leaky coefficient is 0 as in the enumeration."""
    fst, pi = _tiny_graph(3)
    T, P, b = 4, fst.num_pdfs, 0.75
    rng = np.random.default_rng(8)
    y = (np.round(rng.normal(size=(T, P)) * 1024.0) / 1024.0).astype(np.float32)
    a = (rng.integers(-4, 9, size=(T, P)) / 4.0).astype(np.float32)
    sup = synth.random_supervision(fst, 1, T, 2, seed=4, initial_probs=pi)
    assert np.array_equal(br.boosted(y, b, a).astype(np.float64), y.astype(np.float64) - b * a.astype(np.float64))
    with np.errstate(divide="ignore"):
        got = br.float64(fst, pi, sup, y, b, a, l2=0.0, leaky=0.0)
        plain = br.float64(fst, pi, sup, y, 0.0, a, l2=0.0, leaky=0.0)
    want = br.enumerate_den_logprob(fst, pi, y, a, b)
    assert abs(got["den"] - want) <= 1e-12 * max(1.0, abs(want)), (got["den"], want)
    assert got["num"] == plain["num"] and abs(got["den"] - plain["den"]) > 1e-3  # (the numerator never sees the boost)
    assert abs(got["objf"] - float(sup.weight) * (got["num"] - want)) <= 1e-12 * max(1.0, abs(want))


def _workload(S=3, T=7, seed=2, weight=0.7):
    fst = synth.random_den_fst(30, 3, 12, seed=seed)
    pi = synth.initial_probs_f64(fst)
    sup = synth.random_supervision(fst, S, T, 2, seed=seed + 1, weight=weight, initial_probs=pi)
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=seed + 2)
    return fst, pi, sup, y


def test_the_two_cpu_compositions_agree(oracle):
    fst, pi, sup, y = _workload()
    S, T, P = 3, 7, fst.num_pdfs
    rng = np.random.default_rng(9)
    ref = rng.integers(-1, P, size=(S, T))
    cases = [br.indicator(ref, rng.integers(0, 4, size=P), P), rng.random(size=(S * T, P)).astype(np.float32)]
    graph = oracle.DenGraph(fst)
    for a in cases:
        for l2 in (0.0, 5e-5):
            f64 = br.float64(fst, graph.initial_probs(), sup, y, 1.5, a, l2=l2, leaky=0.05)
            o32 = br.oracle32(oracle, graph, sup, y, 1.5, a, l2=l2, leaky=0.05)
            assert o32["ok"]
            assert abs(o32["objf"] - f64["objf"]) <= REL * abs(f64["objf"])
            assert abs(o32["l2_term"] - f64["l2_term"]) <= REL * abs(f64["l2_term"]) + 1e-30
            assert o32["weight"] == f64["weight"]
            assert rel_err(o32["deriv"], f64["deriv"], floor=sup.weight) <= REL
            assert rel_err(o32["xent_deriv"], f64["xent_deriv"], floor=sup.weight) <= REL


def test_hard_form_is_the_dense_form_on_the_indicator_bit_for_bit():
    S, T, P, b = 3, 5, 11, np.float32(1.3)
    rng = np.random.default_rng(1)
    y = rng.normal(size=(S * T, P)).astype(np.float32)
    y[0, 0] = -0.0
    ref = rng.integers(-2, P + 2, size=(S, T))
    cls = rng.integers(0, 3, size=P)
    for c in (None, cls):
        a = br.indicator(ref, c, P)
        dense = br.boosted(y, b, a)
        hard = y.copy()  # the statement element by element: a hit loses fl32(b * 1), everything else is y32 itself
        for s in range(S):
            for t in range(T):
                r = int(ref[s, t])
                if 0 <= r < P:
                    hits = np.arange(P) == r if c is None else c == c[r]
                    hard[t * S + s, hits] = (y[t * S + s, hits] - b).astype(np.float32)
        keep = a == 0
        assert np.array_equal(dense.view(np.int32), hard.view(np.int32))
        assert np.array_equal(dense[keep].view(np.int32), y[keep].view(np.int32))  # (y32 itself, a zero's sign included)
        assert a.sum() > 0 and keep.sum() > 0


def test_constant_accuracy_shifts_the_objective_and_nothing_else():
    """a == 1 everywhere: every path loses b * T, so objf rises by w * b * sum(T_s) and the gradient is unchanged.  y on a
    grid of 2^-10 and b = 0.5 keep the float32 subtraction exact, so float64 agrees to 1e-10."""
    fst, pi, sup, y = _workload(S=2, T=6, seed=4, weight=0.5)
    y = (np.round(y * 1024.0) / 1024.0).astype(np.float32)
    b, w = 0.5, 0.5
    ones = np.ones_like(y)
    assert np.array_equal(br.boosted(y, b, ones).astype(np.float64), y.astype(np.float64) - b)
    plain = br.float64(fst, pi, sup, y, 0.0, ones, l2=5e-5, leaky=0.1)
    shifted = br.float64(fst, pi, sup, y, b, ones, l2=5e-5, leaky=0.1)
    assert abs(shifted["objf"] - (plain["objf"] + w * b * 2 * 6)) <= 1e-10
    assert np.abs(shifted["deriv"] - plain["deriv"]).max() <= 1e-10
    assert shifted["l2_term"] == plain["l2_term"]


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched: %s" % name)


def test_chain_loss_refuses_before_the_library_is_touched(monkeypatch):
    fst = synth.random_den_fst(20, 3, 8, seed=1)
    S, T, P = 2, 5, 8
    den = io.DenominatorGraph(fst, P)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 2, seed=2))
    assert (sup.n_batch, sup.n_frame, sup.n_pdf) == (S, T, P)
    monkeypatch.setattr(functions, "lib", _Untouchable())
    monkeypatch.setattr(functions, "_run_step", lambda *a, **k: pytest.fail("the step was reached"))
    x = torch.zeros(S, P, T, requires_grad=True)
    ref = torch.zeros(S, T, dtype=torch.int64)
    acc = torch.zeros(S * T, P)
    bad = [
        dict(boost=float("nan"), boost_ref=ref),
        dict(boost=float("inf"), boost_ref=ref),
        dict(boost="much", boost_ref=ref),
        dict(boost=True, boost_ref=ref),
        dict(boost=1.0, boost_ref=ref, boost_accuracy=acc),                       # both
        dict(boost=1.0, boost_ref=ref.float()),                                   # dtype
        dict(boost=1.0, boost_ref=ref[:, :-1]),                                   # shape
        dict(boost=1.0, boost_ref=[[0] * T] * S),                                 # not a tensor
        dict(boost=1.0, boost_ref=ref, boost_pdf_class=torch.zeros(P + 1, dtype=torch.int32)),
        dict(boost=1.0, boost_ref=ref, boost_pdf_class=torch.zeros(P)),
        dict(boost=1.0, boost_accuracy=acc, boost_pdf_class=torch.zeros(P, dtype=torch.int32)),
        dict(boost=1.0, boost_accuracy=acc.double()),
        dict(boost=1.0, boost_accuracy=acc[:-1]),
        dict(boost=1.0, boost_accuracy=torch.zeros(P, S * T).t()),                # column stride
        dict(boost=1.0, boost_accuracy=acc.clone().requires_grad_(True)),
        dict(boost=1.0, boost_ref=ref.to("meta")),                                # another device
        dict(boost=1.0, boost_ref=ref, xent_regularize=0.1, xent_input=torch.zeros(S, P, T), kaldi_way=False),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            functions.chain_loss(x, den, sup, **kw)
    with pytest.raises(TypeError):
        functions.chain_loss(x, den, sup, boost_reference=ref)
