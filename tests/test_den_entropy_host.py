"""The entropy of the denominator graph's path posterior, without a GPU: the float64 autograd reference of
``tests/den_entropy_reference.py`` (what the GPU tests compare with) against ``-sum P log P`` over an explicit enumeration of
every latent path of a 3-state graph, and the checks the library and the wrapper make before any device call."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib

import den_entropy_reference as der

TC_ERR_INVALID_ARGUMENT = -1
TC_ERR_WORKSPACE = -4


def _enumerate(arcs, pi, y, leaky):
    """(entropy, log Z) of one sequence, ``y`` ``(T, P)``: every latent path -- a start state, at every level no leak or a
    leak into any state of positive pi (into the state it left, too), at every frame an arc -- with its weight."""
    src, dst, pdf, prob = arcs
    H, T = len(pi), y.shape[0]
    steps = [(None, 1.0)] + [(h, leaky * pi[h]) for h in range(H) if pi[h] > 0]  # a level's choices: post state, lambda
    weights = []

    def walk(state, t, w):
        for post, lam in steps:
            here, v = (state if post is None else post), w * lam
            if t == T:
                weights.append(v)
                continue
            for a in np.flatnonzero(src == here):
                walk(int(dst[a]), t + 1, v * prob[a] * np.exp(y[t, pdf[a]]))

    for h in range(H):
        if pi[h] > 0:
            walk(h, 0, pi[h])
    w = np.asarray(weights)
    p = w / w.sum()
    return -(p * np.log(p)).sum(), np.log(w.sum())


@pytest.mark.parametrize("leaky,T", itertools.product((1e-5, 0.2), (1, 2, 3)))
def test_reference_against_every_latent_path(leaky, T):
    fst = synth.random_den_fst(3, 2, 4, seed=5)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    arcs, pi = graph.arcs(), graph.initial_probs().astype(np.float64)
    S, lens = 2, (T, max(T - 1, 1))
    y = np.random.default_rng(T).normal(0.0, 2.0, size=(T * S, fst.num_pdfs))
    got = der.path_entropy(arcs, pi, y, S, leaky, frames=lens)
    for s in range(S):
        h, logz = _enumerate([np.asarray(a) for a in arcs], pi, y[s::S][:lens[s]], leaky)
        assert abs(got["entropy"][s] - h) <= 1e-10 and abs(got["logprob"][s] - logz) <= 1e-10
        assert h > 0.1  # (the comparison is of something)
    # the gradient: central differences of the enumerated entropy in two elements of sequence 0, and 0 in padding rows
    for t, j in ((0, 1), (T - 1, 3)):
        e = np.zeros_like(y)
        e[t * S, j] = 1e-5
        slope = (_enumerate([np.asarray(a) for a in arcs], pi, (y + e)[0::S][:T], leaky)[0]
                 - _enumerate([np.asarray(a) for a in arcs], pi, (y - e)[0::S][:T], leaky)[0]) / 2e-5
        assert abs(got["grad"][t * S, j] - slope) <= 1e-8
    assert not got["grad"].reshape(T, S, -1)[lens[1]:, 1].any()


def test_entry_is_exported_and_checks_its_arguments():
    fst = synth.random_den_fst(60, 4, 30, seed=21)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    S, T, P = 2, 7, fst.num_pdfs
    need, need_grad = (int(lib.tc_den_path_entropy_workspace_bytes(graph.ptr, S, T, g)) for g in (0, 1))
    assert 0 < need < need_grad and lib.tc_den_path_entropy_workspace_bytes(None, S, T, 0) == TC_ERR_INVALID_ARGUMENT
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails before a device call
    before = int(lib.tc_debug_counter(b"den_entropy_launches"))
    assert before >= 0 and int(lib.tc_debug_counter(b"den_entropy_streamed_launches")) >= 0

    def call(g=graph.ptr, s=S, y=fake, rows=S * T, cols=P, stride=P, fr=None, t=T, leaky=1e-5, ent=fake, lp=fake, grad=fake,
             gs=P, sc=None, ws=fake, nbytes=need_grad):
        return lib.tc_den_path_entropy(g, s, y, rows, cols, stride, fr, t, leaky, ent, lp, grad, gs, sc, ws, nbytes, 0, None)

    for bad in (dict(g=None), dict(y=None), dict(ent=None), dict(lp=None), dict(s=0), dict(t=0), dict(rows=S * T + 1),
                dict(cols=P + 1), dict(stride=P - 1), dict(gs=P - 1), dict(grad=None, sc=fake), dict(leaky=-0.5),
                dict(leaky=float("inf")), dict(fr=C.c_void_p(4098)), dict(ent=C.c_void_p(4100)), dict(sc=C.c_void_p(4098))):
        assert call(**bad) == TC_ERR_INVALID_ARGUMENT, bad
    for bad in (dict(ws=None), dict(ws=C.c_void_p(4100)), dict(nbytes=need_grad - 1), dict(grad=None, nbytes=need - 1)):
        assert call(**bad) == TC_ERR_WORKSPACE, bad
    assert int(lib.tc_debug_counter(b"den_entropy_launches")) == before  # nothing was launched
    assert lib.tc_debug_set(b"force_den_entropy_streamed", 0) == 0


def test_wrappers_check_before_any_library_call():
    from torchain.functions import den_path_entropy
    fst = synth.random_den_fst(60, 4, 30, seed=21)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    y = torch.zeros((14, fst.num_pdfs))
    with pytest.raises(TypeError):
        den_path_entropy(y, fst, n_batch=2)
    with pytest.raises(ValueError, match="CUDA tensor"):
        den_path_entropy(y, graph, n_batch=2)
    with pytest.raises(ValueError, match="CUDA tensor"):
        graph.path_entropy(y, n_batch=2)
