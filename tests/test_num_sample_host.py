"""Host side of ``tc_supervision_sample_paths``: the float64 reference of ``tests/num_sample_reference.py`` against the
enumerated path posterior of two tiny FSTs, the workspace and kernel queries, and the refusals of bad arguments.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from torchain_amd import io
from torchain_amd._lib import lib

import e2e_reference as e2e
import num_arc_post_reference as apr
import num_entropy_reference as ner
import num_sample_reference as nsr

r256 = lambda x: x + 255 & ~255  # noqa: E731
# an acyclic acceptor in time order, T = 3: two levels of two states, parallel arcs
LATTICE = e2e._csr(6, [(0, 1, 0, 0.3), (0, 1, 1, 0.9), (0, 2, 2, 0.2), (1, 3, 0, 0.5), (1, 4, 1, 0.1), (2, 4, 3, 0.7), (2, 3, 2, 0.4),
                       (3, 5, 1, 0.6), (4, 5, 0, 0.2), (4, 5, 3, 1.0)], [np.inf] * 5 + [0.25])


@pytest.mark.parametrize("kind", ["cycles", "lattice"])
def test_reference_samples_follow_the_enumerated_posterior(kind):
    fst, T, e2e_kind = (ner.tiny_fst(), 4, True) if kind == "cycles" else (LATTICE, 3, False)
    rng, N = np.random.default_rng(3), 6000
    y = (np.round(rng.normal(0.0, 0.5, size=(T, 4)) * 8) / 8).astype(np.float32)
    want, tab = apr.by_enumeration(fst, y.astype(np.float64)), nsr.tables(fst)
    fwd = nsr.forward(tab, y, e2e_kind)
    assert abs(fwd[2] - want["logprob"]) <= 1e-5
    uses, ends, flagged = np.zeros((N, len(tab[1]))), np.zeros((N, len(tab[5]))), 0
    for k, u in enumerate(rng.random((N, T + 1), dtype=np.float32)):
        pdfs, states, score, close, arcs = nsr.sample(tab, fwd, u, nsr.delta(T, 3, e2e_kind))
        np.add.at(uses[k], arcs, 1)
        ends[k, states[T]] = 1
        flagged += close
        lw = sum(float(tab[4][a]) + float(y[t, tab[3][a]]) for t, a in enumerate(arcs)) + float(tab[5][states[T]])
        assert states[0] == tab[0] and (tab[2][arcs] == states[1:]).all() and abs(score - lw) <= 1e-5
    for got, p in ((uses, want["arcs"]), (ends, want["finals"])):  # the sample's own standard errors (an exact 0 or 1: 1e-9)
        err = np.abs(got.mean(0) - p) / np.maximum(got.std(0) / np.sqrt(N), 1e-9)
        print("MEASURED %s: largest deviation %.2f standard errors, %d flagged" % (kind, err.max(), flagged))
        assert err.max() <= 5.0
    assert ((want["arcs"] > 0.05) & (want["arcs"] < 0.95)).sum() >= 4  # (the comparison is of something)
    assert flagged <= N // 100


def test_queries_answer_on_the_host():
    need, kernel = lib.tc_supervision_sample_paths_workspace_bytes, lib.tc_supervision_sample_paths_kernel
    rng = np.random.default_rng(5)
    ends = io.Supervision.from_e2e_fsts(1.0, 5, 9, [e2e.random_fst(6, 20, 9, rng), e2e.random_fst(4, 9, 9, rng)])
    regular = io.Supervision.from_fsts(1.0, [3], 4, [LATTICE[1:]])
    assert need(ends.ptr) == r256(8 * (5 + 1) * 10) and need(regular.ptr) == r256(8 * 6) and need(None) == -1
    assert kernel(ends.ptr) == 0 and kernel(regular.ptr) == 0 and kernel(None) == -1
    # 16 * ceil4(states) + 8 * ceil4(pdfs) + 2048 <= 163840 ends at 12032 distinct pdfs beside 4096 states; the numerator takes more
    wide = io.Supervision.from_e2e_fsts(1.0, 2, 12036, [e2e.distinct_pdfs_fst(4096, 12036, 12036, 12036, rng)], any_size=True)
    assert kernel(wide.ptr) == 1 and need(wide.ptr) == r256(8 * 3 * 4096)
    assert lib.tc_debug_set(b"force_num_sample_streamed", 1) == 0
    try:
        assert kernel(ends.ptr) == 1 and kernel(regular.ptr) == 1 and need(ends.ptr) == r256(8 * 6 * 10)
    finally:
        assert lib.tc_debug_set(b"force_num_sample_streamed", 0) == 0


def test_bad_arguments_are_refused_before_any_device_call():
    sup = io.Supervision.from_e2e_fsts(1.0, 5, 9, [e2e.random_fst(6, 20, 9, np.random.default_rng(5))])
    fake, call = C.c_void_p(4096), lib.tc_supervision_sample_paths  # (nothing is dereferenced)
    good = [sup.ptr, fake, 0, 0, 5, 9, 9, 3, fake, fake, fake, fake, None, fake, 1 << 20, 0, None]

    def code(**change):
        names = ("sup y dtype bct rows cols stride K u pdf score logprob state ws ws_bytes device stream").split()
        return call(*[change.get(n, v) for n, v in zip(names, good)])

    for bad in (dict(sup=None), dict(y=None), dict(u=None), dict(pdf=None), dict(score=None), dict(logprob=None), dict(K=0), dict(K=-2),
                dict(dtype=7), dict(dtype=1), dict(rows=6), dict(cols=8), dict(stride=8), dict(score=C.c_void_p(4100)),
                dict(state=C.c_void_p(4098))):
        assert code(**bad) == -1, bad  # TC_ERR_INVALID_ARGUMENT
    for bad in (dict(ws=None), dict(ws_bytes=8), dict(ws=C.c_void_p(4104))):
        assert code(**bad) == -4, bad  # TC_ERR_WORKSPACE
