"""End-to-end supervisions on the host: the handle's validation and size limits (tc_supervision_create_e2e), and the
float64 reference the GPU tests compare against (tests/e2e_reference.py)."""
import ctypes as C

import numpy as np
import pytest

from torchain_amd import io
from torchain_amd._lib import TorchainHipError, lib

import e2e_reference as ref

BAD_FST, UNSUPPORTED, INVALID = -2, -3, -1
MAX_STATES, MAX_ARCS, MAX_PDFS = 2048, 8192, 1024


def _make(fsts, T=5, P=50, weight=1.0):
    return io.Supervision.from_e2e_fsts(weight, T, P, fsts)


def _err(fsts, T=5, P=50):
    with pytest.raises(TorchainHipError) as ei:
        _make(fsts, T, P)
    return ei.value


def _loop_fst(n_states=3, pdf=1):
    return ref._csr(n_states, [(i, (i + 1) % n_states, pdf, 0.5) for i in range(n_states)],
                    np.r_[np.float32(0.0), np.full(n_states - 1, np.inf, np.float32)])


def test_handle_reports_shape_and_kind():
    fsts = ref.batch("chain", 4, 30, seed=1)
    sup = _make(fsts, T=20, P=30, weight=0.5)
    assert sup.is_e2e
    assert sup.shape == (4, 20, 30)
    assert sup.weight == 0.5
    assert lib.tc_supervision_is_e2e(None) == 0


def test_regular_handle_is_not_e2e():
    from torchain_amd import synth
    fst = synth.random_den_fst(20, 3, 10, seed=2)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, 2, 6, 2, seed=3))
    assert not sup.is_e2e


def _mutate(field, index, value, fst=None):
    fst = list(fst or _loop_fst())
    arr = np.array(fst[field], copy=True)
    arr[index] = value
    fst[field] = arr
    return tuple(fst)


@pytest.mark.parametrize("case", ["epsilon", "label_high", "next_high", "next_negative", "start_high", "start_negative",
                                  "nan_cost", "nan_final", "minus_inf_cost", "no_final"])
def test_validation_errors_are_bad_fst(case):
    good = _loop_fst()
    fst = {
        "epsilon": lambda: _mutate(2, 0, 0),
        "label_high": lambda: _mutate(2, 1, 51),
        "next_high": lambda: _mutate(4, 0, 3),
        "next_negative": lambda: _mutate(4, 2, -1),
        "start_high": lambda: (3,) + good[1:],
        "start_negative": lambda: (-1,) + good[1:],
        "nan_cost": lambda: _mutate(3, 0, np.nan),
        "nan_final": lambda: _mutate(5, 1, np.nan),
        "minus_inf_cost": lambda: _mutate(3, 1, -np.inf),
        "no_final": lambda: _mutate(5, 0, np.inf),
    }[case]()
    # the bad FST in the middle of a batch of good ones
    e = _err([good, fst, good])
    assert e.code == BAD_FST


def _sized(n_states, n_arcs, n_pdfs):
    """A sequence with exactly these sizes: a ring, then extra arcs cycling over the pdfs 0 .. n_pdfs - 1."""
    arcs = [(i, (i + 1) % n_states, i % n_pdfs, 0.1) for i in range(n_states)]
    k = n_states
    while len(arcs) < n_arcs:
        arcs.append((k % n_states, (k * 7 + 3) % n_states, k % n_pdfs, 0.2))
        k += 1
    final = np.full(n_states, np.inf, np.float32)
    final[0] = 0.0
    return ref._csr(n_states, arcs, final)


@pytest.mark.parametrize("what", ["states", "arcs", "pdfs"])
def test_size_limit_at_and_one_past(what):
    P = MAX_PDFS + 8
    at = dict(states=(MAX_STATES, MAX_ARCS, MAX_PDFS), arcs=(MAX_STATES, MAX_ARCS, MAX_PDFS),
              pdfs=(MAX_STATES, MAX_ARCS, MAX_PDFS))[what]
    past = dict(states=(MAX_STATES + 1, MAX_ARCS, MAX_PDFS), arcs=(MAX_STATES, MAX_ARCS + 1, MAX_PDFS),
                pdfs=(MAX_STATES, MAX_ARCS, MAX_PDFS + 1))[what]
    small = _loop_fst()
    sup = _make([small, _sized(*at)], T=10, P=P)
    assert sup.is_e2e
    e = _err([small, _sized(*past)], T=10, P=P)
    assert e.code == UNSUPPORTED


def test_invalid_arguments():
    h = C.c_void_p()
    z = np.zeros(2, np.int32)
    assert lib.tc_supervision_create_e2e(None, 1.0, 1, 5, 10, None, None, None, None, None, None, None) == INVALID
    assert lib.tc_supervision_create_e2e(C.byref(h), 1.0, 0, 5, 10, z.ctypes.data, z.ctypes.data, z.ctypes.data,
                                         None, None, None, z.ctypes.data) == INVALID
    with pytest.raises(ValueError):
        io.Supervision.from_e2e_fsts(1.0, 5, 10, [])


# ---- the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["chain", "random"])
def test_reference_posteriors_sum_to_one_per_frame(kind):
    S, T, P = 5, 12, 40
    fsts = ref.batch(kind, S, P, seed=4)
    y = np.random.default_rng(5).normal(size=(S * T, P))
    logz, gamma = ref.num_logz(fsts, y, T)
    assert np.isfinite(logz).all()
    sums = gamma.sum(axis=1)
    np.testing.assert_allclose(sums, 1.0, rtol=0, atol=1e-10)
    assert (gamma >= -1e-15).all()


@pytest.mark.parametrize("kind", ["chain", "random"])
def test_reference_log_z_finite_differences(kind):
    S, T, P = 3, 9, 25
    fsts = ref.batch(kind, S, P, seed=6)
    rng = np.random.default_rng(7)
    y = rng.normal(size=(S * T, P))
    logz, gamma = ref.num_logz(fsts, y, T)
    d = rng.normal(size=y.shape)
    eps = 1e-6
    lp, _ = ref.num_logz(fsts, y + eps * d, T, want_gamma=False)
    lm, _ = ref.num_logz(fsts, y - eps * d, T, want_gamma=False)
    fd = (lp.sum() - lm.sum()) / (2 * eps)
    assert abs(fd - (gamma * d).sum()) <= 1e-6 * max(1.0, abs(fd))


def test_reference_log_z_by_enumeration():
    """A two-state FST small enough to enumerate every path of T arcs."""
    fst = ref._csr(2, [(0, 0, 0, 0.3), (0, 1, 1, 1.0), (1, 1, 2, 0.1), (1, 0, 0, 2.0)], [np.inf, 0.7])
    T, P = 4, 3
    y = np.random.default_rng(8).normal(size=(T, P))
    import itertools
    tot = 0.0
    arcs = [(0, 0, 0, 0.3), (0, 1, 1, 1.0), (1, 1, 2, 0.1), (1, 0, 0, 2.0)]
    for path in itertools.product(range(4), repeat=T):
        s, lp = 0, 0.0
        for t, a in enumerate(path):
            if arcs[a][0] != s:
                break
            lp += -float(np.float32(arcs[a][3])) + y[t, arcs[a][2]]  # (the CSR holds fp32 costs)
            s = arcs[a][1]
        else:
            if s == 1:
                tot += np.exp(lp - float(np.float32(0.7)))
    logz, _ = ref.num_logz([fst], y, T, want_gamma=False)
    assert abs(logz[0] - np.log(tot)) <= 1e-12 * abs(np.log(tot)) + 1e-12


def test_reference_infeasible_is_minus_inf():
    rng = np.random.default_rng(9)
    fst = ref.chain_fst(30, rng, words=3, max_phones=2, silence=False)
    shortest = ref.shortest_path_arcs(fst)
    assert shortest >= 3
    good = ref.batch("random", 2, 30, seed=10)
    for T in (shortest - 1, shortest):
        y = rng.normal(size=(3 * T, 30))
        logz, gamma = ref.num_logz([good[0], fst, good[1]], y, T)
        assert np.isfinite(logz[[0, 2]]).all()
        assert np.isfinite(logz[1]) == (T >= shortest)
        assert np.isfinite(gamma).all()
