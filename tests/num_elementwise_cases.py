"""The cases of the element-wise numerator tests (a helper, not a test module): supervisions, network outputs and their
float64 posteriors, built once per process and shared by ``test_gpu_num_elementwise.py`` and ``test_num_elementwise_host.py``.

The references are the two float64 autograd formulations and nothing else: ``oracle.independent_f64.num_logprob`` for regular
supervisions (times the supervision's weight), ``e2e_reference.num_logz`` for end-to-end ones.  Neither clamps the outputs.

Tolerances.  Regular kernels: 2e-5 relative on every entry above 1e-8, three times the CPU oracle's own worst distance to
float64 on these inputs (6.7e-6; the kernels add one float32 rounding of the log-occupation, the device's exp behind a float32
multiply by log2(e), and float32 sums of a few dozen terms: about 4e-6 at an occupation of 1e-8).  End-to-end kernel: 2e-5 up
to 150 frames and 5e-5 for the 1200-frame utterance, four times what ``e2e_reference.kernel_arithmetic`` (the kernel's
arithmetic in numpy) differs from float64 by (5.4e-6 and 1.25e-5).  Log-probabilities: 1e-6 relative (the recursions are in
double)."""
import functools

import numpy as np
import torch

from torchain_amd import synth

import e2e_reference as e2e
import wide_supervisions as ws

REL_REGULAR = 2e-5
REL_E2E = 2e-5
REL_E2E_LONG = 5e-5
REL_LOGPROB = 1e-6
SCALES = (1.0, 8.0)
E2E_SCALES = (2.0, 8.0)
E2E_WEIGHT = 0.7

# ---- regular supervisions -------------------------------------------------------------------------------------------------
SINGLE_PATH = {"single_path_1": 1, "single_path_2": 2, "single_path_150": 150}  # name -> frames (two sequences, paths=1)
RESIDENT = ("trie_150x3", "trie_150x40", "lattice_bursty", "lattice_edge") + tuple(SINGLE_PATH)
WINDOWED = ("lattice_wide", "lattice_pinch", "lattice_mixed")
FORCED = ("lattice_edge", "lattice_fits")  # fit the resident kernel; run under force_num_windowed


def beyond_30(y, row, pdf):
    """Makes sure a matrix drawn at scale 8 leaves +-30 (where the denominator clamps and the numerator does not): a small one
    may not on its own, and then the entry (row, pdf), one that an arc reads, is set to 33."""
    if np.abs(y).max() <= 30.0:
        y[row, pdf] = 33.0
    assert np.abs(y).max() > 30.0
    return y


@functools.lru_cache(maxsize=None)
def regular_supervision(name):
    if name in SINGLE_PATH:
        return synth.random_supervision(ws.den_fst(), 2, SINGLE_PATH[name], 1, seed=11, final_weights=True)
    return ws.supervision(name)


@functools.lru_cache(maxsize=None)
def regular_case(name, scale):
    """(supervision, y, float64 weight * log-prob, float64 weight * posteriors); the arrays are shared: leave them unchanged."""
    from oracle import independent_f64 as ind
    sup = regular_supervision(name)
    y = synth.random_nnet_output(sup.num_sequences, sup.frames_per_sequence, ws.P, seed=5, scale=scale)
    if scale >= 8.0:
        beyond_30(y, 0, int(sup.ilabel[0]) - 1)
    yt = torch.tensor(y.astype(np.float64), requires_grad=True)
    lp = ind.num_logprob(sup, yt)
    (gamma,) = torch.autograd.grad(lp, yt)
    ref = sup.weight * gamma.numpy()
    ref.setflags(write=False)
    return sup, y, sup.weight * float(lp.detach()), ref


def staged_in_lds(stats):
    """Whether the resident kernel copies the sequence's tables into LDS (launch_num in csrc/num_kernels.hip): the sequence
    plus its tables within a quarter of the LDS limit."""
    states, arcs = (stats["max_states"] + 1) & ~1, (stats["max_arcs"] + 3) & ~3
    return stats["resident_lds_bytes"] + 4 * (2 * (states + 2) + 5 * arcs + stats["frames"] + 2) <= ws.LDS_LIMIT // 4


# ---- end-to-end supervisions ----------------------------------------------------------------------------------------------
def _chain_or_random(kind, S, T):
    def make():
        if kind == "chain" and T == 1:  # (the one chain graph with a path of one arc: a single phone, no silence)
            return e2e.batch("chain", S, 60, seed=S * 1000 + T, words=1, max_phones=1, silence=False), T, 60
        return e2e.batch(kind, S, 60, seed=S * 1000 + T), T, 60
    return make


def _states():
    rng = np.random.default_rng(41)
    return [e2e.random_fst(n, 1000, 60, rng) for n in (255, 256, 257)], 12, 60


def _pdfs():
    rng = np.random.default_rng(43)
    return [e2e.distinct_pdfs_fst(300, 1200, 300, k, rng) for k in (255, 256, 257)], 8, 300


def _pdfs_1024():
    """The size-limit sequence of test_long_utterance_and_size_limit_sequence: 2048 states, 8192 arcs, 1024 pdfs."""
    rng = np.random.default_rng(7)
    big = e2e.distinct_pdfs_fst(2048, 8192, 1030, 1024, rng)
    assert len(big[5]) == 2048 and big[1][-1] == 8192
    return [big, e2e.random_fst(5, 12, 1030, rng)], 8, 1030


def _start_and_unreachable():
    """A start state that is not state 0, and states the start cannot reach whose arcs carry pdfs of their own."""
    rng = np.random.default_rng(47)
    fsts = []
    while len(fsts) < 2:
        f = e2e.random_fst(9, 30, 60, rng, pdf_pool=np.arange(50))
        if f[0] != 0:
            fsts.append(e2e.with_unreachable_states(f, [53, 57], rng))
    return fsts, 20, 60


def _long():
    return e2e.batch("chain", 2, 60, seed=5, words=12, max_phones=4), 1200, 60


E2E = {"%s_%dx%d" % (k, S, T): _chain_or_random(k, S, T) for k in ("chain", "random") for S, T in ((3, 150), (7, 37), (1, 1))}
E2E.update(states_255_256_257=_states, pdfs_255_256_257=_pdfs, pdfs_1024=_pdfs_1024,
           start_and_unreachable=_start_and_unreachable)
E2E_SHORT = tuple(E2E)  # at most 150 frames
E2E["long_1200"] = _long


def e2e_rel(name):
    return REL_E2E_LONG if name == "long_1200" else REL_E2E


@functools.lru_cache(maxsize=None)
def e2e_case(name, scale):
    """(fsts, T, P, y, float64 weight * sum of log Z, float64 weight * posteriors), shared: leave the arrays unchanged."""
    fsts, T, P = E2E[name]()
    S = len(fsts)
    seed = 6 if name == "long_1200" else S + T  # (the long pair with the outputs test_gpu_e2e.py gives it)
    y = (np.random.default_rng(seed).normal(size=(S * T, P)) * scale).astype(np.float32)
    if scale >= 8.0:
        start, ab, il = fsts[0][:3]
        beyond_30(y, 0, int(il[ab[start]]) - 1)
    logz, gamma = e2e.num_logz(fsts, y.astype(np.float64), T)
    assert np.isfinite(logz).all()
    ref = E2E_WEIGHT * gamma
    ref.setflags(write=False)
    return fsts, T, P, y, E2E_WEIGHT * float(logz.sum()), ref
