"""End-to-end supervisions beyond the resident numerator kernel's limits (``from_e2e_fsts(..., any_size=True)``): the FSTs
of ``test_e2e_large_host.py`` and ``test_gpu_e2e_large.py``, and the GPU tests' float64 references (``e2e_reference``, computed
once per case and left unchanged).  A helper, not a test module; importing it needs no GPU."""
import functools

import numpy as np

import den_compose_cases as dc
import e2e_reference as ref

MAX_STATES, MAX_ARCS, MAX_PDFS = 2048, 8192, 1024  # the resident kernel's (TC_E2E_MAX_*)
LDS_LIMIT = 163840


def lds_rule(states, pdfs):
    """Left side of the any-size create rule: 16 * ceil4(states) + 4 * ceil4(distinct pdfs) + 2048 (<= LDS_LIMIT: accepted)."""
    return 16 * ((states + 3) // 4 * 4) + 4 * ((pdfs + 3) // 4 * 4) + 2048


# one past each of the resident limits: (states, arcs, distinct pdfs)
ONE_PAST = {"states": (MAX_STATES + 1, MAX_ARCS, MAX_PDFS), "arcs": (MAX_STATES, MAX_ARCS + 1, MAX_PDFS),
            "pdfs": (MAX_STATES, MAX_ARCS, MAX_PDFS + 1)}
AT_NEW_LIMIT = (8192, 40000, 4096)
LONG = (3000, 9000, 60)

# GPU cases against float64: name -> (sizes of the large sequence, T, P); each beside a 5-state FST
CASES = {"states": (ONE_PAST["states"], 20, 1030), "arcs": (ONE_PAST["arcs"], 20, 1030), "pdfs": (ONE_PAST["pdfs"], 20, 1030),
         "limit": (AT_NEW_LIMIT, 12, 4100), "long": (LONG, 300, 60)}
WEIGHT, L2, LEAKY = 0.7, 5e-4, 0.1
# a batch whose largest state count and largest pdf count belong to two sequences, each sequence at the LDS rule: the rule
# is per sequence, so the batch is taken although lds_rule(10108, 7680) is far beyond the limit
MIXED = ((10108, 12000, 4), (8192, 16000, 7680))
MIXED_T, MIXED_P = 6, 7700


def sizes(fst):
    """(states, arcs, distinct pdfs) of an FST tuple."""
    return len(fst[5]), int(fst[1][-1]), len(set(np.asarray(fst[2]).tolist()))


def planted(n_states, n_arcs, distinct, num_pdfs, seed):
    """``e2e_reference.random_fst`` with exactly these sizes: ``random_fst`` does not guarantee that every pdf of its pool
    occurs, so the pdfs 0 .. distinct - 1 are planted on the first arcs.  The start is final and has a self-loop: every T has
    a path."""
    fst = ref.distinct_pdfs_fst(n_states, n_arcs, num_pdfs, distinct, np.random.default_rng(seed))
    assert sizes(fst) == (n_states, n_arcs, distinct)
    return fst


def no_path(n_states, n_arcs, num_pdfs, seed):
    """A left-to-right acceptor of these sizes whose only final state is its last one: no path of fewer than
    ``n_states - 1`` arcs (parallel arcs of other pdfs and a self-loop on the last state make up the arc count)."""
    rng = np.random.default_rng(seed)
    arcs = [(i, i + 1, int(rng.integers(0, num_pdfs)), float(rng.uniform(0, 2))) for i in range(n_states - 1)]
    arcs.append((n_states - 1, n_states - 1, 0, 0.5))
    while len(arcs) < n_arcs:
        i = int(rng.integers(0, n_states - 1))
        arcs.append((i, i + 1, int(rng.integers(0, num_pdfs)), float(rng.uniform(0, 2))))
    final = np.full(n_states, np.inf, np.float32)
    final[-1] = 0.0
    fst = ref._csr(n_states, arcs, final)
    assert ref.shortest_path_arcs(fst) == n_states - 1
    return fst


@functools.lru_cache(maxsize=None)
def fsts(name):
    (n, a, d), T, P = CASES[name]
    rng = np.random.default_rng(len(name))
    return (planted(n, a, d, P, seed=100 + n + a + d), ref.random_fst(5, 12, P, rng))


@functools.lru_cache(maxsize=None)
def mixed_fsts():
    return tuple(planted(n, a, d, MIXED_P, seed=200 + i) for i, (n, a, d) in enumerate(MIXED))


@functools.lru_cache(maxsize=None)
def mixed_reference():
    want = ref.e2e_objective(oracle_graph(MIXED_P), list(mixed_fsts()), MIXED_T, nnet_output("mixed"), weight=WEIGHT, l2=L2,
                             leaky=LEAKY)
    assert want["ok"]
    for k in ("deriv", "xent_deriv"):
        want[k].setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def nnet_output(name, seed=8):
    _, T, P = (None, MIXED_T, MIXED_P) if name == "mixed" else CASES[name]
    y = (np.random.default_rng(seed).normal(size=(2 * T, P)) * 2.0).astype(np.float32)
    y.setflags(write=False)
    return y


def den_fst(P):
    from torchain_amd import synth
    return synth.random_den_fst(80, 4, P, seed=31)


@functools.lru_cache(maxsize=None)
def oracle_graph(P):
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle.DenGraph(den_fst(P))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's float64 objective (``e2e_reference.e2e_objective``: objf, l2_term, weight, deriv, xent_deriv)."""
    _, T, P = CASES[name]
    want = ref.e2e_objective(oracle_graph(P), list(fsts(name)), T, nnet_output(name), weight=WEIGHT, l2=L2, leaky=LEAKY)
    assert want["ok"]
    for k in ("deriv", "xent_deriv"):
        want[k].setflags(write=False)
    return want


# ---- composed with a denominator graph ---------------------------------------------------------------------------------
COMPOSED_GRAPH, COMPOSED_T = "random", 12


@functools.lru_cache(maxsize=None)
def composed_input():
    """An acceptor of 60 states -- a ring whose every state reads every pdf and is final -- that the resident kernel takes
    as it is, and whose composition with ``den_compose_cases``' random graph (one copy of a state per LM history alive in
    it) has more than 2048 states."""
    n = 60
    arcs = [(i, (i + 1) % n, p, 0.1 + 0.01 * p) for i in range(n) for p in range(dc.P)]
    return ref._csr(n, arcs, np.full(n, 0.5, np.float32))
