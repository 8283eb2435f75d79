"""Cases and the float64 statement of ``chain_loss(..., xent_log_softmax=True)`` (``tc_chain_step_log_softmax``):
a helper, not a test module.  ``test_xent_log_softmax_host.py`` runs without a GPU, ``test_gpu_xent_log_softmax.py`` on one.

The contract, row by row (row = one (sequence, frame), c = channel), with V the xent gradient the call WITHOUT the option
returns for the same arguments (``-xent_regularize * dw[row] * w * gamma_num``):

    G[row, c]  = V[row, c] - (sum_c' V[row, c']) * softmax(x[row, :])[c]        (a row of V without a non-zero entry: +0)
    xent_objf  = sum_rows sum_c w * gamma_num[row, c] * (x[row, c] - lse(x[row, :]))

``grad64`` and ``objective64`` state them in float64 numpy.

The shapes (S, T, P) are the smallest that reach the kernels' edges:

    ragged_float4  3 x 7  x 13     a row of 13 floats (3 float4 and one more behind a padded row stride), one partial wave
    full_row       2 x 5  x 4096   a full row per workgroup
    tile_edge      1 x 67 x 4100   a second tile of 3 frames in (B, C, T), a channel tail behind 4096
    two_passes     2 x 3  x 10240  more than one pass of channels per thread in every kernel

Graphs come from ``synth.random_den_fst`` (64 states), supervisions from ``synth.random_supervision``.  ``xent_input`` has
N(0, 1) rows (even rows) and N(0, 25) rows (odd rows); row 1 is shifted by +1e4 and row 2 by -1e4 -- a kernel that takes
``exp(x)`` without subtracting the row's maximum overflows or underflows there.  Importing this module needs no GPU."""
import functools

import numpy as np

from torchain_amd import synth

WEIGHT, L2, LEAKY, XREG = 0.7, 5e-4, 0.1, 0.1
SHIFT = 1.0e4

# name -> (S, T, P)
SHAPES = {
    "ragged_float4": (3, 7, 13),
    "full_row": (2, 5, 4096),
    "tile_edge": (1, 67, 4100),
    "two_passes": (2, 3, 10240),
}
CASES = tuple(SHAPES)
RAGGED_LENGTHS = (7, 3, 5)  # (the ragged handle of ``ragged_float4``'s graph: ``io.Supervision.from_sequences``)


def _seed(name):
    return 100 * (1 + CASES.index(name))


@functools.lru_cache(maxsize=None)
def den_fst(name):
    return synth.random_den_fst(64, 3, SHAPES[name][2], seed=_seed(name))


@functools.lru_cache(maxsize=None)
def initial_probs(name):
    return synth.initial_probs_f64(den_fst(name))


@functools.lru_cache(maxsize=None)
def supervision(name):
    S, T, _ = SHAPES[name]
    return synth.random_supervision(den_fst(name), S, T, 2, seed=_seed(name) + 1, weight=WEIGHT, initial_probs=initial_probs(name))


@functools.lru_cache(maxsize=None)
def ragged_pieces():
    """Single-sequence supervisions of ``RAGGED_LENGTHS`` frames on ``ragged_float4``'s graph."""
    name = "ragged_float4"
    return tuple(synth.random_supervision(den_fst(name), 1, T, 2, seed=_seed(name) + 10 + i, weight=WEIGHT,
                                          initial_probs=initial_probs(name)) for i, T in enumerate(RAGGED_LENGTHS))


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def chain_input(name, S=None, T=None):
    """(T * S, P) float32, rows ``t * S + s``; read-only."""
    s, t, P = SHAPES[name]
    return _frozen(synth.random_nnet_output(S or s, T or t, P, seed=_seed(name) + 2))


@functools.lru_cache(maxsize=None)
def xent_input(name, S=None, T=None):
    """(T * S, P) float32, rows ``t * S + s``: N(0, 1) in even rows, N(0, 25) in odd rows, row 1 + 1e4, row 2 - 1e4; read-only."""
    s, t, P = SHAPES[name]
    rows = (S or s) * (T or t)
    rng = np.random.default_rng(_seed(name) + 3)
    x = rng.standard_normal((rows, P))
    x[1::2] *= 5.0
    x[1] += SHIFT
    x[2] -= SHIFT
    return _frozen(x.astype(np.float32))


# ---- the contract in float64 ----------------------------------------------------------------------------------------------------------
def lse64(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=1, keepdims=True)
    return m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))


def softmax64(x):
    return np.exp(np.asarray(x, np.float64) - lse64(x))


def grad64(V, x):
    """G = V - rowsum(V) * softmax(x) in float64; a row of V without a non-zero entry is +0 whatever x holds there."""
    V = np.asarray(V, np.float64)
    mass = (V != 0).any(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        G = V - V.sum(axis=1, keepdims=True) * softmax64(x)
    return np.where(mass, G, 0.0)


def objective64(wgamma, x):
    """sum_rows sum_c wgamma * (x - lse(row)) in float64, over the entries wgamma has (the numerator's posteriors)."""
    wgamma = np.asarray(wgamma, np.float64)
    with np.errstate(all="ignore"):
        logp = np.asarray(x, np.float64) - lse64(x)
    return float(np.where(wgamma != 0, wgamma * np.where(wgamma != 0, logp, 0.0), 0.0).sum())


def row_mass(V):
    """max over rows of |sum_c V[row, c]|: what the tests' error figures are relative to."""
    return float(np.abs(np.asarray(V, np.float64).sum(axis=1)).max())


def random_wgamma(name, seed=0):
    """A stand-in for the numerator's weighted posteriors without a GPU: (T * S, P) float64, two to four positive entries a
    row, one row of none."""
    S, T, P = SHAPES[name]
    rng = np.random.default_rng(_seed(name) + 7 + seed)
    w = np.zeros((S * T, P))
    for r in range(S * T):
        if r == 3:
            continue
        cols = rng.choice(P, size=int(rng.integers(2, 5)), replace=False)
        p = rng.uniform(0.05, 1.0, size=cols.size)
        w[r, cols] = WEIGHT * p / p.sum()
    return w
