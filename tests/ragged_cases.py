"""Cases and float64 reference of the ragged (unequal sequence lengths) end-to-end tests: a helper, not a test module.

Sequences do not interact, so the ragged objective is the sum over sequences of the existing float64 reference
(``e2e_reference.e2e_objective``) on one sequence of its own length; rows ``t * S + s`` with ``t >= lengths[s]`` are padding
and the reference holds zeros there.  The den graph is the 80-state graph of ``test_gpu_e2e.py`` (P = 60).

The cases: the random family has a final start state with a self-loop, so every length >= 1 is feasible; the chain family's
shortest paths at seed 21 are 6-7 arcs, so (37, 12, 20, 29, 12) is feasible; ``equal`` is the all-lengths-equal ragged handle
that must give the uniform handle's bits.  ``test_ragged_host.py`` asserts ``ok`` for every sequence of every case, so that a
failure on the GPU is the kernel's.  Importing this module needs no GPU."""
import functools

import numpy as np

from torchain_amd import synth

import e2e_reference as ref

P = 60
WEIGHT, L2, LEAKY = 0.7, 5e-4, 0.1

# name -> (FST family, seed, lengths)
CASES = {
    "random": ("random", 3, (7, 1, 4, 2, 7)),
    "chain": ("chain", 21, (37, 12, 20, 29, 12)),
    "equal": ("random", 5, (9, 9, 9, 9)),
}

# Denominator forms (row_contract_cases.FAMILIES) that get a ragged batch, and the lengths: 3 sequences, the longest not last
DEN_FORMS = ("tied8_fused", "tied12_fused", "tied16_fused", "pdfs2_fused", "pdfs3_fused", "planes_fused", "split_fused",
             "general_owner", "general_old", "general_natural")
DEN_LENGTHS = (7, 2, 5)
# ... plus a sequence of one frame on the forms whose uniform call accepts T = 1 (S = 1, forced onto the form): every one of
# them does -- the one-workgroup kernels run frame 0's prologue, one loop frame and the epilogue for any T >= 1 (the forms
# that need T >= 2 are the two-workgroup ones, which a ragged batch never takes)
T1_FORMS = DEN_FORMS
DEN_MANY = 300  # sequences of the many-workgroups case on tied8, lengths cycling 1 .. 9


def den_lengths(form):
    return DEN_LENGTHS + ((1,) if form in T1_FORMS else ())


@functools.lru_cache(maxsize=None)
def den_fst():
    return synth.random_den_fst(80, 4, P, seed=31)


@functools.lru_cache(maxsize=None)
def oracle_graph():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle.DenGraph(den_fst())


@functools.lru_cache(maxsize=None)
def fsts(name):
    kind, seed, lengths = CASES[name]
    return tuple(ref.batch(kind, len(lengths), P, seed=seed))


def lengths(name):
    return CASES[name][2]


def padding_rows(lens):
    """Boolean [Tmax * S]: row t * S + s is padding (t >= lens[s])."""
    lens = np.asarray(lens)
    S, T = len(lens), int(lens.max())
    return (np.arange(T)[:, None] >= lens[None, :]).reshape(T * S)


def valid_rows(lens, s):
    """Row indices t * S + s of sequence s's own frames."""
    return np.arange(int(lens[s])) * len(lens) + s


@functools.lru_cache(maxsize=None)
def nnet_output(name, scale=2.0):
    """(Tmax * S, P) float32, finite everywhere (the tests put what they want into the padding of a copy); read-only."""
    lens = lengths(name)
    y = (np.random.default_rng(100 + len(lens) + max(lens)).normal(size=(max(lens) * len(lens), P)) * scale).astype(np.float32)
    y.setflags(write=False)
    return y


def with_padding(y, lens, value):
    out = np.array(y, copy=True)
    out[padding_rows(lens)] = value
    return out


def ragged_objective(den, seq_fsts, lens, y, weight=WEIGHT, l2=L2, leaky=LEAKY):
    """Sum over sequences of ``e2e_reference.e2e_objective`` on one sequence: dict(objf, l2_term, weight, deriv, xent_deriv,
    ok (per sequence), all_ok) in float64; deriv / xent_deriv are (Tmax * S, P) with zeros in the padding.  When a sequence
    fails the whole minibatch takes the failure route: objf = -10 * weight, deriv = -w * l2 * y on valid rows, xent 0."""
    lens = np.asarray(lens)
    S = len(lens)
    y = np.asarray(y, np.float32)
    out = dict(objf=0.0, l2_term=0.0, weight=0.0, deriv=np.zeros(y.shape), xent_deriv=np.zeros(y.shape), ok=[])
    for s in range(S):
        rows = valid_rows(lens, s)
        one = ref.e2e_objective(den, [seq_fsts[s]], int(lens[s]), y[rows], weight=weight, l2=l2, leaky=leaky)
        out["ok"].append(bool(one["ok"]))
        for k in ("objf", "l2_term", "weight"):
            out[k] += one[k]
        out["deriv"][rows] = one["deriv"]
        out["xent_deriv"][rows] = one["xent_deriv"]
    out["all_ok"] = all(out["ok"])
    if not out["all_ok"]:
        out["objf"] = -10.0 * out["weight"]
        out["deriv"][:] = 0.0
        out["xent_deriv"][:] = 0.0
        valid = ~padding_rows(lens)
        out["deriv"][valid] = -weight * l2 * y[valid].astype(np.float64)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's reference on its finite outputs, computed once; leave it unchanged."""
    out = ragged_objective(oracle_graph(), fsts(name), lengths(name), nnet_output(name))
    for k in ("deriv", "xent_deriv"):
        out[k].setflags(write=False)
    return out


def den_reference(og, lens, y, leaky, deriv_weight):
    """The denominator alone, per sequence: (sum of log-probs, (Tmax * S, P) derivative with zeros in the padding)."""
    from oracle import pyoracle
    lens = np.asarray(lens)
    lp, deriv = 0.0, np.zeros(y.shape)
    for s in range(len(lens)):
        rows = valid_rows(lens, s)
        one = pyoracle.den_forward_backward(og, np.ascontiguousarray(y[rows]), 1, leaky=leaky, deriv_weight=deriv_weight)
        assert one["ok"]
        lp += float(one["logprob"])
        deriv[rows] = one["deriv"]
    return lp, deriv
