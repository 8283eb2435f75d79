"""Cases and float64 references of the ragged REGULAR supervision tests (``io.Supervision.from_sequences`` /
``tc_supervision_create_ragged``): a helper, not a test module.  ``test_gpu_ragged_regular.py`` runs them on the GPU,
``test_ragged_regular_host.py`` without one.

A case is a list of single-sequence supervisions (``synth.SupFst`` with ``num_sequences == 1``), each of its own length, over
the 300-state graph of ``wide_supervisions`` (P = 200).  Sequences do not interact, so every reference is a sum over sequences
of an existing reference on one sequence of its own length: ``oracle.independent_f64.num_logprob`` and its autograd posteriors
for the numerator, the CPU oracle's ``compute_chain_objf_and_deriv`` for the objective; rows ``t * S + s`` with
``t >= lengths[s]`` are padding and the references hold zeros there.  Nothing here is computed by the code under test.

  small   (7, 1, 4, 2, 7), 3 paths        the longest is not last, a sequence has one frame
  trie    (37, 12, 20, 29, 12), 40 paths  resident kernel, too large for its tables to be staged in LDS
  equal   (9, 9, 9, 9), no final weights  against the uniform handle of the same pieces merged
  wide    lattices 120 states wide at (150, 31, 90): the longest is beyond the resident kernel's LDS, so the batch is windowed
  eight   (1, 6, 11, 5, 10, 4, 9, 11) on the tied graph ``tied8`` of ``row_contract_cases`` (P = 100): the denominator's
          two-workgroup ragged form beside the ragged numerator

Importing this module needs no GPU."""
import functools

import numpy as np

from torchain_amd import io, synth

import ragged_cases as rc
import row_contract_cases as rcc
import wide_supervisions as ws

P = ws.P
L2, LEAKY = 5e-4, 0.1
WIDE_WEIGHT = 0.75
TIED_GRAPH = "tied8"

EIGHT = tuple(1 + (5 * i) % 11 for i in range(7)) + (11,)
# name -> (lengths, paths per sequence (None: a lattice), final weights)
CASES = {
    "small": ((7, 1, 4, 2, 7), 3, True),
    "trie": ((37, 12, 20, 29, 12), 40, True),
    "equal": ((9, 9, 9, 9), 3, False),
    "wide": ((150, 31, 90), None, True),
    "eight": (EIGHT, 2, True),
}
NUMERATOR = ("small", "trie", "wide")
FITS_RESIDENT = ("small", "trie")  # also run under force_num_windowed


def lengths(name):
    return CASES[name][0]


def num_pdfs(name):
    return rcc.den_fst(TIED_GRAPH).num_pdfs if name == "eight" else P


@functools.lru_cache(maxsize=None)
def pieces(name):
    """The case's single-sequence supervisions, built once per process."""
    lens, paths, fw = CASES[name]
    seed0 = 100 * (1 + sorted(CASES).index(name))
    if name == "wide":
        return tuple(ws.lattice_supervision(1, T, P, lambda q, t, r: 120, 3, seed=seed0 + i, weight=WIDE_WEIGHT, final_weights=fw)
                     for i, T in enumerate(lens))
    if name == "eight":
        fst, pi = rcc.den_fst(TIED_GRAPH), rcc.initial_probs(TIED_GRAPH)
        return tuple(synth.random_supervision(fst, 1, T, paths, seed0 + i, weight=0.5, initial_probs=pi, final_weights=fw)
                     for i, T in enumerate(lens))
    return tuple(synth.random_supervision(ws.den_fst(), 1, T, paths, seed0 + i, final_weights=fw) for i, T in enumerate(lens))


def weight(name):
    return float(pieces(name)[0].weight)


def handle(name):
    """A fresh ragged handle of the case."""
    return io.Supervision.from_sequences(pieces(name))


@functools.lru_cache(maxsize=None)
def nnet_output(name, scale=1.0):
    """(Tmax * S, P) float32, finite everywhere (the tests put what they want into the padding of a copy); read-only."""
    lens = lengths(name)
    y = synth.random_nnet_output(len(lens), max(lens), num_pdfs(name), seed=200 + len(lens) + max(lens), scale=scale)
    y.setflags(write=False)
    return y


def sequence_rows(name, s, y=None):
    """Sequence s's own rows of the case's outputs, as the contiguous (T_s, P) matrix a call on that sequence alone takes."""
    y = nnet_output(name) if y is None else y
    return np.ascontiguousarray(y[rc.valid_rows(lengths(name), s)])


@functools.lru_cache(maxsize=None)
def num_reference(name):
    """(float64 weight * sum of the sequences' log-probs, float64 weight * posteriors as (Tmax * S, P) with zeros in the
    padding): ``oracle.independent_f64.num_logprob`` on every sequence alone, on its own rows.  Leave the array unchanged."""
    import torch

    from oracle import independent_f64 as ind
    lens = lengths(name)
    y = nnet_output(name)
    total, post = 0.0, np.zeros(y.shape)
    for s, piece in enumerate(pieces(name)):
        yt = torch.tensor(sequence_rows(name, s).astype(np.float64), requires_grad=True)
        lp = ind.num_logprob(piece, yt)
        (gamma,) = torch.autograd.grad(lp, yt)
        total += piece.weight * float(lp.detach())
        post[rc.valid_rows(lens, s)] = piece.weight * gamma.numpy()
    post.setflags(write=False)
    return total, post


@functools.lru_cache(maxsize=None)
def oracle_graph(name):
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle.DenGraph(rcc.den_fst(TIED_GRAPH) if name == "eight" else ws.den_fst())


def ragged_objective(og, seq_pieces, lens, y, l2=L2, leaky=LEAKY):
    """Sum over sequences of the CPU oracle's ``compute_chain_objf_and_deriv`` on one sequence alone (what
    ``ragged_cases.ragged_objective`` is for end-to-end supervisions): dict(objf, l2_term, weight, deriv, xent_deriv) in
    float64; deriv / xent_deriv are (Tmax * S, P) with zeros in the padding.  Every sequence must succeed."""
    from oracle import pyoracle
    lens = np.asarray(lens)
    y = np.asarray(y, np.float32)
    out = dict(objf=0.0, l2_term=0.0, weight=0.0, deriv=np.zeros(y.shape), xent_deriv=np.zeros(y.shape))
    for s, piece in enumerate(seq_pieces):
        assert piece.num_sequences == 1 and piece.frames_per_sequence == lens[s]
        rows = rc.valid_rows(lens, s)
        one = pyoracle.compute_chain_objf_and_deriv(og, piece, np.ascontiguousarray(y[rows]), l2, leaky, want_xent=True)
        assert np.isfinite(one["objf"]) and one["objf"] != -10.0 * one["weight"], (s, one["results"])
        for k in ("objf", "l2_term", "weight"):
            out[k] += float(one[k])
        out["deriv"][rows] = one["deriv"]
        out["xent_deriv"][rows] = one["xent_deriv"]
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's objective reference on its finite outputs, computed once; leave it unchanged."""
    out = ragged_objective(oracle_graph(name), pieces(name), lengths(name), nnet_output(name))
    for k in ("deriv", "xent_deriv"):
        out[k].setflags(write=False)
    return out


def concatenated(seq_pieces):
    """The arguments of ``tc_supervision_create_ragged`` behind label_dim, as numpy arrays: (seq_state_begin, arc_begin, ilabel,
    arc_weight, nextstate, final) of the pieces concatenated."""
    sb, ab, arcs = [0], [np.zeros(1, np.int32)], 0
    for p in seq_pieces:
        sb.append(sb[-1] + p.num_states)
        ab.append(np.asarray(p.arc_begin[1:], np.int32) + arcs)
        arcs += int(p.arc_begin[-1])
    cat = lambda field, dt: np.ascontiguousarray(np.concatenate([np.asarray(getattr(p, field)) for p in seq_pieces]), dt)  # noqa: E731
    return (np.asarray(sb, np.int32), np.ascontiguousarray(np.concatenate(ab), np.int32), cat("ilabel", np.int32),
            cat("arc_weight", np.float32), cat("nextstate", np.int32), cat("final", np.float32))
