"""Ragged end-to-end supervisions without a GPU: the handle (tc_supervision_create_e2e_ragged, tc_supervision_frames,
tc_supervision_is_ragged, num_frame = the longest length), the Python layer, the argument checks of the ragged entries that
need no device, the reference module on its cases and the geometry of the padding."""
import ctypes as C

import numpy as np
import pytest

from torchain_amd import egs, io
from torchain_amd._lib import TorchainHipError, lib

import e2e_reference as ref
import ragged_cases as rc

TC_ERR_INVALID_ARGUMENT, TC_ERR_UNSUPPORTED = -1, -3


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_handle_reports_lengths_and_longest(name):
    lens = rc.lengths(name)
    sup = io.Supervision.from_e2e_fsts(rc.WEIGHT, list(lens), rc.P, rc.fsts(name))
    assert sup.is_e2e and sup.is_ragged  # (also when all lengths are equal)
    assert sup.frames.dtype == np.int32 and tuple(sup.frames) == lens
    assert sup.n_frame == max(lens) == lib.tc_supervision_num_frame(sup.ptr)
    assert sup.shape == (len(lens), max(lens), rc.P)
    assert sup.weight == np.float32(rc.WEIGHT)


def test_uniform_entry_is_unchanged():
    fsts = rc.fsts("random")
    sup = io.Supervision.from_e2e_fsts(0.5, 7, rc.P, fsts)
    assert sup.is_e2e and not sup.is_ragged
    assert tuple(sup.frames) == (7,) * len(fsts) and sup.n_frame == 7
    # numpy integers and 0-d arrays are single lengths too
    assert not io.Supervision.from_e2e_fsts(0.5, np.int64(7), rc.P, fsts).is_ragged
    # a regular supervision reports its one frames_per_sequence
    from torchain_amd import synth
    fst = rc.den_fst()
    reg = io.Supervision.from_synth(synth.random_supervision(fst, 3, 6, 2, seed=1))
    assert not reg.is_ragged and tuple(reg.frames) == (6, 6, 6)


@pytest.mark.parametrize("bad", [(7, 0, 4, 2, 7), (7, -3, 4, 2, 7), (0, 0, 0, 0, 0)])
def test_a_length_below_one_is_refused(bad):
    with pytest.raises(TorchainHipError) as e:
        io.Supervision.from_e2e_fsts(1.0, list(bad), rc.P, rc.fsts("random"))
    assert e.value.code == TC_ERR_INVALID_ARGUMENT


def test_python_argument_checks():
    fsts = rc.fsts("random")
    with pytest.raises(ValueError):
        io.Supervision.from_e2e_fsts(1.0, [7, 1, 4], rc.P, fsts)  # not one length per sequence
    with pytest.raises(ValueError):
        io.Supervision.from_e2e_fsts(1.0, [7.5, 1, 4, 2, 7], rc.P, fsts)
    out = np.zeros(len(fsts), np.int32)
    assert lib.tc_supervision_frames(None, out.ctypes.data_as(C.c_void_p)) == TC_ERR_INVALID_ARGUMENT
    assert lib.tc_supervision_is_ragged(None) == 0


def test_size_limits_use_the_longest_length():
    """S * Tmax <= 2^26, whatever the sum of the lengths is."""
    fsts = rc.fsts("random")[:2]
    with pytest.raises(TorchainHipError) as e:
        io.Supervision.from_e2e_fsts(1.0, [(1 << 25) + 1, 1], rc.P, fsts)
    assert e.value.code == TC_ERR_UNSUPPORTED


def test_e2e_sup_passes_a_list_through():
    lens = rc.lengths("random")
    s = egs.E2eSup(0.5, len(lens), list(lens), rc.P, rc.fsts("random"))
    assert s.frames_per_sequence == list(lens)
    sup = io.Supervision.from_synth(s)
    assert sup.is_ragged and tuple(sup.frames) == lens
    assert egs.E2eSup(0.5, 5, 7, rc.P, rc.fsts("random")).frames_per_sequence == 7


def test_den_entry_argument_checks_need_no_device():
    g = io.DenominatorGraph(rc.den_fst(), rc.P)
    one = C.c_void_p(16)  # (never dereferenced: every call below is refused first)
    args = lambda rows, frames, tmax: (g.ptr, 3, one, rows, rc.P, rc.P, 0.1, 1.0, 0.0, 0, one, rc.P, frames, tmax, one, one, one,
                                       1 << 20, 0, None)
    assert lib.tc_den_forward_backward_ragged(*args(21, None, 7)) == TC_ERR_INVALID_ARGUMENT     # no lengths
    assert lib.tc_den_forward_backward_ragged(*args(20, one, 7)) == TC_ERR_INVALID_ARGUMENT      # rows != max_frames * S
    assert lib.tc_den_forward_backward_ragged(*args(21, one, 0)) == TC_ERR_INVALID_ARGUMENT
    assert lib.tc_den_forward_backward_ragged(*args(21, C.c_void_p(18), 7)) == TC_ERR_INVALID_ARGUMENT  # misaligned lengths


def test_counter_and_header():
    assert lib.tc_debug_counter(b"ragged_steps") >= 0
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "torchain_hip.h")).read()
    for name in ("tc_supervision_create_e2e_ragged", "tc_supervision_frames", "tc_supervision_is_ragged",
                 "tc_den_forward_backward_ragged", '"ragged_steps"'):
        assert name in header, name


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_padding_geometry(name):
    lens = np.asarray(rc.lengths(name))
    S, T = len(lens), int(lens.max())
    pad = rc.padding_rows(lens)
    assert pad.shape == (S * T,) and pad.sum() == S * T - lens.sum()
    seen = np.zeros(S * T, bool)
    for s in range(S):
        rows = rc.valid_rows(lens, s)
        assert (rows % S == s).all() and (rows // S == np.arange(lens[s])).all()
        assert not pad[rows].any() and not seen[rows].any()
        seen[rows] = True
    assert (seen ^ pad).all()  # every row is one sequence's own frame or padding
    filled = rc.with_padding(rc.nnet_output(name), lens, np.nan)
    assert np.isnan(filled[pad]).all() and np.isfinite(filled[~pad]).all()


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_reference_is_feasible_and_zero_in_padding(name):
    want = rc.reference(name)
    lens = rc.lengths(name)
    assert want["ok"] == [True] * len(lens) and want["all_ok"]
    assert want["weight"] == pytest.approx(rc.WEIGHT * sum(lens), rel=1e-12)
    pad = rc.padding_rows(lens)
    assert not want["deriv"][pad].any() and not want["xent_deriv"][pad].any()
    assert want["deriv"][~pad].any()
    # the padding of y is not read: NaN there changes nothing
    again = rc.ragged_objective(rc.oracle_graph(), rc.fsts(name), lens, rc.with_padding(rc.nnet_output(name), lens, np.nan))
    assert again["objf"] == want["objf"] and np.array_equal(again["deriv"], want["deriv"])


def test_equal_lengths_sum_to_the_batch_reference():
    """The sum of single-sequence references is the batch reference.  The oracle returns each denominator log-prob as a
    float32, so objf -- a small difference of the numerator's and the denominator's totals -- agrees to a few float32
    roundings (6e-8 each) of those totals, not of itself: 1e-6 of the numerator's total is asked."""
    lens = rc.lengths("equal")
    want = rc.reference("equal")
    batch = ref.e2e_objective(rc.oracle_graph(), list(rc.fsts("equal")), lens[0], rc.nnet_output("equal"), weight=rc.WEIGHT,
                              l2=rc.L2, leaky=rc.LEAKY)
    assert batch["ok"]
    assert abs(want["objf"] - batch["objf"]) <= 1e-6 * rc.WEIGHT * float(np.abs(batch["logz"]).sum())
    for k in ("l2_term", "weight"):
        assert abs(want[k] - batch[k]) <= 1e-6 * abs(batch[k]), k
    assert np.abs(want["deriv"] - batch["deriv"]).max() <= 1e-6 * max(np.abs(batch["deriv"]).max(), rc.WEIGHT)


def test_chain_case_has_the_stated_shortest_paths_and_an_infeasible_length():
    arcs = [ref.shortest_path_arcs(f) for f in rc.fsts("chain")]
    assert all(a <= t for a, t in zip(arcs, rc.lengths("chain"))), arcs
    # one sequence given one frame fewer than its shortest path: the failure route, with Tmax larger
    lens = list(rc.lengths("chain"))
    lens[1] = arcs[1] - 1
    out = rc.ragged_objective(rc.oracle_graph(), rc.fsts("chain"), lens, rc.nnet_output("chain"))
    assert out["ok"][1] is False and not out["all_ok"]
    assert out["objf"] == -10.0 * out["weight"] and not out["xent_deriv"].any()
