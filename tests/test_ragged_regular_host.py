"""Ragged regular supervisions without a GPU: the handle of tc_supervision_create_ragged (its lengths, the longest as
num_frame, is_ragged and not is_e2e), its tables against the uniform entry's (tc_supervision_stats), every refusal with its
error code, the Python layer (io.Supervision.from_fsts / from_sequences) and the references of tests/ragged_regular_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

from torchain_amd import egs, io, synth
from torchain_amd._lib import TorchainHipError, lib

import num_elementwise_cases as nc
import ragged_cases as rc
import ragged_regular_cases as rr
import wide_supervisions as ws

TC_ERR_INVALID_ARGUMENT, TC_ERR_BAD_FST, TC_ERR_UNSUPPORTED = -1, -2, -3


def _fsts(pieces):
    return [(p.arc_begin, p.ilabel, p.arc_weight, p.nextstate, p.final) for p in pieces]


def _create(pieces, lens, weight=1.0, label_dim=None):
    """tc_supervision_create_ragged itself; returns (code, handle)"""
    arrays = rr.concatenated(pieces)
    frames = np.ascontiguousarray(lens, np.int32)
    handle = C.c_void_p()
    code = lib.tc_supervision_create_ragged(C.byref(handle), weight, len(pieces), frames.ctypes.data_as(C.c_void_p),
                                            pieces[0].label_dim if label_dim is None else label_dim,
                                            *[a.ctypes.data_as(C.c_void_p) for a in arrays])
    return code, handle


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_handle_reports_lengths_and_longest(name):
    lens = rr.lengths(name)
    sup = rr.handle(name)
    assert sup.is_ragged and not sup.is_e2e  # (also when all lengths are equal)
    assert sup.frames.dtype == np.int32 and tuple(sup.frames) == lens
    assert sup.n_frame == max(lens) == lib.tc_supervision_num_frame(sup.ptr)
    assert sup.shape == (len(lens), max(lens), rr.num_pdfs(name))
    assert sup.weight == np.float32(rr.weight(name))
    st = sup.stats()
    assert st["sequences"] == len(lens) and st["frames"] == max(lens)


def test_eight_is_eight_sequences_the_longest_last():
    assert rr.EIGHT == (1, 6, 11, 5, 10, 4, 9, 11) and len(rr.EIGHT) == 8


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_stats_are_the_largest_single_sequences(name):
    """The builder is the uniform entry's: a batch's maxima are the maxima over its sequences' own single-sequence handles, and
    its history the sum."""
    st = rr.handle(name).stats()
    singles = [io.Supervision.from_synth(p).stats() for p in rr.pieces(name)]
    for key in ("max_states", "max_arcs", "max_uniq", "max_level_states", "max_level_arcs", "max_frame_uniq",
                "resident_lds_bytes", "windowed_lds_bytes"):
        assert st[key] == max(s[key] for s in singles), key
    assert st["history_bytes"] == sum(s["history_bytes"] for s in singles)


def test_equal_lengths_build_the_merged_uniform_handles_tables():
    pieces = rr.pieces("equal")
    ragged = io.Supervision.from_sequences(pieces)
    uniform = io.Supervision.from_synth(egs.append_supervisions(list(pieces)))
    assert ragged.is_ragged and not uniform.is_ragged
    assert ragged.stats() == uniform.stats()
    assert ragged.stats() == {**ws.count_stats(egs.append_supervisions(list(pieces))), "route": 0}


def test_wide_takes_the_windowed_kernel_and_trie_the_unstaged_resident_one():
    wide = rr.handle("wide").stats()
    assert wide["kernel"] == "windowed" and wide["resident_lds_bytes"] > ws.LDS_LIMIT
    # ... because of its longest sequence: the 31-frame one alone fits the resident kernel
    assert io.Supervision.from_synth(rr.pieces("wide")[1]).stats()["kernel"] == "resident"
    trie = rr.handle("trie").stats()
    assert trie["kernel"] == "resident" and not nc.staged_in_lds(trie)
    small = rr.handle("small").stats()
    assert small["kernel"] == "resident" and nc.staged_in_lds(small)


# ---- the refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [(7, 0, 4, 2, 7), (7, -3, 4, 2, 7), (0, 0, 0, 0, 0)])
def test_a_length_below_one_is_refused(bad):
    with pytest.raises(TorchainHipError) as e:
        io.Supervision.from_fsts(1.0, list(bad), rr.P, _fsts(rr.pieces("small")))
    assert e.value.code == TC_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("lens", [(7, 2, 4, 2, 7), (6, 1, 4, 2, 7), (7, 1, 4, 2, 8)])
def test_a_sequence_of_another_length_than_its_paths_is_refused(lens):
    with pytest.raises(TorchainHipError) as e:
        io.Supervision.from_fsts(1.0, list(lens), rr.P, _fsts(rr.pieces("small")))
    assert e.value.code == TC_ERR_BAD_FST


def _replace(piece, **fields):
    return piece._replace(**fields)


def test_paths_of_unequal_length_in_one_sequence_are_refused():
    """A second final state one level early: the sequence's paths are 3 and 4 arcs long."""
    piece = rr.pieces("small")[2]  # 4 frames
    final = np.array(piece.final, copy=True)
    times = ws.state_times(piece)
    early = int(np.flatnonzero(times == 3)[0])
    final[early] = 0.5
    bad = _replace(piece, final=final)
    code, _ = _create([bad], [4])
    assert code == TC_ERR_BAD_FST
    code, _ = _create([bad], [3])
    assert code == TC_ERR_BAD_FST


@pytest.mark.parametrize("label", [0, rr.P + 1])
def test_a_label_outside_the_pdfs_is_refused(label):
    pieces = list(rr.pieces("small"))
    il = np.array(pieces[3].ilabel, copy=True)
    il[-1] = label
    pieces[3] = _replace(pieces[3], ilabel=il)
    code, _ = _create(pieces, rr.lengths("small"))
    assert code == TC_ERR_BAD_FST
    # the same label is fine when label_dim allows it
    if label:
        code, handle = _create(pieces, rr.lengths("small"), label_dim=rr.P + 1)
        assert code == 0
        lib.tc_supervision_free(handle)


def test_states_out_of_time_order_are_refused():
    """Two states of different levels exchange their numbers: the same acceptor, no longer numbered in time order."""
    piece = rr.pieces("small")[0]  # 7 frames
    times = ws.state_times(piece)
    a, b = int(np.flatnonzero(times == 2)[0]), int(np.flatnonzero(times == 4)[0])
    perm = np.arange(piece.num_states)
    perm[a], perm[b] = b, a  # new id of old state i
    order = np.argsort(perm)  # old state at new position j
    deg = np.diff(piece.arc_begin)
    arc_begin = np.concatenate([[0], np.cumsum(deg[order])]).astype(np.int32)
    idx = np.concatenate([np.arange(piece.arc_begin[o], piece.arc_begin[o + 1]) for o in order]).astype(np.int64)
    bad = _replace(piece, arc_begin=arc_begin, ilabel=piece.ilabel[idx], arc_weight=piece.arc_weight[idx],
                   nextstate=perm[piece.nextstate[idx]].astype(np.int32), final=piece.final[order])
    code, _ = _create([bad], [7])
    assert code == TC_ERR_BAD_FST
    code, handle = _create([piece], [7])
    assert code == 0
    lib.tc_supervision_free(handle)


def test_a_next_state_of_another_sequence_is_refused():
    pieces = list(rr.pieces("small"))
    nx = np.array(pieces[1].nextstate, copy=True)  # the one-frame sequence: 2 to 4 states
    nx[0] = pieces[1].num_states
    pieces[1] = _replace(pieces[1], nextstate=nx)
    code, _ = _create(pieces, rr.lengths("small"))
    assert code == TC_ERR_BAD_FST


def test_size_limits_use_the_longest_length():
    """S * Tmax <= 2^26, whatever the sum of the lengths is."""
    pieces = rr.pieces("small")[:2]
    with pytest.raises(TorchainHipError) as e:
        io.Supervision.from_fsts(1.0, [(1 << 25) + 1, 1], rr.P, _fsts(pieces))
    assert e.value.code == TC_ERR_UNSUPPORTED


def test_a_history_beyond_four_gib_is_refused():
    """One double per state: 2^29 + 1 states.  The entry refuses by seq_state_begin alone, before it reads a state, so the arrays
    behind it can be small here."""
    handle = C.c_void_p()
    frames, sb = np.array([5], np.int32), np.array([0, (1 << 29) + 1], np.int32)
    small = np.zeros(4, np.int32)
    fl = np.zeros(4, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.tc_supervision_create_ragged(C.byref(handle), 1.0, 1, p(frames), rr.P, p(sb), p(small), p(small), p(fl), p(small),
                                            p(fl)) == TC_ERR_UNSUPPORTED
    assert not handle


def test_python_argument_checks():
    fsts = _fsts(rr.pieces("small"))
    with pytest.raises(ValueError):
        io.Supervision.from_fsts(1.0, [7, 1, 4], rr.P, fsts)  # not one length per sequence
    with pytest.raises(ValueError):
        io.Supervision.from_fsts(1.0, 7, rr.P, fsts)  # a single length: from_fst's business
    with pytest.raises(ValueError):
        io.Supervision.from_fsts(1.0, [7.5, 1, 4, 2, 7], rr.P, fsts)
    with pytest.raises(ValueError):
        io.Supervision.from_fsts(1.0, [], rr.P, [])
    short = list(fsts)
    short[2] = (short[2][0], short[2][1][:-1]) + short[2][2:]
    with pytest.raises(ValueError):
        io.Supervision.from_fsts(1.0, [7, 1, 4, 2, 7], rr.P, short)
    assert lib.tc_supervision_create_ragged(None, 1.0, 1, None, rr.P, None, None, None, None, None, None) == TC_ERR_INVALID_ARGUMENT


def test_from_sequences_wants_single_sequences_of_one_weight_and_label_dim():
    pieces = rr.pieces("small")
    two = synth.random_supervision(ws.den_fst(), 2, 4, 3, seed=1)
    with pytest.raises(ValueError):
        io.Supervision.from_sequences([pieces[0], two])
    with pytest.raises(ValueError):
        io.Supervision.from_sequences([pieces[0], synth.random_supervision(ws.den_fst(), 1, 4, 3, seed=1, weight=0.5)])
    with pytest.raises(ValueError):
        io.Supervision.from_sequences([pieces[0], rr.pieces("eight")[0]])  # label_dim 100
    with pytest.raises(ValueError):
        io.Supervision.from_sequences([])
    # the merge keeps refusing unequal lengths: a merged supervision has one
    with pytest.raises(egs.EgsFormatError):
        egs.append_supervisions(list(pieces))


def test_uniform_handles_are_untouched():
    sup = io.Supervision.from_synth(synth.random_supervision(ws.den_fst(), 3, 6, 2, seed=1))
    assert not sup.is_ragged and not sup.is_e2e and tuple(sup.frames) == (6, 6, 6)


def test_header_names():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "torchain_hip.h")).read()
    assert "int tc_supervision_create_ragged(tc_supervision **out, float weight, int32_t num_sequences," in header
    for name in ("frames_per_sequence", "seq_state_begin"):
        assert name in header.split("int tc_supervision_create_ragged(")[1].split(";")[0], name
    assert hasattr(io.Supervision, "from_fsts") and hasattr(io.Supervision, "from_sequences")


# ---- the references --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "equal"])
def test_numerator_reference_rows_sum_to_the_weight_and_padding_is_zero(name):
    lens = rr.lengths(name)
    lp, post = rr.num_reference(name)
    pad = rc.padding_rows(lens)
    assert np.isfinite(lp) and not post[pad].any()
    assert np.abs(post[~pad].sum(axis=1) / rr.weight(name) - 1.0).max() <= 1e-12


def test_objective_reference_sums_the_sequences():
    lens = rr.lengths("small")
    want = rr.reference("small")
    assert want["weight"] == pytest.approx(rr.weight("small") * sum(lens), rel=1e-6)
    pad = rc.padding_rows(lens)
    assert not want["deriv"][pad].any() and not want["xent_deriv"][pad].any() and want["deriv"][~pad].any()
    # the padding of y is not read
    again = rr.ragged_objective(rr.oracle_graph("small"), rr.pieces("small"), lens,
                                rc.with_padding(rr.nnet_output("small"), lens, np.nan))
    assert again["objf"] == want["objf"] and np.array_equal(again["deriv"], want["deriv"])


def test_equal_lengths_sum_to_the_merged_batchs_objective(oracle):
    """The sum of the single-sequence objectives is the merged batch's.  The oracle returns float32 totals: a few roundings of
    the numerator's and the denominator's totals, 1e-5 of their magnitude, is asked of objf (a small difference of the two)."""
    lens = rr.lengths("equal")
    pieces = rr.pieces("equal")
    want = rr.reference("equal")
    merged = egs.append_supervisions(list(pieces))
    y = rr.nnet_output("equal")
    batch = oracle.compute_chain_objf_and_deriv(rr.oracle_graph("equal"), merged, y, rr.L2, rr.LEAKY, want_xent=True)
    scale = abs(oracle.num_forward_backward(merged, y, want_deriv=False)["logprob_weighted"])
    assert abs(want["objf"] - batch["objf"]) <= 1e-5 * max(scale, abs(batch["objf"]))
    assert want["weight"] == batch["weight"] == len(lens) * lens[0]
    assert np.abs(want["deriv"] - batch["deriv"]).max() <= 1e-5
    assert np.abs(want["xent_deriv"] - batch["xent_deriv"]).max() <= 1e-5
