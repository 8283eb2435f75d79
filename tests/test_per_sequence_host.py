"""The per-sequence report and the isolating step without a GPU (cases: ``tests/per_sequence_cases.py``): the numpy
restatement of the masked scalar epilogue against the CPU oracle, the conditions the GPU tests put on their inputs, keyword
validation, and the C entry's presence in header and library.

Tolerance: ``helpers.REL`` (1e-4 relative), what ``tests/test_gpu_objective.py`` holds the batch objective to."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from torchain_amd import functions, parallel
from torchain_amd._lib import LIB_PATH, lib

import e2e_reference as ref
import per_sequence_cases as ps
from helpers import REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "torchain_hip.h")


@pytest.mark.parametrize("name", ps.HEALTHY)
def test_every_fixture_is_healthy_but_for_the_sequence_the_tests_break(name):
    """The oracle finds every sequence of every case finite on its own, so the intended survivors (all but ``BAD[name]``)
    are B - 1 >= 4 sequences: no GPU test can pass by declaring everything failed."""
    rows = ps.oracle_rows(name)
    S = len(ps.lengths(name))
    assert rows.shape == (S, 3) and np.isfinite(rows).all(), rows
    survivors = [s for s in range(S) if s != ps.BAD[name]]
    assert len(survivors) == S - 1 >= 4 and 0 < ps.BAD[name] < S - 1
    if not ps.uniform(name):
        assert ps.lengths(name)[ps.BAD[name]] < max(ps.lengths(name))
    assert min(ps.lengths(name)) >= 2 and max(ps.lengths(name)) <= 24
    y = ps.nnet_output(name)
    assert y.shape == (max(ps.lengths(name)) * S, ps.P) and np.isfinite(y).all()
    for s in range(S):
        t, pdf = ps.carried_pdf(name, s)
        assert t == 1 and 0 <= pdf < ps.P and pdf != ps.uncarried_pdf(name, s)


@pytest.mark.parametrize("name", ps.HEALTHY)
def test_restatement_against_the_oracle(name):
    """The masked epilogue on the oracle's per-sequence values: with nothing masked the oracle's batch objective, with
    ``BAD[name]`` masked the oracle's objective of the surviving sub-batch; the weight is the float32 product."""
    rows = ps.oracle_rows(name)
    lens = np.asarray(ps.lengths(name))
    S, T = len(lens), int(lens.max())
    ragged = not ps.uniform(name)
    zero = np.zeros(S)
    everyone = list(range(S))
    survivors = [s for s in everyone if s != ps.BAD[name]]
    for keep, isolate in ((everyone, False), (everyone, True), (survivors, True)):
        status = np.zeros(S, np.int64)
        if len(keep) < S:
            status[ps.BAD[name]] = ps.STATUS_NUM
        out = ps.finalize(rows[:, 0], rows[:, 1], rows[:, 2], zero, lens, ps.WEIGHT, ps.L2, T, ragged, isolate, status=status)
        want = ps.oracle_objective(name, keep)
        r = out["results"]
        print("%s keep %s: objf %.9g (oracle %.9g) l2 %.9g (%.9g) weight %.9g (%.9g)" % (name, keep, r[0], want["objf"], r[1],
                                                                                        want["l2_term"], r[2], want["weight"]))
        assert out["fail"] == 0 and out["masked"] == (len(keep) < S)
        assert abs(r[0] - want["objf"]) <= REL * abs(want["objf"])
        assert abs(r[1] - want["l2_term"]) <= REL * abs(want["l2_term"])
        assert abs(r[2] - want["weight"]) <= REL * want["weight"]
        assert r[2] == np.float32(ps.WEIGHT) * np.float32(lens[keep].sum()) or ps.uniform(name)
        assert abs(float(out["loss"]) + float(r[0]) / float(r[2])) <= 1e-6 * abs(float(out["loss"]))
        assert list(out["alive_frames"]) == [int(lens[s]) if s in keep else 0 for s in everyone]


def test_restatement_rule_and_special_cases():
    """Status bits by the rule (non-finite = ``x - x != 0``), an exact +0.0 for a masked term, and the three special cases:
    nothing failed and everything failed give the unmasked call; survivors that miss the sum check give it too."""
    num = np.array([-10.0, -np.inf, -12.0, np.nan, -9.0])
    den = np.array([-8.0, -7.0, np.nan, -6.0, -5.0])
    y2 = np.array([3.0, 4.0, np.inf, 5.0, 6.0])
    xent = np.array([0.5, 0.25, 0.125, 1.0, np.nan])
    assert list(ps.status_bits(num, den, y2, xent)) == [0, 1, 2, 1, 1]
    assert list(ps.status_bits(num, den, y2, xent, ab=np.array([1.0, 1, 1, 1, np.nan]), gs=np.ones(5))) == [0, 1, 2, 1, 5]
    frames = np.array([4, 5, 6, 7, 8])
    # one survivor: its own objective
    out = ps.finalize(num, den, y2, xent, frames, 0.5, 1e-3, 8, True, True)
    assert out["masked"] and out["fail"] == 0 and list(out["alive_frames"]) == [4, 0, 0, 0, 0]
    assert out["results"][0] == np.float32(0.5 * -10.0) - np.float32(0.5) * np.float32(-8.0)
    assert out["results"][2] == np.float32(0.5) * np.float32(4) and out["xent"] == 0.5
    # the switch off: the whole minibatch fails, every sequence keeps its frames
    off = ps.finalize(num, den, y2, xent, frames, 0.5, 1e-3, 8, True, False)
    assert off["fail"] == 1 and not off["masked"] and list(off["alive_frames"]) == list(frames)
    assert off["results"][0] == np.float32(-10.0) * (np.float32(0.5) * np.float32(30)) and off["xent"] == 0.0
    # survivors that miss the sum check: as the switch off
    missed = ps.finalize(num, den, y2, xent, frames, 0.5, 1e-3, 8, True, True, survivors_ok=False)
    assert all(np.array_equal(missed[k], off[k]) for k in ("results", "alive_frames")) and missed["fail"] == 1
    # everything failed
    nothing = ps.finalize(np.full(3, -np.inf), den[:3], y2[:3], xent[:3], frames[:3], 0.5, 0.0, 8, False, True)
    plain = ps.finalize(np.full(3, -np.inf), den[:3], y2[:3], xent[:3], frames[:3], 0.5, 0.0, 8, False, False)
    assert nothing["fail"] == 1 and not nothing["masked"] and np.array_equal(nothing["results"], plain["results"])
    assert nothing["results"][2] == np.float32(0.5) * np.float32(3) * np.float32(8)  # a uniform handle's weight
    # nothing failed: bit for bit the switch off
    ok = [np.array([-10.0, -11.0]), np.array([-8.0, -7.5]), np.array([3.0, 4.0]), np.zeros(2), np.array([8, 8])]
    a, b = ps.finalize(*ok, 0.7, 5e-4, 8, False, True), ps.finalize(*ok, 0.7, 5e-4, 8, False, False)
    assert a["results"].tobytes() == b["results"].tobytes() and not a["masked"] and a["fail"] == 0
    # a negative zero cannot come from a masked term: +0.0 + x == x, and the sum of masked terms alone is +0.0
    assert np.signbit(ps._ordered_sum([-0.0, 5.0], [False, True])) == np.signbit(5.0)
    assert not np.signbit(ps._ordered_sum([-3.0, -0.0], [False, False]))


def test_the_no_path_fst_has_no_path():
    for T in (2, 3, 7):
        fst = ps.no_path_fst(T)
        assert ref.shortest_path_arcs(fst) == T + 2
        y = np.zeros((T, ps.P))
        assert ref.num_logz([fst], y, T, want_gamma=False)[0][0] == -np.inf
        assert np.isfinite(ref.num_logz([fst], np.zeros((T + 2, ps.P)), T + 2, want_gamma=False)[0][0])


def test_keywords_are_checked_before_any_library_call():
    """``on_failure`` is "minibatch" or "sequence"; anything else is a ValueError raised in front of everything else (CPU
    tensors and a graph that is none reach no further check).  ``on_failure="sequence"`` implies the report."""
    x = torch.zeros(4, 3)
    for bad in ("utterance", "", None, 1, "Sequence"):
        for fn in (functions.chain_loss, parallel.chain_loss_data_parallel):
            with pytest.raises(ValueError, match="on_failure"):
                fn(x, None, None, on_failure=bad)
    with pytest.raises(ValueError, match="per_sequence"):
        functions.chain_loss(x, None, None, per_sequence="yes")
    with pytest.raises(TypeError, match="unexpected keyword"):
        functions.chain_loss(x, None, None, per_sequences=True)
    assert functions._failure_options({}) == (False, False)
    assert functions._failure_options({"per_sequence": True}) == (True, False)
    assert functions._failure_options({"on_failure": "sequence"}) == (True, True)
    assert functions._failure_options({"on_failure": "minibatch", "per_sequence": False}) == (False, False)
    rest = {"on_failure": "sequence", "out_of_range_regularize": 0.5}
    assert functions._failure_options(rest) == (True, True) and rest == {"out_of_range_regularize": 0.5}
    res = functions.ChainResults()
    assert res.per_sequence is None and res.failed is None


def test_per_sequence_object():
    rows = torch.tensor([[-10.0, -8.0, 3.0, 0.5, 7.0, 0.0], [float("-inf"), -7.0, 4.0, 0.0, 3.0, 1.0]], dtype=torch.float64)
    seq = functions.PerSequence(rows, 0.5)
    assert len(seq) == 2 and seq.status.tolist() == [0, 1] and seq.status.dtype == torch.int64
    assert seq.objf[0].item() == 0.5 * (-10.0 + 8.0) and seq.objf[1].item() == float("-inf")
    assert seq.frames.tolist() == [7.0, 3.0] and seq.num_logprob.dtype == torch.float64
    res = functions.ChainResults()
    res._seq_host = seq
    assert res.failed.tolist() == [1]


def test_header_declares_and_library_exports_the_entry():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int tc_chain_step_per_sequence\((.*?)\);", code, flags=re.S)
    assert m, "tc_chain_step_per_sequence is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    strided = [p.strip() for p in re.search(r"int tc_chain_step_strided\((.*?)\);", code, flags=re.S).group(1).split(",")]
    assert params[:len(strided)] == strided and params[len(strided):] == ["int isolate_failures", "double *seq_results_dev"]
    assert hasattr(C.CDLL(LIB_PATH), "tc_chain_step_per_sequence")
    assert len(lib.tc_chain_step_per_sequence.argtypes) == len(lib.tc_chain_step_strided.argtypes) + 2
    doc = text[:text.index("int tc_chain_step_per_sequence(")].rsplit("/*", 1)[1]
    for word in ("seq_results_dev", "isolate_failures", "status", "stream capture", "DESIGN.md 4.13"):
        assert word in doc, word
