"""Ragged batches on two workgroups per sequence, without a GPU: the cases' float64 references are feasible for every
sequence (so that a failure on the GPU is the kernel's), the counter exists and the header documents it."""
import os

import numpy as np
import pytest

from torchain_amd._lib import lib

import ragged_cases as rc
import ragged_two_cu_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lengths_cover_the_edge_cases():
    lens = tc.LENGTHS
    assert len(lens) == 8 and {1, 2, 3} <= set(lens)
    assert any(t % 2 for t in lens) and any(t % 2 == 0 for t in lens)
    assert lens.index(max(lens)) != len(lens) - 1 and len(set(lens)) < len(lens)


@pytest.mark.parametrize("form", sorted(tc.FORMS))
def test_den_reference_is_ok_for_every_sequence(form):
    graph = tc.FORMS[form].graph
    lp, d = tc.den_reference(graph)  # (ragged_cases.den_reference asserts the oracle's ok per sequence)
    pad = rc.padding_rows(tc.LENGTHS)
    assert np.isfinite(lp) and np.isfinite(d).all()
    assert not d[pad].any() and d[~pad].any()
    # [K]: the occupations of a frame sum to one
    np.testing.assert_allclose(d[~pad].sum(axis=1), tc.DERIV_WEIGHT, rtol=1e-4)


def test_boundary_reference_is_ok_for_every_sequence():
    lens = tc.boundary_lengths(129)
    assert set(lens) == {1, 2, 3, 4, 5}
    lp, d = tc.den_reference("tied8", lens)
    assert np.isfinite(lp) and not d[rc.padding_rows(lens)].any()


@pytest.mark.parametrize("bfloat16", [False, True])
def test_step_reference_is_ok_for_every_sequence(bfloat16):
    want = tc.step_reference(bfloat16)
    assert want["ok"] == [True] * tc.S and want["all_ok"]
    assert want["weight"] == pytest.approx(rc.WEIGHT * sum(tc.LENGTHS), rel=1e-12)
    pad = rc.padding_rows(tc.LENGTHS)
    assert not want["deriv"][pad].any() and want["deriv"][~pad].any()


def test_counter_and_header():
    assert lib.tc_debug_counter(b"ragged_two_cu_launches") >= 0
    header = open(os.path.join(ROOT, "include", "torchain_hip.h")).read()
    assert '"ragged_two_cu_launches"' in header
