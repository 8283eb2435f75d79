"""The element-wise check of the numerators' posteriors (``helpers.posteriors_elementwise``) on the host, no GPU: it accepts what
is right to the precision of the formats, it rejects an occupation that is lost or lands on the wrong pdf, and the matrix-wise
``rel_err(..., floor=weight) <= REL`` that the suite relied on before accepts both.  The tolerances of the GPU test
(``tests/num_elementwise_cases.py``) are tied to two things that can be reproduced here: the CPU oracle's numerator and the
end-to-end kernel's arithmetic restated in numpy (``e2e_reference.kernel_arithmetic``)."""
import numpy as np
import pytest

import e2e_reference as e2e
import num_elementwise_cases as nc
from helpers import REL, posteriors_elementwise, rel_err


@pytest.mark.parametrize("scale", nc.SCALES)
@pytest.mark.parametrize("name", ["lattice_fits", "trie_150x40"])
def test_checker_accepts_the_oracle_numerator(oracle, name, scale):
    sup, y, want_lp, ref = nc.regular_case(name, scale)
    got = oracle.num_forward_backward(sup, y)
    assert abs(got["logprob_weighted"] - want_lp) <= nc.REL_LOGPROB * abs(want_lp)
    worst = posteriors_elementwise(got["deriv"], ref, sup.weight, "%s scale %g (CPU oracle)" % (name, scale), nc.REL_REGULAR)
    assert max(worst.values()) <= nc.REL_REGULAR / 2  # (the tolerance leaves the kernels room beyond the oracle's own distance)


def _spoiled():
    """float64 posteriors of lattice_fits as float32, and two spoiled copies: an entry of 1e-6 .. 1e-5 lost, and one moved to a
    pdf that no arc of its frame carries."""
    sup, _, _, ref = nc.regular_case("lattice_fits", 1.0)
    good = ref.astype(np.float32)
    rows, cols = np.nonzero((ref > 1e-6) & (ref < 1e-5))
    assert len(rows) >= 2
    lost = good.copy()
    lost[rows[0], cols[0]] = 0.0
    moved = good.copy()
    r, c = rows[1], cols[1]
    empty = int(np.flatnonzero(ref[r] == 0)[0])
    moved[r, empty], moved[r, c] = moved[r, c], 0.0
    return sup, ref, good, lost, moved


def test_checker_rejects_a_lost_and_a_misplaced_occupation():
    sup, ref, good, lost, moved = _spoiled()
    posteriors_elementwise(good, ref, sup.weight, "float64 rounded to float32", nc.REL_REGULAR)
    with pytest.raises(AssertionError, match="worst relative error 1 "):
        posteriors_elementwise(lost, ref, sup.weight, "an occupation lost", nc.REL_REGULAR)
    with pytest.raises(AssertionError):
        posteriors_elementwise(moved, ref, sup.weight, "an occupation on the wrong pdf", nc.REL_REGULAR)
    # the wrong pdf alone (the right entry kept) is caught by the exact-zero rule
    r, c = np.argwhere((lost != good))[0]
    stray = good.copy()
    stray[r, int(np.flatnonzero(ref[r] == 0)[0])] = 1e-12
    with pytest.raises(AssertionError, match="non-zero where no arc"):
        posteriors_elementwise(stray, ref, sup.weight, "a stray occupation", nc.REL_REGULAR)


def test_the_matrix_wise_rule_accepts_both():
    """The hole: max |diff| <= 1e-4 * max(max |ref|, weight) is an absolute 1e-4 on numbers in [0, 1]."""
    sup, ref, good, lost, moved = _spoiled()
    for spoiled in (lost, moved):
        assert not np.array_equal(spoiled, good)
        assert rel_err(spoiled, ref, floor=sup.weight) <= REL


@pytest.mark.parametrize("scale", nc.E2E_SCALES)
@pytest.mark.parametrize("name", tuple(nc.E2E))
def test_checker_accepts_the_e2e_kernel_arithmetic(name, scale):
    """The kernel's arithmetic in numpy (everything but the device's exp) lies within the GPU test's tolerance of float64, with
    room to spare up to 150 frames."""
    fsts, T, P, y, want_lp, ref = nc.e2e_case(name, scale)
    S = len(fsts)
    got, logz = np.zeros(ref.shape, np.float32), 0.0
    for s, fst in enumerate(fsts):
        z, got[s::S] = e2e.kernel_arithmetic(fst, y[s::S], nc.E2E_WEIGHT)
        logz += z
    assert abs(nc.E2E_WEIGHT * logz - want_lp) <= nc.REL_LOGPROB * abs(want_lp)
    worst = posteriors_elementwise(got, ref, nc.E2E_WEIGHT, "%s scale %g (restated arithmetic)" % (name, scale), nc.e2e_rel(name))
    if name in nc.E2E_SHORT:
        assert max(worst.values()) <= nc.REL_E2E / 2
