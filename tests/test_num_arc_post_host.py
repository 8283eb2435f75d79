"""The float64 reference of the arc occupations (``tests/num_arc_post_reference.py``) against itself, without a GPU: the
recursion equals the list of paths, the counts add up, and they are the derivative of ``log Z`` in the arc costs."""
import numpy as np

import e2e_reference as e2e
import num_arc_post_reference as apr
import num_entropy_reference as ner


def test_recursion_equals_enumeration_on_the_tiny_fst():
    y = np.random.default_rng(3).normal(0.0, 2.0, size=(4, 4))
    a, b = apr.by_recursion(ner.tiny_fst(), y), apr.by_enumeration(ner.tiny_fst(), y)
    assert all(np.abs(a[k] - b[k]).max() <= 1e-12 for k in ("arcs", "finals", "logprob")) and a["arcs"].max() > 0.5


def test_counts_add_up_and_are_the_derivative_of_log_z():
    rng, T = np.random.default_rng(4), 6
    fst = e2e.random_fst(9, 30, 7, rng)
    y, cost = rng.normal(0.0, 2.0, size=(T, 7)), np.asarray(fst[3], np.float64)
    got = apr.by_recursion(fst, y)
    assert abs(got["arcs"].sum() - T) <= 1e-12 * T and abs(got["finals"].sum() - 1) <= 1e-12
    h = 1e-5  # central difference of log Z in -cost: error h^2 * |third derivative| / 6 of a function with derivatives O(T)
    for a in range(len(cost)):
        lz = [apr.by_recursion(fst, y, cost - s * h * (np.arange(len(cost)) == a))["logprob"] for s in (1, -1)]
        assert abs((lz[0] - lz[1]) / (2 * h) - got["arcs"][a]) <= 1e-8
