"""The three numerator kernels' posteriors, entry by entry against float64 (``helpers.posteriors_elementwise``): the resident
kernel (``csrc/num_kernels.hip``), the level-windowed one (``csrc/num_windowed_kernels.hip``) and the end-to-end one
(``csrc/num_e2e_kernels.hip``).  Cases, references and tolerances are those of ``tests/num_elementwise_cases.py``.

Every case reads the posteriors three ways: from ``tc_num_forward_backward`` into a zeroed matrix, and as ``xent_deriv`` of
``compute_chain_objf_and_deriv`` in the default order (beside the denominator: staged, then scattered) and in line
(``no_num_overlap``).  A run into a matrix of a sentinel shows that an entry no arc carries is not touched (``deriv`` is ``+=``),
the sentinel the ``xent_deriv`` matrices start from that such an entry is written as 0.  Every case prints which kernel ran and
the worst relative error per magnitude class (``-s``; one run is kept in ``profiles/num_elementwise/worst_errors.txt``)."""
import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import ChainResults, compute_chain_objf_and_deriv

import num_elementwise_cases as nc
import wide_supervisions as ws
from helpers import hip_num, posteriors_elementwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 3.0
_cache = {}


def _counters():
    return {k: int(lib.tc_debug_counter(k.encode())) for k in ("num_launches", "num_windowed_launches", "num_e2e_staged_launches")}


def _since(before):
    return {k: v - before[k] for k, v in _counters().items()}


def _graph(P):
    """A denominator graph with P pdfs for the calls of the whole objective (the regular cases: the supervisions' own)."""
    if P not in _cache:
        fst = ws.den_fst() if P == ws.P else synth.random_den_fst(80, 4, P, seed=31)
        _cache[P] = io.DenominatorGraph(fst, P).prepare(0)
    return _cache[P]


def _xent_deriv(hsup, y):
    """xent_deriv of the whole objective, into a matrix that held 7 everywhere; not the soft-failure route."""
    yt = torch.from_numpy(y).to(DEV)
    deriv, xd = torch.full(yt.shape, 7.0, device=DEV), torch.full(yt.shape, 7.0, device=DEV)
    res = ChainResults()
    compute_chain_objf_and_deriv(_graph(y.shape[1]), hsup, yt, res.data, deriv, xd, 0.0, 0.1, 0.1)
    torch.cuda.synchronize()
    r = res.data.numpy()
    assert np.isfinite(r).all() and r[0] != np.float32(-10.0) * r[2], r
    return xd.cpu().numpy()


def _check(what, hsup, y, weight, want_lp, ref, rel, kernel_family, windowed, e2e=False):
    """The comparisons of the module's docstring for one case; ``windowed``: whether the level-windowed kernel must run."""
    before = _counters()
    out = hip_num(hsup, y)
    fwd = hip_num(hsup, y, want_deriv=False)
    kept = hip_num(hsup, y, init=SENTINEL)
    ran = _since(before)
    print("%s: %s" % (what, ran))
    assert ran["num_launches"] == 3 and ran["num_windowed_launches"] == (3 if windowed else 0), ran
    assert ran["num_e2e_staged_launches"] == 0
    lp_err = abs(out["logprob_weighted"] - want_lp) / abs(want_lp)
    print("%s: log-prob %.9g (float64 %.9g), relative error %.2e" % (what, out["logprob_weighted"], want_lp, lp_err))
    assert lp_err <= nc.REL_LOGPROB
    assert fwd["logprob_weighted"] == out["logprob_weighted"] and fwd["deriv"] is None
    assert kept["logprob_weighted"] == out["logprob_weighted"]
    posteriors_elementwise(out["deriv"], ref, weight, what + " [tc_num_forward_backward]", rel)
    # deriv is +=: an entry no arc carries keeps what it held, the others moved (those large enough to show beside 3)
    assert np.all(kept["deriv"][ref == 0] == np.float32(SENTINEL)), what
    assert np.all(kept["deriv"][ref > 1e-3 * weight] > np.float32(SENTINEL)), what
    for route, serial in (("beside the denominator", 0), ("in line", 1)):
        kernel_family("no_num_overlap", serial)
        before = _counters()
        xd = _xent_deriv(hsup, y)
        ran = _since(before)
        print("%s: xent_deriv %s: %s" % (what, route, ran))
        assert ran["num_launches"] == 1 and ran["num_windowed_launches"] == (1 if windowed else 0), ran
        if e2e:  # (these batches leave most CUs idle: the default order stages the posteriors for the scatter kernel)
            assert ran["num_e2e_staged_launches"] == (0 if serial else 1), ran
        posteriors_elementwise(xd, ref, weight, "%s [xent_deriv %s]" % (what, route), rel)
        assert np.array_equal(xd, out["deriv"]), (what, route)  # (one value, three ways to it)


def _regular(name, scale, kernel_family, expect, forced=False):
    sup, y, want_lp, ref = nc.regular_case(name, scale)
    hsup = io.Supervision.from_synth(sup)
    st = hsup.stats()
    print("%s scale %g: %s, tables in LDS: %s" % (name, scale, st, nc.staged_in_lds(st)))
    assert st["kernel"] == expect, st
    if forced:
        kernel_family("force_num_windowed", 1)
        assert hsup.stats()["kernel"] == ws.WINDOWED
    if scale >= 8.0:
        assert np.abs(y).max() > 30.0
    _check("%s scale %g" % (name, scale), hsup, y, sup.weight, want_lp, ref, nc.REL_REGULAR, kernel_family,
           windowed=forced or expect == ws.WINDOWED)
    return st


@pytest.mark.parametrize("scale", nc.SCALES)
@pytest.mark.parametrize("name", nc.RESIDENT)
def test_resident_kernel(kernel_family, name, scale):
    st = _regular(name, scale, kernel_family, ws.RESIDENT)
    # the two forms of the resident kernel: tables in LDS for the small ones, read from global memory otherwise
    assert nc.staged_in_lds(st) == (name == "trie_150x3" or name in nc.SINGLE_PATH), st
    if name == "lattice_edge":  # (arcs and unique (frame, pdf) entries of a sequence: several passes of 128 and a partial one)
        count = ws.count_stats(nc.regular_supervision(name))
        for key in ("max_arcs", "max_uniq"):
            assert count[key] == st[key] and count[key] > 2 * 128 and count[key] % 128 != 0, (key, count)
        assert count["max_level_states"] == 129


@pytest.mark.parametrize("scale", nc.SCALES)
@pytest.mark.parametrize("name", nc.WINDOWED)
def test_windowed_kernel(kernel_family, name, scale):
    _regular(name, scale, kernel_family, ws.WINDOWED)


@pytest.mark.parametrize("scale", nc.SCALES)
@pytest.mark.parametrize("name", nc.FORCED)
def test_windowed_kernel_forced_on_a_supervision_that_fits(kernel_family, name, scale):
    _regular(name, scale, kernel_family, ws.RESIDENT, forced=True)


@pytest.mark.parametrize("scale", nc.E2E_SCALES)
@pytest.mark.parametrize("name", tuple(nc.E2E))
def test_e2e_kernel(kernel_family, name, scale):
    fsts, T, P, y, want_lp, ref = nc.e2e_case(name, scale)
    print("%s scale %g: end-to-end kernel, %d sequences of %d frames; states %s, arcs %s, distinct pdfs %s, starts %s" % (
        name, scale, len(fsts), T, [len(f[5]) for f in fsts], [int(f[1][-1]) for f in fsts],
        [len(set(f[2].tolist())) for f in fsts], [f[0] for f in fsts]))
    if scale >= 8.0:
        assert np.abs(y).max() > 30.0
    if name == "start_and_unreachable":
        assert all(f[0] != 0 for f in fsts)
        assert not ref[:, [53, 57]].any() and all(np.isin([54, 58], f[2]).all() for f in fsts)
    hsup = io.Supervision.from_e2e_fsts(nc.E2E_WEIGHT, T, P, fsts)
    assert hsup.is_e2e
    _check("%s scale %g" % (name, scale), hsup, y, nc.E2E_WEIGHT, want_lp, ref, nc.e2e_rel(name), kernel_family,
           windowed=False, e2e=True)
