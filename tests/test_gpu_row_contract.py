"""What every denominator kernel form does with the caller's rows as they are handed over (cases: tests/row_contract_cases.py).

Bad values.  DESIGN.md 1 and include/torchain_hip.h promise a soft failure for NaN / inf outputs; which kernel a minibatch
takes depends on the batch and on a measured choice, so the promise has to hold in every one of them and at every position:
the prologue's row, the first loop frame, both sides of the meeting frame, the epilogue's row, the first and the last
sequence (the two-sequence kernel's phantom partner, the sequence past a whole slab), the first and the last column, every
plane of 4096 pdfs, a ragged last float4, a column no arc carries.  The bare denominator states the failure as a non-finite
log-prob (``finalize_kernel`` turns that into objf = -10 * weight); a finite value beyond the clamp (31) must not fail, a value
whose square overflows float32 (1e20) must, and whatever lies in a row's padding is not read.

Rows as they lie.  The 16-byte and the four-dword row path (api.cpp: y_vec, d_vec, x_vec) change how values are fetched and
stored, not what is computed: log-prob, derivative and the objective's three matrices are bit for bit those of the contiguous,
aligned call in every mixed state, and no float of the caller's buffers outside the (rows, cols) view is written -- in front of
the first row, between the rows, behind the last.  The contiguous call itself is held to float64 with ``helpers.peaky_check``'s
bounds.  Every call here is a legal one on the test's own allocations."""
import numpy as np
import pytest
import torch

from torchain_amd import io
from torchain_amd.functions import ChainResults, compute_chain_objf_and_deriv

import row_contract_cases as rc
from helpers import hip_den_on

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAD = (float("nan"), float("inf"), float("-inf"))
L2 = 1e-3
fam_ids = dict(ids=lambda f: f.name)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def sentinel_kept(buffer, view, fill=rc.SENTINEL):
    want = torch.tensor([fill], dtype=torch.float32).view(torch.int32).item()
    return bool((rc.outside(buffer, view) == want).all())


def on_device(y):
    return torch.from_numpy(np.array(y, np.float32)).to(DEV)


# ---- bad values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", rc.BAD_VALUE_FAMILIES, **fam_ids)
def test_one_bad_element_fails_the_denominator(kernel_family, family):
    """One NaN, +inf or -inf anywhere in y: the log-prob is not finite, with a derivative and in the forward-only call (the
    evaluation step).  31.0 in the same place -- finite, beyond the clamp -- gives a finite one."""
    graph = rc.den_graph(family, kernel_family)
    assert graph.stats()["tied"] == family.tied
    S, T = family.S, family.T
    yt = on_device(rc.nnet_output(family.graph, S, T))
    deriv = torch.zeros_like(yt)
    for d in (deriv, None):
        clean = hip_den_on(graph, S, yt, d, leaky=rc.LEAKY)
        assert np.isfinite(clean["logprob"]) and clean["status"] == 0
    finite, clamped = [], []
    for t, s, c in rc.bad_value_picks(family):
        row = t * S + s
        keep = yt[row, c].item()
        for bad in BAD:
            yt[row, c] = bad
            for d in (deriv, None):
                out = hip_den_on(graph, S, yt, d, leaky=rc.LEAKY)
                if np.isfinite(out["logprob"]):
                    finite.append((t, s, c, bad, "deriv" if d is not None else "forward only", out["logprob"]))
        yt[row, c] = 31.0
        for d in (deriv, None):
            out = hip_den_on(graph, S, yt, d, leaky=rc.LEAKY)
            if not (np.isfinite(out["logprob"]) and out["status"] == 0):
                clamped.append((t, s, c, out))
        yt[row, c] = keep
    assert not finite, "%s: a finite log-prob for (t, s, c, value, call): %s" % (family.name, finite)
    assert not clamped, "%s: 31.0 failed at %s" % (family.name, clamped)


@pytest.mark.parametrize("family", rc.BAD_VALUE_FAMILIES, **fam_ids)
def test_a_value_whose_square_overflows_fails(kernel_family, family):
    """A single 1e20: finite, but sum(y^2) -- the l2 term's sum, which carries the failure -- is infinite in float32.  Every
    kernel takes the failure route for it (include/torchain_hip.h)."""
    graph = rc.den_graph(family, kernel_family)
    S, T = family.S, family.T
    yt = on_device(rc.nnet_output(family.graph, S, T))
    t, s, c = rc.objective_picks(family)[1]
    yt[t * S + s, c] = 1e20
    assert bool(torch.isfinite(yt).all())
    for d in (torch.zeros_like(yt), None):
        assert not np.isfinite(hip_den_on(graph, S, yt, d, leaky=rc.LEAKY)["logprob"]), (family.name, d is None)


@pytest.mark.parametrize("family", rc.BAD_VALUE_FAMILIES, **fam_ids)
def test_nan_in_the_padding_of_y_is_not_read(kernel_family, family):
    """Rows P + 4 apart with NaN between them (and in front of and behind the matrix): the bits of the unpadded call."""
    graph = rc.den_graph(family, kernel_family)
    S, T = family.S, family.T
    yt = on_device(rc.nnet_output(family.graph, S, T))
    rows, P = yt.shape
    ybuf, yv = rc.strided(rows, P, P + 4, 0, float("nan"), DEV)
    yv.copy_(yt)
    assert int(torch.isnan(ybuf).sum()) == ybuf.numel() - rows * P
    d0, d1 = torch.full_like(yt, 3.0), torch.full_like(yt, 5.0)
    a = hip_den_on(graph, S, yt, d0, leaky=rc.LEAKY, l2_scale=L2)
    b = hip_den_on(graph, S, yv, d1, leaky=rc.LEAKY, l2_scale=L2)
    assert a["status"] == 0 and b["status"] == 0 and np.isfinite(a["logprob"])
    assert a["logprob"] == b["logprob"] and same_bits(d0, d1)
    assert hip_den_on(graph, S, yv, None, leaky=rc.LEAKY)["logprob"] == hip_den_on(graph, S, yt, None, leaky=rc.LEAKY)["logprob"]


@pytest.mark.parametrize("family", rc.BAD_VALUE_FAMILIES, **fam_ids)
def test_one_bad_element_fails_the_objective_softly(kernel_family, family):
    """[K]'s order as include/torchain_hip.h states it: objf = -10 * weight, both derivatives zeroed, then the l2 derivative:
    deriv = -(w * l2) * y, one float32 product, wherever y is finite; xent_deriv = 0 everywhere."""
    graph = rc.den_graph(family, kernel_family)
    S, T = family.S, family.T
    sup = rc.supervision(family.graph, S, T)
    hsup = io.Supervision.from_synth(sup)
    w = np.float32(sup.weight)
    y = np.array(rc.nnet_output(family.graph, S, T), np.float32)
    yt = on_device(y)

    def run():
        deriv, xd = torch.full_like(yt, 7.0), torch.full_like(yt, 7.0)
        res = ChainResults()
        compute_chain_objf_and_deriv(graph, hsup, yt, res.data, deriv, xd, L2, rc.LEAKY, 0.1)
        torch.cuda.synchronize()
        return res.data.numpy().copy(), deriv.cpu().numpy(), xd.cpu().numpy()

    weight = w * np.float32(S) * np.float32(T)
    res, _, xd = run()
    assert np.isfinite(res).all() and res[0] != np.float32(-10.0) * weight and res[2] == weight and xd.any()   # the clean input does not fail
    scale = np.float32(w * np.float32(L2))
    for t, s, c in rc.objective_picks(family):
        row = t * S + s
        for bad in BAD:
            y_bad = y.copy()
            y_bad[row, c] = bad
            yt[row, c] = bad
            res, deriv, xd = run()
            what = (family.name, t, s, c, bad, res)
            assert res[0] == np.float32(-10.0) * weight and res[2] == weight, what
            ok = np.isfinite(y_bad)
            want = -(scale * y_bad[ok])
            assert np.array_equal(deriv[ok].view(np.int32), want.view(np.int32)), what
            assert not xd.any(), what
        yt[row, c] = float(y[row, c])


# ---- rows as they lie ------------------------------------------------------------------------------------------------------
def reference_calls(graph, family, yt):
    """The plain call -- contiguous, aligned -- in the three modes: name -> (log-prob, derivative).  The derivative starts from
    another value than the strided calls' wherever it is to be overwritten, so an element no store reaches differs."""
    out = {}
    for mode, (accumulate, l2_scale, init) in rc.MODES.items():
        d = torch.full_like(yt, init if accumulate else 3.0)
        r = hip_den_on(graph, family.S, yt, d, leaky=rc.LEAKY, l2_scale=l2_scale, accumulate=accumulate)
        assert r["status"] == 0 and np.isfinite(r["logprob"]), (family.name, mode, r)
        out[mode] = (r["logprob"], d)
    return out


@pytest.mark.parametrize("family", rc.FAMILIES, **fam_ids)
def test_rows_as_they_lie(kernel_family, family):
    """Padded, y scalar / deriv vector, y vector / deriv scalar, both bases off: the reference call's bits, the buffers' other
    floats untouched.  The reference call against float64: log-prob within 1e-6 relative, max |d - gamma| <= 1e-5, row sums
    within 1e-5 of 1 (``helpers.peaky_check``'s bounds for this comparison; worst values of one run:
    profiles/row_contract/worst_errors.txt)."""
    graph = rc.den_graph(family, kernel_family)
    assert graph.stats()["tied"] == family.tied
    S, T = family.S, family.T
    yt = on_device(rc.nnet_output(family.graph, S, T))
    rows, P = yt.shape
    ref = reference_calls(graph, family, yt)

    lp64, gam = rc.float64_reference(family.graph, S, T)
    lp, d = ref["write"][0], ref["write"][1].cpu().numpy().astype(np.float64)
    worst = (abs(lp - lp64) / abs(lp64), np.abs(d - gam).max(), np.abs(d.sum(axis=1) - 1.0).max())
    print("row_contract float64 %-16s log-prob rel %.2e  max |d - gamma| %.2e  max |row sum - 1| %.2e" % ((family.name,) + worst))
    assert worst[0] <= 1e-6 and worst[1] <= 1e-5 and worst[2] <= 1e-5, (family.name, worst)

    for name, ((ys, yo, ds, do), want) in rc.row_variants(P).items():
        for mode, (accumulate, l2_scale, init) in rc.MODES.items():
            ybuf, yv = rc.strided(rows, P, ys, yo, float("nan"), DEV)
            yv.copy_(yt)
            dbuf, dv = rc.strided(rows, P, ds, do, rc.SENTINEL, DEV)
            dv.fill_(init)
            assert (rc.vector_path(yv), rc.vector_path(dv)) == want, (name, yv.data_ptr(), dv.data_ptr())
            r = hip_den_on(graph, S, yv, dv, leaky=rc.LEAKY, l2_scale=l2_scale, accumulate=accumulate)
            what = (family.name, name, mode)
            assert r["status"] == 0, what
            assert r["logprob"] == ref[mode][0], what + (r["logprob"], ref[mode][0])
            assert same_bits(dv, ref[mode][1]), what + (float((dv - ref[mode][1]).abs().max()),)
            assert sentinel_kept(dbuf, dv), what
            assert same_bits(yv, yt) and int(torch.isnan(ybuf).sum()) == ybuf.numel() - rows * P, what


@pytest.mark.parametrize("family", rc.OBJECTIVE_FAMILIES, **fam_ids)
def test_objective_on_rows_as_they_lie(kernel_family, family):
    """y, deriv and xent_deriv each on a buffer of its own, strides and bases drawn independently (both states of x_vec against
    both of d_vec): results, deriv and xent_deriv are the contiguous call's bits, the padding of both outputs is untouched,
    xent_deriv is exactly 0 where no numerator arc carries the entry."""
    graph = rc.den_graph(family, kernel_family)
    S, T = family.S, family.T
    sup = rc.supervision(family.graph, S, T)
    hsup = io.Supervision.from_synth(sup)
    not_carried = torch.from_numpy(~rc.carried(sup)).to(DEV)
    yt = on_device(rc.nnet_output(family.graph, S, T))
    rows, P = yt.shape

    def run(y, deriv, xd):
        res = ChainResults()
        compute_chain_objf_and_deriv(graph, hsup, y, res.data, deriv, xd, L2, rc.LEAKY, 0.1)
        torch.cuda.synchronize()
        return res.data.clone()

    d0, x0 = torch.full_like(yt, 3.0), torch.full_like(yt, 3.0)
    res0 = run(yt, d0, x0)
    assert bool(torch.isfinite(res0).all()) and res0[0] != -10.0 * res0[2] and res0[2] == sup.weight * S * T
    assert bool((x0[not_carried] == 0).all()) and bool((x0[~not_carried] >= 0).all()) and bool(x0.any())
    for name, (places, want) in rc.OBJECTIVE_PLACEMENTS.items():
        (ybuf, yv), (dbuf, dv), (xbuf, xv) = (rc.strided(rows, P, P + pad, off, fill, DEV)
                                              for (pad, off), fill in zip(places, (float("nan"), rc.SENTINEL, rc.SENTINEL)))
        yv.copy_(yt)
        assert tuple(rc.vector_path(v) for v in (yv, dv, xv)) == want, name
        res = run(yv, dv, xv)
        what = (family.name, name)
        assert same_bits(res, res0), what + (res, res0)
        assert same_bits(dv, d0), what + (float((dv - d0).abs().max()),)
        assert same_bits(xv, x0), what + (float((xv - x0).abs().max()),)
        assert sentinel_kept(dbuf, dv) and sentinel_kept(xbuf, xv), what
        assert bool((xv[not_carried] == 0).all()), what
