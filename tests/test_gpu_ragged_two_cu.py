"""Ragged batches of 8 sequences up to half the chip on TWO workgroups per sequence (the RAGGED instantiations of
den_tied_mitm.hip and of den_tied_planes.hip's two-workgroup form): every sequence meets at half its own
length.  Cases and float64 references: tests/ragged_two_cu_cases.py.  Beside the references every valid row is held to THE
BITS of the uniform two-workgroup call on that sequence alone (same frames, same data, same meeting frame), every padding
element to +0 (write) or its initial value (accumulate), and the result to the one-workgroup ragged route."""
import ctypes as C

import numpy as np
import pytest
import torch

from torchain_amd import io
from torchain_amd._lib import check, lib
from torchain_amd.functions import ChainResults, chain_loss, compute_chain_objf_and_deriv

import ragged_cases as rc
import ragged_two_cu_cases as tc
import row_contract_cases as rcc
from helpers import hip_den_on, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 1e-4  # test_gpu_ragged.py::test_den_form's bound (floors: the derivative weight / the supervision weight)
# tests/test_gpu_tied.py::_mitm_vs_fused holds the uniform meet-in-the-middle form to the fused kernel at these two (log-prob
# relative; derivative matrix-wise, rel_err without a floor); tests/test_gpu_planes.py holds the plane-wise kernel's two forms
# to the oracle only, so the tied kernels' -- the stricter -- is asked of them as well: the scheme and the per-state formulas
# are the same.
LOGPROB_FORMS, DERIV_FORMS = 1e-6, 2e-5
SENTINEL = rcc.SENTINEL
LENS, S, T = tc.LENGTHS, tc.S, tc.TMAX


def _counter(name):
    return int(lib.tc_debug_counter(name.encode()))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _den_ragged(graph, lens, yt, deriv, accumulate=False, deriv_weight=tc.DERIV_WEIGHT):
    """tc_den_forward_backward_ragged on device tensors where they lie; returns (log-prob, status)."""
    rows, cols = yt.shape
    n, tmax = len(lens), max(lens)
    assert rows == n * tmax
    graph.prepare(yt.device)
    frames = torch.tensor(list(lens), dtype=torch.int32, device=yt.device)
    nbytes = lib.tc_chain_workspace_bytes(graph.ptr, n, tmax)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=yt.device)
    lp = torch.full((1,), -123.0, dtype=torch.float64, device=yt.device)
    st = torch.full((1,), -1, dtype=torch.int32, device=yt.device)
    rcode = lib.tc_den_forward_backward_ragged(
        graph.ptr, n, C.c_void_p(yt.data_ptr()), rows, cols, yt.stride(0), rcc.LEAKY, deriv_weight, 0.0, 1 if accumulate else 0,
        C.c_void_p(deriv.data_ptr()) if deriv is not None else None, deriv.stride(0) if deriv is not None else cols,
        C.c_void_p(frames.data_ptr()), tmax, C.c_void_p(lp.data_ptr()), C.c_void_p(st.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes,
        torch.cuda.current_device(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rcode == 0, rcode
    return float(lp.item()), int(st.item())


def _inputs(form, lens=LENS):
    fam = tc.FORMS[form]
    y = tc.den_output(fam.graph, lens)
    return fam, y, torch.from_numpy(rc.with_padding(y, lens, np.nan)).to(DEV)


def _force_two_cu(form, kernel_family, on=1):
    """The uniform call onto the two-workgroup meet-in-the-middle form: the plane-wise graphs take it by default"""
    if form not in tc.PLANEWISE:
        kernel_family("force_mitm", on)


# ---- 1. the route ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["write", "accumulate"])
@pytest.mark.parametrize("form", sorted(tc.FORMS))
def test_route(form, mode, kernel_family):
    fam, y, yt = _inputs(form)
    graph = rcc.den_graph(fam, kernel_family)
    deriv = torch.full((S * T, y.shape[1]), 0.25, device=DEV)
    two, den = _counter("ragged_two_cu_launches"), _counter("den_launches")
    assert two >= 0  # (the counter exists)
    _, st = _den_ragged(graph, LENS, yt, deriv, accumulate=mode == "accumulate")
    assert st == 0
    assert _counter("ragged_two_cu_launches") == two + 1 and _counter("den_launches") == den + 1
    _den_ragged(graph, LENS, yt, None)  # the evaluation step stays one-workgroup
    assert _counter("ragged_two_cu_launches") == two + 1 and _counter("den_launches") == den + 2
    kernel_family("no_phase_split")
    _den_ragged(graph, LENS, yt, deriv, accumulate=mode == "accumulate")
    assert _counter("ragged_two_cu_launches") == two + 1 and _counter("den_launches") == den + 3


# ---- 2, 3, 5. against float64, the uniform two-workgroup call on each sequence alone, the one-workgroup ragged route ------------
@pytest.mark.parametrize("mode", ["write", "accumulate"])
@pytest.mark.parametrize("form", sorted(tc.FORMS))
def test_den_form(form, mode, kernel_family):
    fam, y, yt = _inputs(form)
    graph = rcc.den_graph(fam, kernel_family)
    P = y.shape[1]
    accumulate, init = mode == "accumulate", (0.25 if mode == "accumulate" else SENTINEL)
    dw, pad = tc.DERIV_WEIGHT, rc.padding_rows(LENS)

    def run():
        buf, view = rcc.strided(S * T, P, P + 4, 0, SENTINEL, device=DEV)
        view.fill_(init)
        lp, st = _den_ragged(graph, LENS, yt, view, accumulate=accumulate)
        return lp, st, buf, view

    two = _counter("ragged_two_cu_launches")
    lp, st, buf, view = run()
    assert _counter("ragged_two_cu_launches") == two + 1 and st == 0
    got = view.cpu().numpy()
    # 2. float64, the oracle on each sequence alone
    want_lp, want_d = tc.den_reference(fam.graph)
    err_lp = abs(lp - want_lp) / abs(want_lp)
    err_d = rel_err(got[~pad] - np.float32(init), want_d[~pad], floor=abs(dw)) if accumulate else rel_err(got, want_d, floor=abs(dw))
    print("%s %s: log-prob %.12g (float64 %.12g, rel %.2e), derivative rel %.2e" % (form, mode, lp, want_lp, err_lp, err_d))
    assert err_lp <= REL
    if accumulate:
        assert np.all(got[pad] == np.float32(init))  # untouched
        assert err_d <= REL + 1e-6  # (one rounding of init + g)
    else:
        assert not _bits(got[pad]).any()  # +0, not -0, not NaN
        assert err_d <= REL
    assert np.all(rcc.outside(buf, view).cpu().numpy() == _bits(np.float32(SENTINEL)))
    # 3. every sequence of two frames or more: the bits of the uniform call on it alone, on the same two-workgroup form (the same
    # frames, data and meeting frame T_s / 2; no block sum's order depends on the batch)
    _force_two_cu(form, kernel_family)
    sbuf, sview = rcc.strided(S * T, P, P + 4, 0, SENTINEL, device=DEV)
    sview.fill_(init)
    for s, Ts in enumerate(LENS):
        if Ts < 2:
            continue
        one = hip_den_on(graph, 1, yt[s::S][:Ts], sview[s::S][:Ts], leaky=rcc.LEAKY, deriv_weight=dw, accumulate=accumulate)
        assert one["status"] == 0, (form, s, Ts)
        rows = rc.valid_rows(LENS, s)
        assert np.array_equal(_bits(got[rows]), _bits(sview.cpu().numpy()[rows])), (form, mode, s, Ts)
    _force_two_cu(form, kernel_family, 0)
    # 5. the one-workgroup ragged route on the same batch
    kernel_family("no_phase_split")
    lp1, st1, buf1, view1 = run()
    assert _counter("ragged_two_cu_launches") == two + 1 and st1 == 0
    one_wg = view1.cpu().numpy()
    d_forms = rel_err(got[~pad], one_wg[~pad])
    print("%s %s: against the one-workgroup route: log-prob rel %.2e, derivative rel %.2e" % (form, mode, abs(lp - lp1) / abs(lp1), d_forms))
    assert abs(lp - lp1) <= LOGPROB_FORMS * abs(lp1)
    assert d_forms <= DERIV_FORMS
    assert np.array_equal(_bits(got[pad]), _bits(one_wg[pad]))


# ---- 4. equal lengths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [6, 7])
@pytest.mark.parametrize("form", sorted(tc.FORMS))
def test_equal_lengths_give_the_uniform_calls_bits(form, frames, kernel_family):
    lens = (frames,) * S
    fam, y, yt = _inputs(form, lens)
    graph = rcc.den_graph(fam, kernel_family)
    ragged = torch.full((S * frames, y.shape[1]), SENTINEL, device=DEV)
    uniform = torch.full((S * frames, y.shape[1]), SENTINEL, device=DEV)
    two = _counter("ragged_two_cu_launches")
    lp, st = _den_ragged(graph, lens, yt, ragged)
    assert _counter("ragged_two_cu_launches") == two + 1 and st == 0
    _force_two_cu(form, kernel_family)
    one = hip_den_on(graph, S, yt, uniform, leaky=rcc.LEAKY, deriv_weight=tc.DERIV_WEIGHT)
    assert one["status"] == 0 and one["logprob"] == lp
    assert torch.equal(ragged.view(torch.int32), uniform.view(torch.int32))


# ---- 6. the chip boundary --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beyond", [0, 1])
def test_chip_boundary(beyond, kernel_family):
    n = torch.cuda.get_device_properties(0).multi_processor_count
    lens = tc.boundary_lengths(n // 2 + beyond)
    fam, y, yt = _inputs("tied8_two_cu", lens)
    graph = rcc.den_graph(fam, kernel_family)
    deriv = torch.full((len(lens) * max(lens), y.shape[1]), SENTINEL, device=DEV)
    two = _counter("ragged_two_cu_launches")
    lp, st = _den_ragged(graph, lens, yt, deriv)
    assert _counter("ragged_two_cu_launches") == two + (0 if beyond else 1)  # both roles of every sequence must be resident
    want_lp, want_d = tc.den_reference(fam.graph, lens)
    got = deriv.cpu().numpy()
    assert st == 0 and abs(lp - want_lp) <= REL * abs(want_lp)
    assert rel_err(got, want_d, floor=abs(tc.DERIV_WEIGHT)) <= REL
    assert not _bits(got[rc.padding_rows(lens)]).any()


# ---- 7. the step -----------------------------------------------------------------------------------------------------------------
_graphs = {}


def _den():
    if "g" not in _graphs:
        _graphs["g"] = io.DenominatorGraph(rc.den_fst(), rc.P).prepare(0)
    return _graphs["g"]


def _as_layout(y2d, layout, dtype):
    """The (Tmax * S, P) matrix as chain_loss input; returns (tensor, function: its gradient -> (T, S, P))"""
    t = torch.from_numpy(np.ascontiguousarray(y2d)).to(DEV).view(T, S, -1)
    if layout == "rows":
        return t.reshape(T * S, -1).to(dtype), lambda g: g.view(T, S, -1)
    assert layout == "bct"
    return t.permute(1, 2, 0).contiguous().to(dtype), lambda g: g.permute(2, 0, 1)


def _sup():
    return io.Supervision.from_e2e_fsts(rc.WEIGHT, list(LENS), rc.P, tc.step_fsts())


@pytest.mark.parametrize("xent", [False, True])
@pytest.mark.parametrize("layout,dtype", [("bct", torch.float32), ("rows", torch.float32), ("bct", torch.bfloat16)])
def test_chain_loss(layout, dtype, xent):
    w, pad = rc.WEIGHT, rc.padding_rows(LENS)
    y = tc.step_output()
    x, back = _as_layout(rc.with_padding(y, LENS, np.nan), layout, dtype)
    xx, _ = _as_layout(rc.with_padding((0.5 * y).astype(np.float32), LENS, np.nan), layout, dtype)
    x.requires_grad_(True)
    xx.requires_grad_(True)
    kw = dict(l2_regularize=rc.L2, leaky_hmm_coefficient=rc.LEAKY)
    if xent:
        kw.update(xent_regularize=0.1, kaldi_way=True)
    two = _counter("ragged_two_cu_launches")
    loss, res = chain_loss(x, _den(), _sup(), xent_input=xx if xent else None, **kw)
    grads = torch.autograd.grad(loss, (x, xx) if xent else (x,))
    torch.cuda.synchronize()
    assert _counter("ragged_two_cu_launches") == two + 1
    r = res.data.numpy().copy()
    g = back(grads[0]).reshape(T * S, -1).float().cpu().numpy()
    # the float64 reference of the outputs the step was given (rounded to bfloat16 there); a bfloat16 gradient is the float32
    # one rounded to 8 significant bits: 2^-8 relative on top
    bf = dtype == torch.bfloat16
    want = tc.step_reference(bf)
    tol = REL + (2.0 ** -8 if bf else 0.0)
    print("%s %s xent=%d: objf %.9g (float64 %.9g), l2 %.9g (%.9g), gradient rel %.2e" %
          (layout, dtype, xent, r[0], want["objf"], r[1], want["l2_term"], rel_err(-g, want["deriv"], floor=w)))
    assert abs(r[0] - want["objf"]) <= REL * abs(want["objf"])
    assert abs(r[1] - want["l2_term"]) <= REL * abs(want["l2_term"])
    assert r[2] == np.float32(w) * np.float32(sum(LENS))
    assert rel_err(-g, want["deriv"], floor=w) <= tol
    assert not _bits(g[pad]).any()
    if xent:
        gx = back(grads[1]).reshape(T * S, -1).float().cpu().numpy()
        assert rel_err(-gx, 0.1 * want["xent_deriv"], floor=0.1 * w) <= tol
        assert not _bits(gx[pad]).any()


def test_captured_step_replays():
    kw = dict(l2_regularize=rc.L2, leaky_hmm_coefficient=rc.LEAKY, xent_regularize=0.1, kaldi_way=True)
    sup = _sup()
    x, _ = _as_layout(rc.with_padding(tc.step_output(), LENS, np.nan), "bct", torch.float32)
    x.requires_grad_(True)
    xe = (0.5 * x.detach()).clone().requires_grad_(True)

    def step():
        loss, results = chain_loss(x, _den(), sup, xent_input=xe, **kw)
        g, gx = torch.autograd.grad(loss, (x, xe))
        return loss.detach(), g, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    side.synchronize()
    cg = torch.cuda.CUDAGraph()
    two = _counter("ragged_two_cu_launches")
    with torch.cuda.graph(cg, stream=side):
        captured = step()
    assert _counter("ragged_two_cu_launches") == two + 1
    cg.replay()
    torch.cuda.synchronize()
    got = [c.clone() for c in captured]
    want = step()
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_warm_steps_allocate_nothing():
    x, _ = _as_layout(rc.with_padding(tc.step_output(), LENS, np.nan), "bct", torch.float32)
    x.requires_grad_(True)
    kw = dict(l2_regularize=rc.L2, leaky_hmm_coefficient=rc.LEAKY)

    def step():
        loss, _ = chain_loss(x, _den(), _sup(), **kw)  # (a fresh handle every step, as a reader's)
        return torch.autograd.grad(loss, x)[0]

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    before = _counter("pool_device_allocs")
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    assert _counter("pool_device_allocs") == before


# ---- 8. soft failure ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", ["first", "last"])
def test_nan_in_a_valid_frame_fails_softly(frame):
    """One NaN in a frame of role F's pure half (frame 0) or of role B's (the last frame) of the longest sequence: that role's
    partner still gets its publish -- nobody hangs -- and the batch takes the failure route."""
    w = rc.WEIGHT
    s = int(np.argmax(LENS))
    y = rc.with_padding(tc.step_output(), LENS, 3.0)
    y[(0 if frame == "first" else LENS[s] - 1) * S + s, 5] = np.nan
    yt = torch.from_numpy(y).to(DEV)
    deriv, xd = torch.full(yt.shape, 7.0, device=DEV), torch.full(yt.shape, 7.0, device=DEV)
    res = ChainResults()
    two = _counter("ragged_two_cu_launches")
    compute_chain_objf_and_deriv(_den(), _sup(), yt, res.data, deriv, xd, rc.L2, rc.LEAKY, 0.1)
    torch.cuda.synchronize()
    assert _counter("ragged_two_cu_launches") == two + 1
    r, d, x = res.data.numpy().copy(), deriv.cpu().numpy(), xd.cpu().numpy()
    assert r[0] == np.float32(-10.0) * (np.float32(w) * np.float32(sum(LENS)))
    pad = rc.padding_rows(LENS)
    assert not _bits(d[pad]).any() and not _bits(x).any()
    want = -w * rc.L2 * y[~pad].astype(np.float64)
    ok = np.isfinite(want)
    np.testing.assert_allclose(d[~pad][ok], want[ok], rtol=1e-6, atol=0)
    assert np.isnan(d[~pad][~ok]).all() and (~ok).sum() == 1
