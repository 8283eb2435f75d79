"""Ragged (unequal sequence lengths) end-to-end minibatches on the GPU: every one-workgroup-per-sequence denominator form
through tc_den_forward_backward_ragged, the end-to-end numerator, the 2-D objective, the failure routes and chain_loss in
every layout.  Cases and the float64 reference: tests/ragged_cases.py (the sum over sequences of the single-sequence
references).  Beside the references, every valid row is held to THE BITS of the uniform call on that sequence alone, and
every padding element to +0."""
import ctypes as C

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import check, lib
from torchain_amd.functions import ChainResults, chain_loss, compute_chain_objf_and_deriv

import e2e_reference as ref
import num_elementwise_cases as nc
import ragged_cases as rc
import row_contract_cases as rcc
from helpers import hip_den_on, hip_num, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 1e-4
TC_ERR_UNSUPPORTED = -3
SENTINEL = rcc.SENTINEL


def _counter(name):
    return int(lib.tc_debug_counter(name.encode()))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- a. the denominator forms ----------------------------------------------------------------------------------------------
def _den_ragged(graph, lens, yt, deriv, accumulate=False, leaky=rcc.LEAKY, deriv_weight=1.0, l2_scale=0.0, expect=0):
    """tc_den_forward_backward_ragged on device tensors where they lie; returns (log-prob, status)."""
    rows, cols = yt.shape
    S, T = len(lens), max(lens)
    assert rows == S * T
    graph.prepare(yt.device)
    frames = torch.tensor(list(lens), dtype=torch.int32, device=yt.device)
    nbytes = lib.tc_chain_workspace_bytes(graph.ptr, S, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=yt.device)
    lp = torch.full((1,), -123.0, dtype=torch.float64, device=yt.device)
    st = torch.full((1,), -1, dtype=torch.int32, device=yt.device)
    rcode = lib.tc_den_forward_backward_ragged(
        graph.ptr, S, C.c_void_p(yt.data_ptr()), rows, cols, yt.stride(0), leaky, deriv_weight, l2_scale, 1 if accumulate else 0,
        C.c_void_p(deriv.data_ptr()) if deriv is not None else None, deriv.stride(0) if deriv is not None else cols,
        C.c_void_p(frames.data_ptr()), T, C.c_void_p(lp.data_ptr()), C.c_void_p(st.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes,
        torch.cuda.current_device(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rcode == expect, rcode
    return float(lp.item()), int(st.item())


_oracle_graphs = {}


def _oracle_graph(graph_name):
    if graph_name not in _oracle_graphs:
        from oracle import pyoracle
        pyoracle.build()
        _oracle_graphs[graph_name] = pyoracle.DenGraph(rcc.den_fst(graph_name))
    return _oracle_graphs[graph_name]


def _den_inputs(graph_name, lens, seed):
    """(y with NaN in the padding, the same with zeros there for the oracle's slices) as (Tmax * S, P) float32"""
    S, T, P = len(lens), max(lens), rcc.den_fst(graph_name).num_pdfs
    y = synth.random_nnet_output(S, T, P, seed=seed)
    return rc.with_padding(y, lens, np.nan), y


@pytest.mark.parametrize("mode", ["write", "accumulate", "forward"])
@pytest.mark.parametrize("form", rc.DEN_FORMS)
def test_den_form(form, mode, kernel_family):
    fam = rcc.BY_NAME[form]
    graph = rcc.den_graph(fam, kernel_family)
    lens = rc.den_lengths(form)
    S, T = len(lens), max(lens)
    P = rcc.den_fst(fam.graph).num_pdfs
    y_nan, y = _den_inputs(fam.graph, lens, seed=40 + S)
    yt = torch.from_numpy(y_nan).to(DEV)
    accumulate, init = mode == "accumulate", (0.25 if mode == "accumulate" else SENTINEL)
    dw, pad = -0.8, rc.padding_rows(lens)

    def run():
        if mode == "forward":
            return _den_ragged(graph, lens, yt, None, deriv_weight=dw) + (None, None)
        buf, view = rcc.strided(S * T, P, P + 4, 0, SENTINEL, device=DEV)
        view.fill_(init)
        lp, st = _den_ragged(graph, lens, yt, view, accumulate=accumulate, deriv_weight=dw)
        return lp, st, buf, view

    lp, st, buf, view = run()
    # the uniform single-sequence calls, forced onto the same form by the family's launch switches (set by den_graph)
    single_lp = 0.0
    sbuf, sview = rcc.strided(S * T, P, P + 4, 0, SENTINEL, device=DEV)
    sview.fill_(init)
    for s, Ts in enumerate(lens):
        one = hip_den_on(graph, 1, yt[s::S][:Ts], None if mode == "forward" else sview[s::S][:Ts], leaky=rcc.LEAKY, deriv_weight=dw,
                         accumulate=accumulate)
        assert one["status"] == 0, (form, s, Ts)
        single_lp += one["logprob"]
    print("%s %s: log-prob %.12g, singles %.12g" % (form, mode, lp, single_lp))
    assert st == 0
    assert abs(lp - single_lp) <= 1e-9 * abs(single_lp)
    want_lp, want_d = rc.den_reference(_oracle_graph(fam.graph), lens, y, rcc.LEAKY, dw)
    assert abs(lp - want_lp) <= REL * abs(want_lp), (lp, want_lp)
    if mode != "forward":
        got, single = view.cpu().numpy(), sview.cpu().numpy()
        assert np.array_equal(_bits(got[~pad]), _bits(single[~pad]))
        if accumulate:
            assert np.all(got[pad] == np.float32(init))
            assert rel_err(got[~pad] - np.float32(init), want_d[~pad], floor=abs(dw)) <= REL + 1e-6  # (one rounding of init + g)
        else:
            assert not _bits(got[pad]).any()  # +0, not -0, not NaN
            assert rel_err(got, want_d, floor=abs(dw)) <= REL
        assert np.all(rcc.outside(buf, view).cpu().numpy() == _bits(np.float32(SENTINEL)))
    # the route does not depend on the launch switches
    for key in fam.launch:
        check(lib.tc_debug_set(key.encode(), 0), key)
    lp2, st2, buf2, view2 = run()
    assert lp2 == lp and st2 == st
    if mode != "forward":
        assert torch.equal(buf2.view(torch.int32), buf.view(torch.int32))


def test_den_more_workgroups_than_cus(kernel_family):
    fam = rcc.BY_NAME["tied8_fused"]
    graph = rcc.den_graph(fam, kernel_family)
    lens = tuple(1 + i % 9 for i in range(rc.DEN_MANY))
    S, T, P = len(lens), 9, rcc.den_fst(fam.graph).num_pdfs
    y_nan, y = _den_inputs(fam.graph, lens, seed=61)
    deriv = torch.full((S * T, P), SENTINEL, device=DEV)
    lp, st = _den_ragged(graph, lens, torch.from_numpy(y_nan).to(DEV), deriv, deriv_weight=1.0)
    want_lp, want_d = rc.den_reference(_oracle_graph(fam.graph), lens, y, rcc.LEAKY, 1.0)
    assert st == 0 and abs(lp - want_lp) <= REL * abs(want_lp)
    got = deriv.cpu().numpy()
    assert rel_err(got, want_d, floor=1.0) <= REL
    assert not _bits(got[rc.padding_rows(lens)]).any()


def test_den_streamed_graph_is_refused(kernel_family):
    fam = rcc.BY_NAME["streamed_narrow"]
    graph = rcc.den_graph(fam, kernel_family)
    assert graph.stats()["tied"] == 2
    lens = (5, 2, 4) + (5,) * (fam.S - 3)
    P = rcc.den_fst(fam.graph).num_pdfs
    yt = torch.from_numpy(synth.random_nnet_output(len(lens), 5, P, seed=3)).to(DEV)
    deriv = torch.full(yt.shape, SENTINEL, device=DEV)
    launches = _counter("den_launches")
    lp, st = _den_ragged(graph, lens, yt, deriv, expect=TC_ERR_UNSUPPORTED)
    assert (lp, st) == (-123.0, -1) and bool((deriv == SENTINEL).all())
    assert _counter("den_launches") == launches


# ---- b. the numerator --------------------------------------------------------------------------------------------------------
def _elementwise(got, want, weight, rel, what):
    """helpers.posteriors_elementwise's comparisons for one sequence's rows -- every entry above 1e-8 * weight within ``rel``
    relative, every other within 1e-9 * weight, exactly 0 where the reference is, rows summing to the weight -- without its
    demand that every magnitude class be populated (a sequence of one or two frames has a few dozen entries)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(got).all(), what
    big = want > 1e-8 * weight
    assert big.any(), what
    worst = float((np.abs(got - want)[big] / want[big]).max())
    print("%s: worst relative error %.2e over %d entries" % (what, worst, int(big.sum())))
    assert worst <= rel, what
    assert np.abs(got - want)[~big].max(initial=0.0) <= 1e-9 * weight, what
    assert not got[want == 0].any(), what
    assert np.abs(got.sum(axis=1) / weight - 1.0).max() <= 1e-5, what


@pytest.mark.parametrize("name", ["random", "chain"])
def test_numerator(name):
    lens, fsts, w = rc.lengths(name), rc.fsts(name), nc.E2E_WEIGHT
    S = len(lens)
    y = rc.with_padding(rc.nnet_output(name), lens, np.nan)
    sup = io.Supervision.from_e2e_fsts(w, list(lens), rc.P, fsts)
    out = hip_num(sup, y, init=0.0)
    kept = hip_num(sup, y, init=SENTINEL)
    pad = rc.padding_rows(lens)
    assert np.all(kept["deriv"][pad] == np.float32(SENTINEL)) and not _bits(out["deriv"][pad]).any()
    want_lp = 0.0
    for s, Ts in enumerate(lens):
        rows = rc.valid_rows(lens, s)
        ys = np.ascontiguousarray(rc.nnet_output(name)[rows])
        logz, gamma = ref.num_logz([fsts[s]], ys.astype(np.float64), Ts)
        want_lp += w * float(logz.sum())
        _elementwise(out["deriv"][rows], w * gamma, w, nc.REL_E2E, "%s sequence %d" % (name, s))
        one = hip_num(io.Supervision.from_e2e_fsts(w, Ts, rc.P, [fsts[s]]), ys, init=0.0)
        assert np.array_equal(_bits(out["deriv"][rows]), _bits(one["deriv"])), (name, s)
    assert abs(out["logprob_weighted"] - want_lp) <= nc.REL_LOGPROB * abs(want_lp)
    assert kept["logprob_weighted"] == out["logprob_weighted"]


# ---- c. the objective ----------------------------------------------------------------------------------------------------------
_graphs = {}


def _den():
    if "g" not in _graphs:
        _graphs["g"] = io.DenominatorGraph(rc.den_fst(), rc.P).prepare(0)
    return _graphs["g"]


def _hip(sup, y, xent=False, l2=rc.L2, leaky=rc.LEAKY):
    yt = torch.from_numpy(np.array(y, dtype=np.float32)).to(DEV)
    deriv = torch.full(yt.shape, 7.0, device=DEV)
    xd = torch.full(yt.shape, 7.0, device=DEV) if xent else None
    res = ChainResults()
    compute_chain_objf_and_deriv(_den(), sup, yt, res.data, deriv, xd, l2, leaky, 0.1 if xent else 0.0)
    torch.cuda.synchronize()
    return res.data.numpy().copy(), deriv.cpu().numpy(), None if xd is None else xd.cpu().numpy()


def _check(got_res, got_d, want, w, lens):
    """The comparisons of test_gpu_e2e._check.  The weight is held to the float32 product of the supervision's float32
    weight and the frame count, which is all the library is given (the float64 reference's 0.7 * 36 rounds to another
    float32 than 0.7f * 36 does)."""
    assert abs(got_res[0] - want["objf"]) <= REL * abs(want["objf"]), (got_res, want["objf"])
    assert abs(got_res[1] - want["l2_term"]) <= REL * abs(want["l2_term"]) + 1e-30, (got_res, want["l2_term"])
    assert got_res[2] == np.float32(w) * np.float32(sum(lens))
    assert abs(got_res[2] - want["weight"]) <= 1e-6 * want["weight"]
    assert rel_err(got_d, want["deriv"], floor=w) <= REL


@pytest.mark.parametrize("xent", [False, True])
@pytest.mark.parametrize("name", ["random", "chain"])
def test_objective(name, xent, kernel_family):
    lens, fsts, w = rc.lengths(name), rc.fsts(name), rc.WEIGHT
    y = rc.with_padding(rc.nnet_output(name), lens, np.nan)
    sup = io.Supervision.from_e2e_fsts(w, list(lens), rc.P, fsts)
    steps = _counter("ragged_steps")
    res, d, xd = _hip(sup, y, xent=xent)
    assert _counter("ragged_steps") == steps + 1
    want = rc.reference(name)
    _check(res, d, want, w, lens)
    pad = rc.padding_rows(lens)
    assert not _bits(d[pad]).any()
    if xent:
        assert rel_err(xd, want["xent_deriv"], floor=w) <= REL
        assert not _bits(xd[pad]).any()
    again = _hip(sup, y, xent=xent)
    for a, b in zip((res, d, xd), again):
        assert (a is None and b is None) or np.array_equal(_bits(a), _bits(b))
    # valid rows: the bits of the uniform call on that sequence alone, forced onto the one-workgroup form a ragged batch
    # takes (the graph is a tied one: a uniform batch of one sequence would run on two workgroups)
    kernel_family("no_phase_split")
    for s, Ts in enumerate(lens):
        rows = rc.valid_rows(lens, s)
        one = _hip(io.Supervision.from_e2e_fsts(w, Ts, rc.P, [fsts[s]]), rc.nnet_output(name)[rows], xent=xent)
        assert np.array_equal(_bits(d[rows]), _bits(one[1])), (name, s)
        if xent:
            assert np.array_equal(_bits(xd[rows]), _bits(one[2])), (name, s)


@pytest.mark.parametrize("xent", [False, True])
def test_equal_lengths_give_the_uniform_handles_bits(xent, kernel_family):
    kernel_family("no_phase_split")  # (the uniform call onto the one-workgroup form; the ragged one takes it anyway)
    lens, fsts, w = rc.lengths("equal"), rc.fsts("equal"), rc.WEIGHT
    y = rc.nnet_output("equal")
    ragged = _hip(io.Supervision.from_e2e_fsts(w, list(lens), rc.P, fsts), y, xent=xent)
    uniform = _hip(io.Supervision.from_e2e_fsts(w, lens[0], rc.P, fsts), y, xent=xent)
    for a, b in zip(ragged, uniform):
        assert (a is None and b is None) or np.array_equal(_bits(a), _bits(b))
    _check(ragged[0], ragged[1], rc.reference("equal"), w, lens)


# ---- d. the failure routes -----------------------------------------------------------------------------------------------------
def test_nan_in_a_valid_frame_fails_softly():
    name = "random"
    lens, fsts, w = rc.lengths(name), rc.fsts(name), rc.WEIGHT
    s = int(np.argmin(lens))
    y = rc.with_padding(rc.nnet_output(name), lens, 3.0)
    y[(lens[s] - 1) * len(lens) + s, 5] = np.nan  # the last valid frame of the shortest sequence
    res, d, xd = _hip(io.Supervision.from_e2e_fsts(w, list(lens), rc.P, fsts), y, xent=True)
    assert res[0] == np.float32(-10.0) * (np.float32(w) * np.float32(sum(lens)))
    pad = rc.padding_rows(lens)
    assert not _bits(d[pad]).any() and not _bits(xd).any()
    want = -w * rc.L2 * y[~pad].astype(np.float64)
    ok = np.isfinite(want)
    np.testing.assert_allclose(d[~pad][ok], want[ok], rtol=1e-6, atol=0)
    assert np.isnan(d[~pad][~ok]).all() and (~ok).sum() == 1


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_padding_values_change_no_bit(value):
    name = "chain"
    lens, fsts, w = rc.lengths(name), rc.fsts(name), rc.WEIGHT
    sup = io.Supervision.from_e2e_fsts(w, list(lens), rc.P, fsts)
    clean = _hip(sup, rc.nnet_output(name), xent=True)
    dirty = _hip(sup, rc.with_padding(rc.nnet_output(name), lens, value), xent=True)
    assert clean[0][0] != np.float32(-10.0) * clean[0][2]
    for a, b in zip(clean, dirty):
        assert np.array_equal(_bits(a), _bits(b))


def test_a_sequence_shorter_than_its_shortest_path_fails_softly():
    name = "chain"
    fsts, w = rc.fsts(name), rc.WEIGHT
    lens = list(rc.lengths(name))
    lens[1] = ref.shortest_path_arcs(fsts[1]) - 1
    y = rc.with_padding(rc.nnet_output(name), lens, np.nan)
    res, d, xd = _hip(io.Supervision.from_e2e_fsts(w, lens, rc.P, fsts), y, xent=True)
    assert res[0] == np.float32(-10.0) * (np.float32(w) * np.float32(sum(lens)))
    pad = rc.padding_rows(lens)
    assert not _bits(d[pad]).any() and not _bits(xd).any()
    np.testing.assert_allclose(d[~pad], -w * rc.L2 * y[~pad], rtol=1e-6, atol=0)


# ---- e. chain_loss ---------------------------------------------------------------------------------------------------------------
def _as_layout(y2d, S, T, layout, dtype):
    """The (Tmax * S, P) matrix as chain_loss input of the layout; returns (tensor, function: its gradient -> (T, S, P))"""
    t = torch.from_numpy(np.ascontiguousarray(y2d)).to(DEV).view(T, S, -1)
    if layout == "rows":
        return t.reshape(T * S, -1).to(dtype), lambda g: g.view(T, S, -1)
    if layout == "bct":
        return t.permute(1, 2, 0).contiguous().to(dtype), lambda g: g.permute(2, 0, 1)
    if layout == "batch_first":
        return t.permute(1, 0, 2).contiguous().to(dtype).permute(0, 2, 1), lambda g: g.permute(2, 0, 1)
    assert layout == "time_major"
    return t.contiguous().to(dtype).permute(1, 2, 0), lambda g: g.permute(2, 0, 1)


def _single(y2d, s, S, Ts, layout, dtype):
    rows = np.arange(Ts) * S + s
    return _as_layout(y2d[rows], 1, Ts, layout, dtype)


LAYOUTS = [("bct", torch.float32), ("bct", torch.bfloat16), ("batch_first", torch.float32), ("time_major", torch.float32),
           ("rows", torch.float32)]
MODES = ["xent_kaldi", "xent_reference", "deriv_weights", "out_of_range", "no_grad"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
def test_chain_loss(layout, dtype, mode, kernel_family):
    kernel_family("no_phase_split")  # (the single-sequence calls onto the one-workgroup form a ragged batch takes)
    name = "random"
    lens, fsts, w = rc.lengths(name), rc.fsts(name), rc.WEIGHT
    S, T = len(lens), max(lens)
    pad = rc.padding_rows(lens)
    y = np.array(rc.nnet_output(name), copy=True)
    kw = dict(l2_regularize=rc.L2, leaky_hmm_coefficient=rc.LEAKY)
    dwt = None
    if mode in ("xent_kaldi", "xent_reference", "no_grad"):
        kw.update(xent_regularize=0.1, kaldi_way=mode != "xent_reference")
    if mode == "out_of_range":
        kw.update(out_of_range_regularize=0.01)
        y[0 * S + 0, 3], y[1 * S + 4, 7] = 33.0, -35.0  # valid frames of sequences 0 and 4 beyond +-30
    if mode == "deriv_weights":
        dwt = np.random.default_rng(9).uniform(0.0, 2.0, size=T * S).astype(np.float32)
        kw.update(deriv_weights=torch.from_numpy(dwt).to(DEV))
    y_in = rc.with_padding(y, lens, 40.0 if mode == "out_of_range" else np.nan)  # (out of range in the padding too)
    xe = (0.5 * y).astype(np.float32)
    xe_in = rc.with_padding(xe, lens, np.nan)
    sup = io.Supervision.from_e2e_fsts(w, list(lens), rc.P, fsts)
    x, back = _as_layout(y_in, S, T, layout, dtype)
    xx, _ = _as_layout(xe_in, S, T, layout, dtype)
    use_xent = "xent_regularize" in kw

    if mode == "no_grad":
        with torch.no_grad():
            loss, res = chain_loss(x, _den(), sup, xent_input=xx, **kw)
        want = rc.reference(name)
        r = res.data.numpy()
        assert abs(r[0] - want["objf"]) <= (REL if dtype == torch.float32 else 2e-2) * abs(want["objf"])
        assert r[2] == np.float32(w) * np.float32(sum(lens))
        assert abs(float(loss) + r[0] / r[2]) <= 1e-2 * abs(float(loss))
        return

    x.requires_grad_(True)
    xx.requires_grad_(True)
    loss, res = chain_loss(x, _den(), sup, xent_input=xx if use_xent else None, **kw)
    grads = torch.autograd.grad(loss, (x, xx) if use_xent else (x,))
    torch.cuda.synchronize()
    r = res.data.numpy().copy()
    g = back(grads[0]).reshape(T * S, -1).float().cpu().numpy()
    gx = back(grads[1]).reshape(T * S, -1).float().cpu().numpy() if use_xent else None
    assert r[2] == np.float32(w) * np.float32(sum(lens))
    # (kaldi_way=False: the objective of xent_input; out of range: the kernels clamp exp(y), the oracle does not -- both are
    # held to the sum of the single-sequence calls below)
    if dtype == torch.float32 and mode not in ("xent_reference", "out_of_range"):
        want = rc.reference(name)
        assert abs(r[0] - want["objf"]) <= REL * abs(want["objf"])
        assert abs(r[1] - want["l2_term"]) <= REL * abs(want["l2_term"])
        assert abs(float(loss.detach()) + r[0] / r[2]) <= 1e-6 * abs(float(loss.detach()))
    # padding: exactly zero, of either sign for nothing: +0
    assert not _bits(g[pad]).any()
    if use_xent:
        assert not _bits(gx[pad]).any()
    # valid positions: chain_loss on each sequence alone
    objf = 0.0
    for s, Ts in enumerate(lens):
        rows = rc.valid_rows(lens, s)
        one = io.Supervision.from_e2e_fsts(w, Ts, rc.P, [fsts[s]])
        xs, back1 = _single(y, s, S, Ts, layout, dtype)
        xxs, _ = _single(xe, s, S, Ts, layout, dtype)
        xs.requires_grad_(True)
        xxs.requires_grad_(True)
        kw1 = dict(kw)
        if dwt is not None:
            kw1["deriv_weights"] = torch.from_numpy(np.ascontiguousarray(dwt[rows])).to(DEV)
        loss1, res1 = chain_loss(xs, _den(), one, xent_input=xxs if use_xent else None, **kw1)
        g1 = torch.autograd.grad(loss1, (xs, xxs) if use_xent else (xs,))
        objf += float(res1.data.numpy()[0])
        a, b = g[rows], back1(g1[0]).reshape(Ts, -1).float().cpu().numpy()
        assert np.array_equal(a, b), (layout, mode, s)  # in value (+0 == -0) ...
        if dtype == torch.float32:  # ... and in bits where the value is not an exact zero
            nz = b != 0
            assert np.array_equal(_bits(a)[nz], _bits(b)[nz])
        if use_xent:
            assert np.array_equal(gx[rows], back1(g1[1]).reshape(Ts, -1).float().cpu().numpy()), (layout, mode, s)
    assert abs(r[0] - objf) <= 1e-5 * abs(objf)


def test_warm_steps_allocate_nothing():
    name = "chain"
    lens, fsts = rc.lengths(name), rc.fsts(name)
    S, T = len(lens), max(lens)
    x, _ = _as_layout(rc.with_padding(rc.nnet_output(name), lens, np.nan), S, T, "bct", torch.float32)
    x.requires_grad_(True)
    kw = dict(l2_regularize=rc.L2, leaky_hmm_coefficient=rc.LEAKY)

    def step():
        sup = io.Supervision.from_e2e_fsts(rc.WEIGHT, list(lens), rc.P, fsts)  # (a fresh handle every step, as a reader's)
        loss, _ = chain_loss(x, _den(), sup, **kw)
        return torch.autograd.grad(loss, x)[0]

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    # (the counter test_gpu_e2e.py reads: a warm pool hands the tables', the lengths' and the scratch's slot out again)
    before = _counter("pool_device_allocs")
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    assert _counter("pool_device_allocs") == before


def test_captured_step_replays():
    name = "chain"
    lens, fsts = rc.lengths(name), rc.fsts(name)
    S, T = len(lens), max(lens)
    sup = io.Supervision.from_e2e_fsts(rc.WEIGHT, list(lens), rc.P, fsts)
    kw = dict(l2_regularize=rc.L2, leaky_hmm_coefficient=rc.LEAKY, xent_regularize=0.1, kaldi_way=True)
    x, _ = _as_layout(rc.with_padding(rc.nnet_output(name), lens, np.nan), S, T, "bct", torch.float32)
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
    with torch.cuda.graph(cg, stream=side):
        captured = step()
    cg.replay()
    torch.cuda.synchronize()
    got = [c.clone() for c in captured]
    want = step()
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
