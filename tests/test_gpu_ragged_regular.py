"""Ragged REGULAR supervisions (io.Supervision.from_sequences, tc_supervision_create_ragged) on the GPU: the RAGGED
instantiations of the resident and the level-windowed numerator kernel alone, then the objective and chain_loss in every
layout.  Cases and float64 references: tests/ragged_regular_cases.py (sums over sequences of single-sequence references).
Beside the references, every valid row of the numerator is held to THE BITS of the uniform call on that sequence alone, and
every padding element to +0."""
import numpy as np
import pytest
import torch

from torchain_amd import egs, io
from torchain_amd._lib import TorchainHipError, lib
from torchain_amd.functions import ChainResults, chain_loss, compute_chain_objf_and_deriv

import num_elementwise_cases as nc
import ragged_cases as rc
import ragged_regular_cases as rr
import row_contract_cases as rcc
from helpers import REL, hip_num, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TC_ERR_UNSUPPORTED = -3
SENTINEL = rcc.SENTINEL


def _counter(name):
    return int(lib.tc_debug_counter(name.encode()))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- a. the numerator alone ------------------------------------------------------------------------------------------------------
def _elementwise(got, want, weight, rel, what):
    """test_gpu_ragged.py::_elementwise: every entry above 1e-8 * weight within ``rel`` relative, every other within
    1e-9 * weight, exactly 0 where the reference is, rows summing to the weight."""
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


@pytest.mark.parametrize("name,forced", [(n, False) for n in rr.NUMERATOR] + [(n, True) for n in rr.FITS_RESIDENT])
def test_numerator(name, forced, kernel_family):
    lens, pieces, w = rr.lengths(name), rr.pieces(name), rr.weight(name)
    sup = rr.handle(name)
    stats = sup.stats()
    if name == "trie":
        assert stats["kernel"] == "resident" and not nc.staged_in_lds(stats)
    if name == "small":
        assert stats["kernel"] == "resident" and nc.staged_in_lds(stats)
    if name == "wide":
        assert stats["kernel"] == "windowed"
    if forced:
        kernel_family("force_num_windowed")
    y = rc.with_padding(rr.nnet_output(name), lens, np.nan)
    windowed = _counter("num_windowed_launches")
    out = hip_num(sup, y, init=0.0)
    assert _counter("num_windowed_launches") == windowed + (1 if forced or name == "wide" else 0)
    kept = hip_num(sup, y, init=SENTINEL)
    pad = rc.padding_rows(lens)
    assert not _bits(out["deriv"][pad]).any()                     # +0: nothing was added to the padding
    assert np.all(kept["deriv"][pad] == np.float32(SENTINEL))     # ... and nothing written there
    assert kept["logprob_weighted"] == out["logprob_weighted"]
    want_lp, want = rr.num_reference(name)
    for s, Ts in enumerate(lens):
        rows = rc.valid_rows(lens, s)
        _elementwise(out["deriv"][rows], want[rows], w, nc.REL_REGULAR, "%s sequence %d (%d frames)" % (name, s, Ts))
        # the uniform call on the sequence alone, whichever kernel it takes
        one = hip_num(io.Supervision.from_fst(w, 1, Ts, pieces[s].label_dim, pieces[s].arc_begin, pieces[s].ilabel,
                                              pieces[s].arc_weight, pieces[s].nextstate, pieces[s].final),
                      rr.sequence_rows(name, s), init=0.0)
        assert np.array_equal(_bits(out["deriv"][rows]), _bits(one["deriv"])), (name, s)
    print("%s: weighted log-prob %.12g, float64 %.12g" % (name, out["logprob_weighted"], want_lp))
    assert abs(out["logprob_weighted"] - want_lp) <= nc.REL_LOGPROB * abs(want_lp)
    # forward only: the same log-prob
    assert hip_num(sup, y, want_deriv=False)["logprob_weighted"] == out["logprob_weighted"]


@pytest.mark.parametrize("forced", [False, True])
def test_equal_lengths_give_the_merged_uniform_handles_bits(forced, kernel_family):
    if forced:
        kernel_family("force_num_windowed")
    pieces = rr.pieces("equal")
    y = np.array(rr.nnet_output("equal"))
    ragged = hip_num(io.Supervision.from_sequences(pieces), y, init=0.0)
    uniform = hip_num(io.Supervision.from_synth(egs.append_supervisions(list(pieces))), y, init=0.0)
    assert np.array_equal(_bits(ragged["deriv"]), _bits(uniform["deriv"]))
    assert ragged["logprob_weighted"] == uniform["logprob_weighted"]
    want_lp, want = rr.num_reference("equal")
    assert abs(ragged["logprob_weighted"] - want_lp) <= nc.REL_LOGPROB * abs(want_lp)
    for s in range(len(pieces)):
        rows = rc.valid_rows(rr.lengths("equal"), s)
        _elementwise(ragged["deriv"][rows], want[rows], rr.weight("equal"), nc.REL_REGULAR, "equal sequence %d" % s)


# ---- b. the objective ------------------------------------------------------------------------------------------------------------
_graphs = {}
NAME = "small"


def _den():
    if "g" not in _graphs:
        import wide_supervisions as ws
        _graphs["g"] = io.DenominatorGraph(ws.den_fst(), rr.P).prepare(0)
    return _graphs["g"]


def _hip(sup, y, xent=False, graph=None, l2=rr.L2, leaky=rr.LEAKY):
    yt = torch.from_numpy(np.array(y, dtype=np.float32)).to(DEV)
    deriv = torch.full(yt.shape, 7.0, device=DEV)
    xd = torch.full(yt.shape, 7.0, device=DEV) if xent else None
    res = ChainResults()
    compute_chain_objf_and_deriv(graph or _den(), sup, yt, res.data, deriv, xd, l2, leaky, 0.1 if xent else 0.0)
    torch.cuda.synchronize()
    return res.data.numpy().copy(), deriv.cpu().numpy(), None if xd is None else xd.cpu().numpy()


def _check(got_res, got_d, got_x, want, w, lens, what):
    """objf, l2_term, weight, deriv and xent_deriv within helpers.REL; the weight is also the float32 product the library
    forms.  The derivatives are compared matrix-wise on the scale of the supervision's weight (helpers.rel_err)."""
    print("%s: objf %.9g (oracle %.9g), l2 %.9g (%.9g), weight %.9g, deriv rel %.2e" % (
        what, got_res[0], want["objf"], got_res[1], want["l2_term"], got_res[2], rel_err(got_d, want["deriv"], floor=w)))
    assert abs(got_res[0] - want["objf"]) <= REL * abs(want["objf"]), (got_res, want["objf"])
    assert abs(got_res[1] - want["l2_term"]) <= REL * abs(want["l2_term"]) + 1e-30, (got_res, want["l2_term"])
    assert got_res[2] == np.float32(w) * np.float32(sum(lens))
    assert abs(got_res[2] - want["weight"]) <= REL * want["weight"]
    assert rel_err(got_d, want["deriv"], floor=w) <= REL
    if got_x is not None:
        assert rel_err(got_x, want["xent_deriv"], floor=w) <= REL


@pytest.mark.parametrize("xent", [False, True])
def test_objective(xent):
    lens, w = rr.lengths(NAME), rr.weight(NAME)
    y = rc.with_padding(rr.nnet_output(NAME), lens, np.nan)
    sup = rr.handle(NAME)
    steps = _counter("ragged_steps")
    res, d, xd = _hip(sup, y, xent=xent)
    assert _counter("ragged_steps") == steps + 1
    _check(res, d, xd, rr.reference(NAME), w, lens, "2-D objective xent=%d" % xent)
    pad = rc.padding_rows(lens)
    assert not _bits(d[pad]).any()
    if xent:
        assert not _bits(xd[pad]).any()
    again = _hip(sup, y, xent=xent)
    for a, b in zip((res, d, xd), again):
        assert (a is None and b is None) or np.array_equal(_bits(a), _bits(b))


def test_nan_in_a_valid_frame_fails_softly():
    lens, w = rr.lengths(NAME), rr.weight(NAME)
    S = len(lens)
    s = int(np.argmin(lens))
    piece = rr.pieces(NAME)[s]
    y = rc.with_padding(rr.nnet_output(NAME), lens, 3.0)
    y[(lens[s] - 1) * S + s, int(piece.ilabel[0]) - 1] = np.nan  # a pdf that an arc of the shortest sequence's last frame reads
    res, d, xd = _hip(rr.handle(NAME), y, xent=True)
    assert res[0] == np.float32(-10.0) * (np.float32(w) * np.float32(sum(lens)))
    pad = rc.padding_rows(lens)
    assert not _bits(d[pad]).any() and not _bits(xd).any()
    want = -w * rr.L2 * y[~pad].astype(np.float64)
    ok = np.isfinite(want)
    np.testing.assert_allclose(d[~pad][ok], want[ok], rtol=1e-6, atol=0)
    assert np.isnan(d[~pad][~ok]).all() and (~ok).sum() == 1


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_padding_values_change_no_bit(value):
    lens = rr.lengths(NAME)
    sup = rr.handle(NAME)
    clean = _hip(sup, rr.nnet_output(NAME), xent=True)
    dirty = _hip(sup, rc.with_padding(rr.nnet_output(NAME), lens, value), xent=True)
    assert clean[0][0] != np.float32(-10.0) * clean[0][2]
    for a, b in zip(clean, dirty):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("xent", [False, True])
def test_eight_sequences_take_two_workgroups_beside_the_ragged_numerator(xent, kernel_family):
    name = "eight"
    graph = rcc.den_graph(rcc.BY_NAME["tied8_two_cu"], kernel_family)
    assert graph.stats()["tied"] == 1
    lens, w = rr.lengths(name), rr.weight(name)
    y = rc.with_padding(rr.nnet_output(name), lens, np.nan)
    two = _counter("ragged_two_cu_launches")
    res, d, xd = _hip(rr.handle(name), y, xent=xent, graph=graph)
    assert _counter("ragged_two_cu_launches") == two + 1
    _check(res, d, xd, rr.reference(name), w, lens, "eight xent=%d" % xent)
    pad = rc.padding_rows(lens)
    assert not _bits(d[pad]).any() and (xd is None or not _bits(xd[pad]).any())


def test_streamed_graph_is_refused_before_any_launch(kernel_family):
    graph = rcc.den_graph(rcc.BY_NAME["streamed_narrow"], kernel_family)
    assert graph.stats()["tied"] == 2
    name = "eight"
    sup = rr.handle(name)
    yt = torch.from_numpy(np.array(rr.nnet_output(name))).to(DEV)
    deriv = torch.full(yt.shape, SENTINEL, device=DEV)
    res = ChainResults()
    keys = ("den_launches", "num_launches")
    before = [_counter(k) for k in keys]
    with pytest.raises(TorchainHipError) as e:
        compute_chain_objf_and_deriv(graph, sup, yt, res.data, deriv, None, rr.L2, rr.LEAKY, 0.0)
    torch.cuda.synchronize()
    assert e.value.code == TC_ERR_UNSUPPORTED
    assert [_counter(k) for k in keys] == before and bool((deriv == SENTINEL).all())
    x = yt.view(max(rr.lengths(name)), len(rr.lengths(name)), -1).permute(1, 2, 0).contiguous().requires_grad_(True)
    with pytest.raises(TorchainHipError) as e:
        chain_loss(x, graph, sup, l2_regularize=rr.L2, leaky_hmm_coefficient=rr.LEAKY)
    assert e.value.code == TC_ERR_UNSUPPORTED and [_counter(k) for k in keys] == before


# ---- c. chain_loss ---------------------------------------------------------------------------------------------------------------
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


_bf16_reference = {}


def _reference(dtype):
    """The float64-side reference of the outputs the step is given: rounded to bfloat16 for that dtype"""
    if dtype == torch.float32:
        return rr.reference(NAME)
    if "r" not in _bf16_reference:
        y = torch.from_numpy(np.array(rr.nnet_output(NAME))).to(torch.bfloat16).float().numpy()
        _bf16_reference["r"] = rr.ragged_objective(rr.oracle_graph(NAME), rr.pieces(NAME), rr.lengths(NAME), y)
    return _bf16_reference["r"]


LAYOUTS = [("bct", torch.float32), ("bct", torch.bfloat16), ("batch_first", torch.float32), ("time_major", torch.float32),
           ("rows", torch.float32)]
MODES = ["plain", "xent_kaldi", "xent_reference", "deriv_weights", "out_of_range", "no_grad"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout,dtype", LAYOUTS)
def test_chain_loss(layout, dtype, mode, kernel_family):
    kernel_family("no_phase_split")  # (the single-sequence calls onto the one-workgroup form a ragged batch of 5 takes)
    lens, pieces, w = rr.lengths(NAME), rr.pieces(NAME), rr.weight(NAME)
    S, T = len(lens), max(lens)
    pad = rc.padding_rows(lens)
    y = np.array(rr.nnet_output(NAME), copy=True)
    kw = dict(l2_regularize=rr.L2, leaky_hmm_coefficient=rr.LEAKY)
    dwt = None
    if mode in ("xent_kaldi", "xent_reference"):
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
    sup = rr.handle(NAME)
    x, back = _as_layout(y_in, S, T, layout, dtype)
    xx, _ = _as_layout(xe_in, S, T, layout, dtype)
    use_xent = "xent_regularize" in kw
    bf = dtype == torch.bfloat16
    want = _reference(dtype)
    # a bfloat16 gradient is the float32 one rounded to 8 significant bits: 2^-8 relative on top (test_gpu_ragged_two_cu.py)
    tol = REL + (2.0 ** -8 if bf else 0.0)

    if mode == "no_grad":
        # (without a cross-entropy output, as test_gpu_step.py's evaluation steps: its objective would need the posteriors)
        keys = ("num_launches", "num_backward_launches", "den_launches", "den_backward_launches")
        before = [_counter(k) for k in keys]
        with torch.no_grad():
            loss, res = chain_loss(x, _den(), sup, **kw)
        torch.cuda.synchronize()
        assert [_counter(k) - b for k, b in zip(keys, before)] == [1, 0, 1, 0]  # forward recursions only
        r = res.data.numpy()
        assert abs(r[0] - want["objf"]) <= REL * abs(want["objf"])
        assert abs(r[1] - want["l2_term"]) <= REL * abs(want["l2_term"])
        assert r[2] == np.float32(w) * np.float32(sum(lens))
        assert abs(float(loss) + r[0] / r[2]) <= (1e-2 if bf else 1e-6) * abs(float(loss))
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
    # the oracle's objective where it states what the call computes (kaldi_way=False: the objective of xent_input; out of range:
    # the penalty's term and the denominator's clamp; deriv_weights: rows of the gradient scaled -- those are held to the sum
    # of the single-sequence calls below)
    if mode in ("plain", "xent_kaldi"):
        print("%s %s %s: objf %.9g (oracle %.9g), gradient rel %.2e" % (layout, dtype, mode, r[0], want["objf"],
                                                                        rel_err(-g, want["deriv"], floor=w)))
        assert abs(r[0] - want["objf"]) <= REL * abs(want["objf"])
        assert abs(r[1] - want["l2_term"]) <= REL * abs(want["l2_term"])
        assert rel_err(-g, want["deriv"], floor=w) <= tol
        if use_xent:
            assert rel_err(-gx, 0.1 * want["xent_deriv"], floor=0.1 * w) <= tol
        if not bf:
            assert abs(float(loss.detach()) + r[0] / r[2]) <= 1e-6 * abs(float(loss.detach()))
    if mode == "deriv_weights" and not bf:
        assert rel_err(-g, want["deriv"] * dwt[:, None].astype(np.float64), floor=w) <= REL
    # padding: exactly zero, of either sign for nothing: +0
    assert not _bits(g[pad]).any()
    if use_xent:
        assert not _bits(gx[pad]).any()
    # valid positions: chain_loss on each sequence alone
    objf = 0.0
    for s, Ts in enumerate(lens):
        rows = rc.valid_rows(lens, s)
        one = io.Supervision.from_synth(pieces[s])
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
        if not bf:  # ... and in bits where the value is not an exact zero
            nz = b != 0
            assert np.array_equal(_bits(a)[nz], _bits(b)[nz])
        if use_xent:
            assert np.array_equal(gx[rows], back1(g1[1]).reshape(Ts, -1).float().cpu().numpy()), (layout, mode, s)
    assert abs(r[0] - objf) <= 1e-5 * abs(objf)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_channel_last_view_gives_the_contiguous_calls_bits(dtype):
    lens = rr.lengths(NAME)
    S, T = len(lens), max(lens)
    kw = dict(l2_regularize=rr.L2, leaky_hmm_coefficient=rr.LEAKY, xent_regularize=0.1, kaldi_way=True)
    y = rc.with_padding(rr.nnet_output(NAME), lens, np.nan)
    view, _ = _as_layout(y, S, T, "batch_first", dtype)
    xview, _ = _as_layout((0.5 * y).astype(np.float32), S, T, "batch_first", dtype)
    assert not view.is_contiguous() and view.shape == (S, rr.P, T)
    outs = []
    for x, xe in ((view, xview), (view.contiguous(), xview.contiguous())):
        x = x.detach().requires_grad_(True)
        xe = xe.detach().requires_grad_(True)
        loss, res = chain_loss(x, _den(), rr.handle(NAME), xent_input=xe, **kw)
        g, gx = torch.autograd.grad(loss, (x, xe))
        torch.cuda.synchronize()
        outs.append((loss.detach().float().cpu().numpy(), res.data.numpy().copy(), g.float().cpu().numpy(), gx.float().cpu().numpy()))
    for a, b in zip(*outs):
        assert np.array_equal(_bits(a), _bits(b))


def test_warm_steps_allocate_nothing():
    lens = rr.lengths("trie")
    S, T = len(lens), max(lens)
    x, _ = _as_layout(rc.with_padding(rr.nnet_output("trie"), lens, np.nan), S, T, "bct", torch.float32)
    x.requires_grad_(True)
    kw = dict(l2_regularize=rr.L2, leaky_hmm_coefficient=rr.LEAKY)

    def step():
        loss, _ = chain_loss(x, _den(), rr.handle("trie"), **kw)  # (a fresh handle every step, as a reader's)
        return torch.autograd.grad(loss, x)[0]

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    before = _counter("pool_device_allocs")
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    assert _counter("pool_device_allocs") == before
