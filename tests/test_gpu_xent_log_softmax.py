"""``chain_loss(..., xent_log_softmax=True)`` on the GPU (``tc_chain_step_log_softmax``, ``csrc/xent_softmax_kernels.hip``, DESIGN
4.14; cases and the float64 statement of the contract: ``tests/xent_log_softmax_cases.py``).

The yardstick of the gradient is the route callers took before the option: ``F.log_softmax(x, dim=1)`` in the tensor's dtype
in front of the call and autograd through it.  Both routes are held against ``G64 = V64 - rowsum(V64) * softmax64(x)``, V being
the float32 xent gradient of the default call on the same (widened) inputs, and the fused call's worst ``|G - G64| /
max|rowsum(V)|`` must stay within 4 times the other route's: 4096 to 10240 terms are summed in another order and the kernels'
``expf`` stands against torch's.  Row sums of the live rows are held the same way against the other route's own row sums.  The
cross-entropy objective is held to 1e-6 relative of the float64 objective, the project's tolerance for ``xent_objf``
(``tests/composed_step.py``).  Everything else is compared bit for bit."""
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss

import xent_log_softmax_cases as xc
from helpers import free_port

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
# (layout, dtype): 2-D float32 rows (dense and with a padded row stride), (B, C, T) in the three dtypes, a batch-first
# channel-last view, a time-major view; the widened scratch of 16-bit rows and the gathered scratch of a 16-bit view
CONFIGS = (("rows", F32), ("rows_padded", F32), ("bct", F32), ("bct", BF16), ("bct", F16), ("batch_first", F32),
           ("time_major", F32), ("rows", BF16), ("batch_first", F16))
_ids = ["%s-%s" % (lay, str(dt).replace("torch.", "")) for lay, dt in CONFIGS]
OBJF_REL = 1e-6
RATIO = 4.0


def _counter(name):
    return int(lib.tc_debug_counter(name.encode()))


@pytest.fixture(autouse=True)
def _fixed_kernel_choice(kernel_family):
    kernel_family("no_tune")  # (no timing launches: the counters of this module move by the steps alone)


_graphs, _sups = {}, {}


def _graph(name):
    if name not in _graphs:
        _graphs[name] = io.DenominatorGraph(xc.den_fst(name), xc.SHAPES[name][2])
    return _graphs[name].prepare(0)


def _sup(name):
    if name not in _sups:
        _sups[name] = io.Supervision.from_synth(xc.supervision(name))
    return _sups[name]


def _ragged_sup():
    if "ragged" not in _sups:
        _sups["ragged"] = io.Supervision.from_sequences(list(xc.ragged_pieces()))
    return _sups["ragged"]


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == F32 else (t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int16))


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _plus_zero(t):
    return not bool(_bits(t).any())


def _as_layout(m2d, S, T, layout, dtype):
    """The (T * S, P) float32 matrix as a chain_loss tensor of the layout and dtype; returns (tensor, its gradient -> (T, S, P))."""
    t = torch.from_numpy(np.array(m2d, np.float32)).to(DEV).view(T, S, -1)
    P = t.shape[2]
    if layout == "rows":
        return t.reshape(T * S, P).to(dtype), lambda g: g.view(T, S, P)
    if layout == "rows_padded":  # (13 -> 16, 4096 -> 4100: float4 rows with and without a tail behind them)
        wide = torch.zeros(T * S, (P + 4) & ~3, dtype=dtype, device=DEV)
        wide[:, :P] = t.reshape(T * S, P).to(dtype)
        return wide[:, :P], lambda g: g.view(T, S, P)
    if layout == "bct":
        return t.permute(1, 2, 0).contiguous().to(dtype), lambda g: g.permute(2, 0, 1)
    if layout == "batch_first":
        return t.permute(1, 0, 2).contiguous().to(dtype).permute(0, 2, 1), lambda g: g.permute(2, 0, 1)
    assert layout == "time_major"
    return t.contiguous().to(dtype).permute(1, 2, 0), lambda g: g.permute(2, 0, 1)


def _rounded(m2d, dtype):
    """The matrix as the tensor of ``dtype`` holds it, widened back to float32 (exact)."""
    return torch.from_numpy(np.array(m2d, np.float32)).to(dtype).float().numpy()


Out = namedtuple("Out", "loss data xent g gx seq failed results")


def _step(y, x, sup, graph, S, T, layout="rows", dtype=F32, route="fused", dw=None, grad=True, **opts):
    """One chain_loss step with the xent branch, Kaldi's way.  ``route``: "default" (the option off: the gradient V), "fused"
    (the option on) or "torch" (``F.log_softmax`` in front of the default call and autograd through it).  Gradients come back
    as (T * S, P) tensors of the input's dtype, rows ``t * S + s``."""
    yt, back = _as_layout(np.array(y, np.float32), S, T, layout, dtype)
    xt, _ = _as_layout(np.array(x, np.float32), S, T, layout, dtype)
    kw = dict(l2_regularize=xc.L2, leaky_hmm_coefficient=xc.LEAKY, xent_regularize=xc.XREG, kaldi_way=True)
    if dw is not None:
        kw["deriv_weights"] = torch.from_numpy(np.asarray(dw, np.float32)).to(DEV)
    if route == "fused":
        kw["xent_log_softmax"] = True
    kw.update(opts)
    flat = lambda g: back(g).contiguous().view(T * S, -1)  # noqa: E731
    if not grad:
        with torch.no_grad():
            loss, res = chain_loss(yt, graph, sup, xent_input=F.log_softmax(xt, dim=1) if route == "torch" else xt, **kw)
        torch.cuda.synchronize()
        return Out(loss.clone(), res.data.clone(), res.xent_objf, None, None, res.per_sequence, res.failed, res)
    yt = yt.detach().requires_grad_(True)
    xt = xt.detach().requires_grad_(True)
    loss, res = chain_loss(yt, graph, sup, xent_input=F.log_softmax(xt, dim=1) if route == "torch" else xt, **kw)
    g, gx = torch.autograd.grad(loss, (yt, xt))
    torch.cuda.synchronize()
    return Out(loss.detach().clone(), res.data.clone(), res.xent_objf, flat(g), flat(gx), res.per_sequence, res.failed, res)


def _f64(t):
    return t.double().cpu().numpy()


def _figures(out, V32, x_widened, live=None):
    """(worst |G - G64| / max|rowsum V|, worst |rowsum G| / max|rowsum V|) of a step's xent gradient over the rows ``live``."""
    G64 = xc.grad64(V32, x_widened)
    mass = xc.row_mass(V32)
    G = _f64(out.gx)
    rows = slice(None) if live is None else live
    return float(np.abs(G - G64)[rows].max() / mass), float(np.abs(G.sum(axis=1))[rows].max() / mass)


def _hold_to_the_torch_route(tag, fused, torch_route, V32, x_widened, live=None):
    fe, fs = _figures(fused, V32, x_widened, live)
    te, ts = _figures(torch_route, V32, x_widened, live)
    print("%s: |G - G64| / row mass: fused %.3e, torch route %.3e (ratio %.2f); |rowsum G| / row mass: fused %.3e, torch route %.3e"
          % (tag, fe, te, fe / te if te else float("inf"), fs, ts))
    assert fe <= RATIO * te, (fe, te)
    assert fs <= RATIO * max(ts, te), (fs, ts, te)


_references = {}


def _reference(name, dtype):
    """Per case and dtype, once: the widened inputs, the default call's float32 gradient V on them (2-D rows), the float64
    objective of its entries."""
    key = (name, dtype)
    if key not in _references:
        S, T, _ = xc.SHAPES[name]
        y, x = _rounded(xc.chain_input(name), dtype), _rounded(xc.xent_input(name), dtype)
        V = _step(y, x, _sup(name), _graph(name), S, T, route="default").gx.cpu().numpy()
        _references[key] = (y, x, V, xc.objective64(V.astype(np.float64) / -xc.XREG, x))
    return _references[key]


# ---- 1. gradient, row sums, objective; everything else unchanged -----------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype", CONFIGS, ids=_ids)
@pytest.mark.parametrize("name", xc.CASES)
def test_gradient_and_objective_against_float64(name, layout, dtype):
    S, T, P = xc.SHAPES[name]
    y, x, V, objf64 = _reference(name, dtype)
    assert (V != 0).any(axis=1).all() and np.isfinite(V).all()  # (every row carries posteriors)
    graph, sup = _graph(name), _sup(name)
    default = _step(y, x, sup, graph, S, T, layout, dtype, route="default")
    before = _counter("xent_log_softmax_launches")
    fused = _step(y, x, sup, graph, S, T, layout, dtype, route="fused")
    assert _counter("xent_log_softmax_launches") == before + 2  # (the row statistics and the gradient pass)
    via_torch = _step(y, x, sup, graph, S, T, layout, dtype, route="torch")
    assert fused.gx.dtype == dtype and bool(torch.isfinite(fused.gx).all())
    _hold_to_the_torch_route("%s %s %s" % (name, layout, dtype), fused, via_torch, V, x)
    print("xent_objf %.12g (float64 %.12g, torch route %.12g)" % (fused.xent, objf64, via_torch.xent))
    assert abs(fused.xent - objf64) <= OBJF_REL * abs(objf64)
    # the chain output's side does not move by a bit
    assert _same(fused.data, default.data) and _same(fused.loss, default.loss) and _same(fused.g, default.g)


# ---- 2. the option off --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype", CONFIGS, ids=_ids)
def test_option_off_is_the_default_call(layout, dtype):
    name = "ragged_float4"
    S, T, _ = xc.SHAPES[name]
    y, x, _, _ = _reference(name, dtype)
    default = _step(y, x, _sup(name), _graph(name), S, T, layout, dtype, route="default")
    before = _counter("xent_log_softmax_launches")
    off = _step(y, x, _sup(name), _graph(name), S, T, layout, dtype, route="default", xent_log_softmax=False)
    seq = _step(y, x, _sup(name), _graph(name), S, T, layout, dtype, route="default", xent_log_softmax=False, per_sequence=True)
    assert _counter("xent_log_softmax_launches") == before
    for got in (off, seq):
        assert _same(got.data, default.data) and _same(got.loss, default.loss) and got.xent == default.xent
        assert _same(got.g, default.g) and _same(got.gx, default.gx)
    # without the xent branch the option does nothing
    yt, _ = _as_layout(np.array(y), S, T, layout, dtype)
    yt.requires_grad_(True)
    a, ra = chain_loss(yt, _graph(name), _sup(name), l2_regularize=xc.L2, leaky_hmm_coefficient=xc.LEAKY, kaldi_way=True)
    ga = torch.autograd.grad(a, yt)[0]
    b, rb = chain_loss(yt, _graph(name), _sup(name), l2_regularize=xc.L2, leaky_hmm_coefficient=xc.LEAKY, kaldi_way=True,
                       xent_log_softmax=True)
    gb = torch.autograd.grad(b, yt)[0]
    torch.cuda.synchronize()
    assert _same(ga, gb) and _same(ra.data, rb.data) and rb.xent_objf is None
    assert _counter("xent_log_softmax_launches") == before


# ---- 3. ragged minibatches ---------------------------------------------------------------------------------------------------------------
def _ragged_inputs(dtype, pad):
    S, T = len(xc.RAGGED_LENGTHS), max(xc.RAGGED_LENGTHS)
    y = np.array(_rounded(xc.chain_input("ragged_float4", S, T), dtype))
    x = np.array(_rounded(xc.xent_input("ragged_float4", S, T), dtype))
    live = np.array([t < xc.RAGGED_LENGTHS[s] for t in range(T) for s in range(S)])
    x[~live] = pad
    return S, T, y, x, live


@pytest.mark.parametrize("layout,dtype", CONFIGS, ids=_ids)
def test_ragged_padding_is_plus_zero_and_is_not_read(layout, dtype):
    name = "ragged_float4"
    graph, sup = _graph(name), _ragged_sup()
    S, T, y, x, live = _ragged_inputs(dtype, 0.25)
    V = _step(y, x, sup, graph, S, T, route="default").gx.cpu().numpy()
    assert not V[~live].any() and (V[live] != 0).any(axis=1).all()
    fused = _step(y, x, sup, graph, S, T, layout, dtype, route="fused", per_sequence=True)
    via_torch = _step(y, x, sup, graph, S, T, layout, dtype, route="torch")
    _hold_to_the_torch_route("ragged %s %s" % (layout, dtype), fused, via_torch, V, x, live)
    assert _plus_zero(fused.gx[torch.from_numpy(~live).to(DEV)])
    objf64 = xc.objective64(V.astype(np.float64) / -xc.XREG, x)
    assert abs(fused.xent - objf64) <= OBJF_REL * abs(objf64)
    # the sequences' own sums, scaled as the library's sum, add up to the objective
    total = float(fused.seq.xent_sum.sum()) / -xc.XREG
    assert abs(total - fused.xent) <= 1e-12 * abs(fused.xent) and fused.failed.numel() == 0
    # NaN in the padding of xent_input changes nothing
    _, _, _, x_nan, _ = _ragged_inputs(dtype, np.nan)
    again = _step(y, x_nan, sup, graph, S, T, layout, dtype, route="fused", per_sequence=True)
    assert _same(again.gx, fused.gx) and again.xent == fused.xent and _same(again.g, fused.g) and _same(again.data, fused.data)
    assert _same(again.seq.xent_sum, fused.seq.xent_sum)


# ---- 4. deriv_weights --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype", CONFIGS, ids=_ids)
def test_deriv_weights_scale_the_rows_and_a_zero_weight_row_is_plus_zero(layout, dtype):
    name = "ragged_float4"
    S, T, _ = xc.SHAPES[name]
    graph, sup = _graph(name), _sup(name)
    y, x, V, objf64 = _reference(name, dtype)
    dw = np.random.default_rng(11).uniform(0.25, 2.0, size=S * T).astype(np.float32)
    dead = 4
    dw[dead] = 0.0
    Vw = _step(y, x, sup, graph, S, T, route="default", dw=dw).gx.cpu().numpy()
    assert not Vw[dead].any()
    keep = np.arange(S * T) != dead
    fused = _step(y, x, sup, graph, S, T, layout, dtype, route="fused", dw=dw)
    via_torch = _step(y, x, sup, graph, S, T, layout, dtype, route="torch", dw=dw)
    _hold_to_the_torch_route("deriv_weights %s %s" % (layout, dtype), fused, via_torch, Vw, x, keep)
    assert _plus_zero(fused.gx[dead])
    # the other rows are dw[row] times the unweighted gradient, within the same bound (relative to the weighted row mass)
    G64 = dw[:, None].astype(np.float64) * xc.grad64(V, x)
    err = float(np.abs(_f64(fused.gx) - G64)[keep].max() / xc.row_mass(Vw))
    te, _ = _figures(via_torch, Vw, x, keep)
    print("dw * unweighted: %.3e (torch route against its own V: %.3e)" % (err, te))
    assert err <= RATIO * te
    # the objective ignores the weights
    assert abs(fused.xent - objf64) <= OBJF_REL * abs(objf64)
    # NaN in the row of weight 0: its gradient is still +0 (a select, not a product), the other rows keep their bits; the
    # objective, which ignores the weights, is NaN
    x_nan = np.array(x)
    x_nan[dead] = np.nan
    poisoned = _step(y, x_nan, sup, graph, S, T, layout, dtype, route="fused", dw=dw)
    assert _plus_zero(poisoned.gx[dead]) and _same(poisoned.gx, fused.gx)
    assert poisoned.xent != poisoned.xent
    assert _same(poisoned.g, fused.g) and _same(poisoned.data, fused.data)


# ---- 5. failures -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype", CONFIGS, ids=_ids)
def test_a_failed_sequence_is_plus_zero_and_the_objective_is_the_survivors(layout, dtype):
    name = "ragged_float4"
    S, T, _ = xc.SHAPES[name]
    graph, sup = _graph(name), _sup(name)
    y, x, _, _ = _reference(name, dtype)
    bad = 1
    clean = _step(y, x, sup, graph, S, T, layout, dtype, route="fused", on_failure="sequence")
    assert clean.failed.numel() == 0
    y_bad = np.array(y)
    y_bad[bad::S] = np.nan  # (every frame of the sequence, through the chain input)
    got = _step(y_bad, x, sup, graph, S, T, layout, dtype, route="fused", on_failure="sequence")
    assert got.failed.tolist() == [bad], got.seq.status
    rows_bad = torch.arange(S * T, device=DEV) % S == bad
    assert _plus_zero(got.gx[rows_bad]) and _plus_zero(got.g[rows_bad])
    assert _same(got.gx[~rows_bad], clean.gx[~rows_bad]) and _same(got.g[~rows_bad], clean.g[~rows_bad])
    survivors = [s for s in range(S) if s != bad]
    assert _same(got.seq.xent_sum[survivors], clean.seq.xent_sum[survivors])
    want = float(clean.seq.xent_sum[survivors].sum()) / -xc.XREG
    assert abs(got.xent - want) <= 1e-12 * abs(want), (got.xent, want)


@pytest.mark.parametrize("layout,dtype", CONFIGS, ids=_ids)
def test_soft_failure_of_the_whole_minibatch_is_all_plus_zero(layout, dtype):
    name = "ragged_float4"
    S, T, _ = xc.SHAPES[name]
    y, x, _, _ = _reference(name, dtype)
    y_bad = np.array(y)
    y_bad[0] = np.nan  # (one NaN: the reference's route gives up the whole minibatch)
    for opts in ({}, {"on_failure": "sequence"}):
        y_all = np.full_like(y_bad, np.nan) if opts else y_bad  # (isolating: every sequence failed is the same route)
        got = _step(y_all, x, _sup(name), _graph(name), S, T, layout, dtype, route="fused", **opts)
        assert float(got.data[0]) == float(np.float32(-10.0) * np.float32(float(got.data[2])))  # (the failure route's objf)
        assert _plus_zero(got.gx), got.gx


def test_a_non_finite_xent_input_stays_in_its_row():
    """NaN, +inf and -inf in a live row of ``xent_input``: that row's gradient and the objective are non-finite, the row's
    sequence reports a non-finite ``xent_sum`` and status bit 1; every other row keeps its bits."""
    name = "ragged_float4"
    S, T, _ = xc.SHAPES[name]
    y, x, _, _ = _reference(name, F32)
    for layout in ("rows", "bct", "batch_first"):
        clean = _step(y, x, _sup(name), _graph(name), S, T, layout, F32, route="fused", per_sequence=True)
        for row, value in ((5, np.nan), (7, np.inf), (9, -np.inf)):
            x_bad = np.array(x)
            x_bad[row, 3] = value
            got = _step(y, x_bad, _sup(name), _graph(name), S, T, layout, F32, route="fused", per_sequence=True)
            others = torch.arange(S * T, device=DEV) != row
            assert not bool(torch.isfinite(got.gx[row]).any()), (layout, value, got.gx[row])
            assert _same(got.gx[others], clean.gx[others]) and _same(got.g, clean.g) and _same(got.data, clean.data)
            assert not np.isfinite(got.xent)
            s = row % S
            assert not bool(torch.isfinite(got.seq.xent_sum[s])) and int(got.seq.status[s]) & 1
            rest = [q for q in range(S) if q != s]
            assert _same(got.seq.xent_sum[rest], clean.seq.xent_sum[rest]) and not got.seq.status[rest].any()


# ---- 6. the evaluation step, capture, determinism ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype", CONFIGS, ids=_ids)
def test_evaluation_step_returns_the_objective_and_launches_no_backward(layout, dtype):
    name = "full_row"
    S, T, _ = xc.SHAPES[name]
    y, x, _, _ = _reference(name, dtype)
    train = _step(y, x, _sup(name), _graph(name), S, T, layout, dtype, route="fused")
    before = _counter("den_backward_launches"), _counter("xent_log_softmax_launches")
    got = _step(y, x, _sup(name), _graph(name), S, T, layout, dtype, route="fused", grad=False)
    assert _counter("den_backward_launches") == before[0]
    assert _counter("xent_log_softmax_launches") == before[1] + 1  # (the row statistics; no gradient pass)
    assert got.xent == train.xent and _same(got.data, train.data) and _same(got.loss, train.loss)


@pytest.mark.parametrize("layout", ("rows", "bct", "batch_first"))
def test_captured_step_replays_the_eager_bits(layout):
    name = "tile_edge" if layout == "bct" else "ragged_float4"
    S, T, P = xc.SHAPES[name]
    graph, sup = _graph(name), _sup(name)
    yt, _ = _as_layout(np.array(xc.chain_input(name)), S, T, layout, F32)
    xt, _ = _as_layout(np.array(xc.xent_input(name)), S, T, layout, F32)
    yt, xt = yt.detach().requires_grad_(True), xt.detach().requires_grad_(True)
    kw = dict(l2_regularize=xc.L2, leaky_hmm_coefficient=xc.LEAKY, xent_regularize=xc.XREG, kaldi_way=True, xent_log_softmax=True)
    seen = []

    def step():
        loss, res = chain_loss(yt, graph, sup, xent_input=xt, **kw)
        g, gx = torch.autograd.grad(loss, (yt, xt))
        seen.append(res)
        return loss.detach(), g, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()  # (warm-up outside the capture: tables, pools, side streams)
    side.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        captured = step()
    captured_results = seen[-1]
    for seed in (21, 22):
        gen = torch.Generator(device=DEV).manual_seed(seed)
        with torch.no_grad():
            yt.copy_(torch.randn(yt.shape, device=DEV, generator=gen))
            xt.copy_(3.0 * torch.randn(xt.shape, device=DEV, generator=gen))
        before = _counter("xent_log_softmax_launches")
        cg.replay()
        torch.cuda.synchronize()
        assert _counter("xent_log_softmax_launches") == before  # (no library call: the graph's own nodes ran)
        got = [t.clone() for t in captured]
        captured_results.invalidate()
        got_xent = captured_results.xent_objf
        want = step()
        torch.cuda.synchronize()
        assert got_xent == seen[-1].xent_objf and float(got[2].abs().max()) > 0
        for a, b in zip(got, want):
            assert _same(a, b)


@pytest.mark.parametrize("layout,dtype", (("rows", F32), ("bct", F32), ("bct", BF16), ("batch_first", F32)))
@pytest.mark.parametrize("name", ("full_row", "two_passes"))
def test_two_runs_give_the_same_bits(name, layout, dtype):
    S, T, _ = xc.SHAPES[name]
    y, x, _, _ = _reference(name, dtype)
    a = _step(y, x, _sup(name), _graph(name), S, T, layout, dtype, route="fused", per_sequence=True)
    b = _step(y, x, _sup(name), _graph(name), S, T, layout, dtype, route="fused", per_sequence=True)
    assert _same(a.gx, b.gx) and _same(a.g, b.g) and a.xent == b.xent and _same(a.seq.xent_sum, b.seq.xent_sum)


# ---- 7. data parallel ----------------------------------------------------------------------------------------------------------------------
DP_S, DP_T, DP_P = 3, 6, 64


def _dp_inputs():
    fst = synth.random_den_fst(40, 3, DP_P, seed=81)
    sup = synth.random_supervision(fst, DP_S, DP_T, 1, seed=82, weight=xc.WEIGHT, initial_probs=synth.initial_probs_f64(fst))
    y = synth.random_nnet_output(DP_S, DP_T, DP_P, seed=83)
    x = synth.random_nnet_output(DP_S, DP_T, DP_P, seed=84, scale=3.0)
    return fst, sup, y, x


def _dp_worker(rank, world, port, out_dir):
    """One rank: its shard through ``chain_loss_data_parallel(..., xent_log_softmax=True)`` on cuda:0 (the ranks share the
    test box's GPU; the collective travels over gloo)."""
    import os

    import torch.distributed as dist

    from torchain_amd import parallel

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        fst, sup, y, x = _dp_inputs()
        lo, hi = parallel.shard_range(DP_S, rank, world)
        den = io.DenominatorGraph(fst, DP_P)
        hsup = io.Supervision.from_synth(parallel.shard_supervision_fst(sup, lo, hi))
        yl = parallel.shard_rows(torch.from_numpy(y), DP_S, lo, hi).contiguous().to(DEV).requires_grad_(True)
        xl = parallel.shard_rows(torch.from_numpy(x), DP_S, lo, hi).contiguous().to(DEV).requires_grad_(True)
        loss, res = parallel.chain_loss_data_parallel(yl, den, hsup, xc.L2, xc.LEAKY, xc.XREG, xl, kaldi_way=True,
                                                      xent_log_softmax=True)
        gx = torch.autograd.grad(loss, xl)[0]
        torch.cuda.synchronize()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), xent=res.xent_objf, gx=gx.cpu().numpy(), data=res.data.numpy())
    finally:
        dist.destroy_process_group()


def test_data_parallel_objective_is_the_single_rank_one(tmp_path):
    import torch.multiprocessing as mp

    from torchain_amd import parallel

    fst, sup, y, x = _dp_inputs()
    den, hsup = io.DenominatorGraph(fst, DP_P), io.Supervision.from_synth(sup)
    yt = torch.from_numpy(y).to(DEV).requires_grad_(True)
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    loss, res = chain_loss(yt, den, hsup, xc.L2, xc.LEAKY, xc.XREG, xt, kaldi_way=True, xent_log_softmax=True)
    gx = torch.autograd.grad(loss, xt)[0].cpu()
    want = res.xent_objf
    world = 2
    mp.spawn(_dp_worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [np.load(str(tmp_path / ("rank%d.npz" % k))) for k in range(world)]
    assert float(r[0]["xent"]) == float(r[1]["xent"])
    assert abs(float(r[0]["xent"]) - want) <= OBJF_REL * abs(want), (float(r[0]["xent"]), want)
    for k in range(world):
        lo, hi = parallel.shard_range(DP_S, k, world)
        # (the term is per row of the local shard: a rank's rows are the full batch's rows of its own sequences, bit for bit)
        assert np.array_equal(r[k]["gx"], parallel.shard_rows(gx, DP_S, lo, hi).numpy())
