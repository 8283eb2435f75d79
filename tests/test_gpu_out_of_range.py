"""The out-of-range penalty on the GPU (``chain_loss(..., out_of_range_regularize=c)``, ``tc_chain_step_penalized``):
``g' = fl32(g + t)`` with ``t = fl32(fl32(2c) * p)`` and ``p`` the part of the chain output beyond +-30, in front of
``deriv_weights``, rounded once for 16-bit outputs; results, loss, ``xent_objf`` and the xent gradient untouched.

Held bit for bit to the unpenalised call's float32 gradient plus the numpy statement of ``t`` (out_of_range_cases.py) on every
route -- (B, C, T), 2-D and 2-D with a row stride; float32 / bfloat16 / float16; without and with the cross-entropy branch
both ways of ``kaldi_way``; regular and end-to-end supervisions; every denominator kernel family; C3 -- and to the CPU oracle
under the project's matrix-wise tolerance.  Also: no effect where it should have none, soft failure, that it restores range
under SGD, the registered operator, stream capture, two data-parallel ranks and a recipe loop.  Every element is compared."""
import os

import numpy as np
import pytest
import torch

from torchain_amd import io, parallel, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss, compute_chain_objf_and_deriv, ChainResults

import e2e_reference as ref
import out_of_range_cases as oor
from helpers import REL, free_port, from3d, rel_err, to3d

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
LAYOUTS = ["3d", "2d", "2d_strided"]
XENT = [None, True, False]  # no cross-entropy branch, kaldi_way=True, kaldi_way=False
C = 0.01  # (Kaldi's default)
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
_COUNTERS = (b"den_launches", b"den_backward_launches", b"num_launches", b"num_backward_launches", b"layout_launches")


def _bits(t):
    return t.detach().contiguous().view(_BITS[t.dtype]).cpu()


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    diff = (_bits(a) != _bits(b))
    assert not bool(diff.any()), "%s: %d of %d elements differ" % (what, int(diff.sum()), diff.numel())


def _layout(y2d, S, T, layout, dtype, pad=5):
    """(S*T, P) float32 values -> a leaf tensor of ``dtype`` in the given layout."""
    y2d = torch.as_tensor(y2d)
    P = y2d.shape[1]
    y = y2d.to(DEV).to(dtype)
    if layout == "3d":
        return y.view(T, S, P).permute(1, 2, 0).contiguous().requires_grad_(True)
    if layout == "2d":
        return y.clone().requires_grad_(True)
    wide = torch.zeros(S * T, P + pad, dtype=dtype, device=DEV)
    wide[:, :P] = y
    return wide[:, :P].detach().requires_grad_(True)  # (row stride P + pad)


def _in_layout(w, S, T, three_d):
    w = w.to(DEV)
    return w.view(T, S).t().unsqueeze(1) if three_d else w.unsqueeze(1)


def _run(x, xe, graph, sup, xent, l2, leaky, w=None, c=None, fn=chain_loss):
    kw = dict(l2_regularize=l2, leaky_hmm_coefficient=leaky)
    if xent is not None:
        kw.update(xent_regularize=0.1, xent_input=xe, kaldi_way=xent)
    if w is not None:
        kw.update(deriv_weights=w)
    if c is not None:
        kw.update(out_of_range_regularize=c)
    loss, res = fn(x, graph, sup, **kw)
    loss.sum().backward()
    return loss.detach(), res.data.clone(), res.xent_objf, x.grad, (xe.grad if xent is not None else None)


def _expected(g32, x, c, w_layout, dtype):
    """w * fl32(g + t) from the unpenalised float32 gradient and the widened output, t in numpy float32; 16-bit: rounded once,
    through torch's own cast."""
    y = x.detach().float().cpu().numpy()
    want = oor.penalized(g32.detach().cpu().numpy(), y, c)
    want = torch.from_numpy(want).to(DEV)
    if w_layout is not None:
        want = want * w_layout
    return want.to(dtype)


def _check(graph, sup, S, T, y2d, xe2d, dtype, layout, xent, c=C, w=None, l2=0.0, leaky=1e-5, succeeded=True):
    """The penalised call against (a) the same call with c = 0: results, loss, xent objective and xent gradient equal bit for
    bit; (b) the unpenalised, unweighted float32 call on the widened values: the gradient is w * fl32(g + t), cast once."""
    mk = lambda: (_layout(y2d, S, T, layout, dtype), _layout(xe2d, S, T, layout, dtype) if xent is not None else None)  # noqa: E731
    x, xe = mk()
    got = _run(x, xe, graph, sup, xent, l2, leaky, w=w, c=c)
    x0, xe0 = mk()
    base = _run(x0, xe0, graph, sup, xent, l2, leaky, w=w, c=0.0)
    if dtype == torch.float32 and w is None:
        g32 = base[3]
    else:
        xf = x.detach().float().requires_grad_(True)
        xef = xe.detach().float().requires_grad_(True) if xe is not None else None
        g32 = _run(xf, xef, graph, sup, xent, l2, leaky)[3]
    _same_bits(got[0], base[0], "loss")
    _same_bits(got[1], base[1], "results.data")
    assert got[2] == base[2]
    if succeeded:
        assert not oor.took_soft_failure(float(got[1][0]), float(got[1][2])), got[1]
    if xent is not None:
        _same_bits(got[4], base[4], "xent grad")
    assert got[3].dtype == dtype and tuple(got[3].shape) == tuple(x.shape)
    wl = _in_layout(w, S, T, layout == "3d") if w is not None else None
    _same_bits(got[3], _expected(g32, x, c, wl, dtype), "grad")
    return got, base


def _weights(S, T, seed):
    pool = np.array([0.0, 1.0 / 255, 128.0 / 255, 1.0, 1.0, 1.0, 1.5, 3.25], np.float32)
    w = np.random.default_rng(seed).choice(pool, size=S * T)
    w[:len(pool)] = pool
    return torch.from_numpy(w.astype(np.float32))


_cache = {}


def _small(spec_name, kind):
    """One of out_of_range_cases' two workloads on the GPU: graph, supervision, outputs of the kind, a tame xent_input."""
    key = (spec_name, kind)
    if key not in _cache:
        spec = getattr(oor, spec_name)
        fst, sup, y, n = oor.workload(spec, kind)
        gkey = (spec_name, "graph")
        if gkey not in _cache:
            _cache[gkey] = io.DenominatorGraph(fst, fst.num_pdfs).prepare(DEV)
        xe = synth.random_nnet_output(spec["S"], spec["T"], fst.num_pdfs, seed=5)  # (nothing out of range: a wrong matrix shows)
        _cache[key] = dict(graph=_cache[gkey], sup=io.Supervision.from_synth(sup), S=spec["S"], T=spec["T"], y=y, xe=xe, n=n,
                           fst=fst, synth_sup=sup)
    return _cache[key]


# ---- layouts x dtypes x cross-entropy branch, sparse and dense inputs -------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("xent", XENT)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gradient_is_the_unpenalised_one_plus_the_term(dtype, layout, xent, kind):
    """The medium graph (4 x 30 x 300); the dense case carries deriv_weights as well (penalised, then weighted)."""
    s = _small("MEDIUM", kind)
    assert s["n"] > 0
    w = _weights(s["S"], s["T"], 1) if kind == "dense" else None
    got, base = _check(s["graph"], s["sup"], s["S"], s["T"], s["y"], s["xe"], dtype, layout, xent, w=w)
    assert not torch.equal(got[3], base[3])


@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_graph_with_odd_sizes(dtype, layout, kind):
    """2 x 6 x 20: T not a multiple of 4, few columns -- the narrow paths of the three passes."""
    s = _small("SMALL", kind)
    for xent in XENT:
        _check(s["graph"], s["sup"], s["S"], s["T"], s["y"], s["xe"], dtype, layout, xent, c=0.25,
               w=_weights(s["S"], s["T"], 2) if xent else None, l2=1e-3)


@pytest.mark.parametrize("T", [5, 6, 8])
def test_unaligned_shapes_take_the_scalar_paths(T):
    """Odd T, odd P and an odd row stride: none of the vector paths' alignment conditions hold."""
    S, P = 3, 21
    fst = synth.random_den_fst(40, 4, P, seed=6)
    graph = io.DenominatorGraph(fst, P).prepare(DEV)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 2, seed=1))
    y, n = oor.overwrite(synth.random_nnet_output(S, T, P, seed=1), "dense")
    xe = synth.random_nnet_output(S, T, P, seed=2)
    assert n > 0
    for dtype in DTYPES:
        for layout in LAYOUTS:
            _check(graph, sup, S, T, y, xe, dtype, layout, False, w=_weights(S, T, 3))
            _check(graph, sup, S, T, y, xe, dtype, layout, None)


@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("T", sorted(oor.TILED))
def test_second_tile_of_the_copy_back(T, kind):
    """2 x 72 x T with T just past 240: a second tile of the (B, C, T) copy back along the frames and along the channels.
    In the second frame tile the frames' factors in LDS are indexed by the tile-local frame and loaded from the rows of
    frame 240 on; the leftover is one frame (element-wise stores), two (4-byte) or four (8-byte, 16-bit tensors)."""
    spec = oor.TILED[T]
    fst, sup, y, n = oor.workload(spec, kind)
    assert n > 0 and spec["S"] == 2 and fst.num_pdfs == 72
    graph = io.DenominatorGraph(fst, fst.num_pdfs).prepare(DEV)
    hsup = io.Supervision.from_synth(sup)
    xe = synth.random_nnet_output(2, T, fst.num_pdfs, seed=2)
    for dtype in DTYPES:
        for xent in (None, False):
            _check(graph, hsup, 2, T, y, xe, dtype, "3d", xent, c=0.25, w=_weights(2, T, 4))


# ---- kernel families, numerator modes, e2e supervisions, C3 -----------------------------------------------------------
@pytest.mark.parametrize("family", [None, "force_general", "force_streamed", "force_pair", "force_mitm", "no_num_overlap"])
def test_kernel_families(kernel_family, family):
    if family is not None:
        kernel_family(family)
    S, T = 16, 60
    cfg = synth.CONFIGS["C2"]
    fst = synth.config_den_fst("C2")
    graph = io.DenominatorGraph(fst, cfg["P"]).prepare(DEV)  # (built anew: the switches are read when a graph is built)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=11))
    y, n = oor.overwrite(synth.random_nnet_output(S, T, cfg["P"], seed=12), "sparse")
    xe = synth.random_nnet_output(S, T, cfg["P"], seed=13)
    assert n > 0
    for layout, dtype, xent, w in (("2d", torch.float32, None, None), ("2d_strided", torch.float32, True, _weights(S, T, 4)),
                                   ("3d", torch.float32, False, None), ("3d", torch.bfloat16, True, _weights(S, T, 4)),
                                   ("2d", torch.float16, False, None)):
        _check(graph, sup, S, T, y, xe, dtype, layout, xent, w=w, l2=cfg["l2"], leaky=cfg["leaky"])


@pytest.mark.parametrize("layout", ["3d", "2d"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_e2e_supervision(dtype, layout):
    S, T, P = 16, 40, 60
    graph = io.DenominatorGraph(synth.random_den_fst(80, 4, P, seed=31), P).prepare(DEV)
    sup = io.Supervision.from_e2e_fsts(0.9, T, P, ref.batch("chain", S, P, seed=11))
    rng = np.random.default_rng(12)
    y, n = oor.overwrite((rng.normal(size=(S * T, P)) * 2.0).astype(np.float32), "sparse")
    xe = rng.normal(size=(S * T, P)).astype(np.float32)
    assert n > 0
    for xent in XENT:
        _check(graph, sup, S, T, y, xe, dtype, layout, xent, w=_weights(S, T, 5) if xent is None else None, l2=1e-4)


def test_c3_step():
    S, T = 256, 150
    cfg = synth.CONFIGS["C3"]
    fst = synth.config_den_fst("C3")
    graph = io.DenominatorGraph(fst, cfg["P"]).prepare(DEV)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=5))
    y, n = oor.overwrite(synth.random_nnet_output(S, T, cfg["P"], seed=6), "sparse")
    assert n > 0.005 * y.size
    _check(graph, sup, S, T, y, None, torch.float32, "3d", None, l2=cfg["l2"], leaky=cfg["leaky"])
    _check(graph, sup, S, T, y, None, torch.bfloat16, "3d", None, w=_weights(S, T, 6), l2=cfg["l2"], leaky=cfg["leaky"])
    _check(graph, sup, S, T, y, None, torch.float32, "2d", None, l2=cfg["l2"], leaky=cfg["leaky"])


# ---- the pairs that are normalised in front of the one call -------------------------------------------------------------
def _close(a, b, what):
    assert abs(float(a) - float(b)) <= 1e-6 * abs(float(b)), (what, float(a), float(b))


def test_fallback_routes_agree_bit_for_bit():
    """2-D tensors of different row strides and a (B, C, T) view whose channel stride is not 1 are made contiguous and take
    the one call: the same g' as the one call gives on the same values -- all five outputs bit for bit those of chain_loss
    on the contiguous copies.  They went through to2d() and _ChainLoss, and through _ChainLoss3d: results and both
    gradients are bit for bit those of these composed classes (tests/composed_step.py), loss and xent_objf within the 1e-6
    relative the two routes are documented to differ by."""
    from composed_step import chain_loss_composed
    s = _small("MEDIUM", "sparse")
    S, T, g, sup = s["S"], s["T"], s["graph"], s["sup"]
    kw = dict(l2_regularize=1e-3, leaky_hmm_coefficient=1e-5, xent_regularize=0.1, kaldi_way=True)
    w = _weights(S, T, 7)
    y_dev = torch.from_numpy(s["y"]).to(DEV)
    for c in (C, 0.25):
        # (a) 2-D input and xent_input of different row strides -> to2d() and _ChainLoss
        outs = {}
        for key, (ww, cc) in dict(plain=(None, 0.0), on=(None, c), both=(w, c)).items():
            a, b = _layout(s["y"], S, T, "2d", torch.float32), _layout(s["xe"], S, T, "2d_strided", torch.float32)
            outs[key] = _run(a, b, g, sup, True, 1e-3, 1e-5, w=ww, c=cc)
            a2, b2 = _layout(s["y"], S, T, "2d", torch.float32), _layout(s["xe"], S, T, "2d", torch.float32)
            copies = _run(a2, b2, g, sup, True, 1e-3, 1e-5, w=ww, c=cc)  # (what the planner makes of the pair)
            for i in (0, 1, 3, 4):
                _same_bits(outs[key][i], copies[i], key + ", contiguous copies, output %d" % i)
            assert outs[key][2] == copies[2], key
            a3, b3 = _layout(s["y"], S, T, "2d", torch.float32), _layout(s["xe"], S, T, "2d_strided", torch.float32)
            comp = _run(a3, b3, g, sup, True, 1e-3, 1e-5, w=ww, c=cc, fn=chain_loss_composed)
            for i in (1, 3, 4):
                _same_bits(outs[key][i], comp[i], key + ", composed, output %d" % i)
            _close(outs[key][0], comp[0], key + ": loss, composed")
            _close(outs[key][2], comp[2], key + ": xent_objf, composed")
        want = torch.from_numpy(oor.penalized(outs["plain"][3].cpu().numpy(), s["y"], c)).to(DEV)
        _same_bits(outs["on"][3], want, "grad, mixed strides")
        _same_bits(outs["both"][3], want * w.to(DEV).unsqueeze(1), "weighted grad, mixed strides")
        _same_bits(outs["on"][4], outs["plain"][4], "xent grad, mixed strides")
        _same_bits(outs["on"][1], outs["plain"][1], "results")
        # (b) a (B, C, T) view that is not contiguous -> _ChainLoss3d
        grads = {}
        for key, (ww, cc) in dict(plain=(None, 0.0), on=(None, c), both=(w, c)).items():
            leaf = y_dev.view(T, S, -1).permute(1, 0, 2).contiguous().requires_grad_(True)  # (B, T, C)
            loss, res = chain_loss(leaf.permute(0, 2, 1), g, sup, 1e-3, 1e-5, deriv_weights=ww, out_of_range_regularize=cc)
            loss.backward()
            grads[key] = leaf.grad.permute(1, 0, 2).reshape(S * T, -1)  # (frame-major rows again)
            leaf2 = leaf.detach().clone().requires_grad_(True)
            loss2, res2 = chain_loss_composed(leaf2.permute(0, 2, 1), g, sup, 1e-3, 1e-5, deriv_weights=ww,
                                              out_of_range_regularize=cc)
            loss2.backward()
            _same_bits(leaf.grad, leaf2.grad, key + ": grad, composed")
            _same_bits(res.data, res2.data, key + ": results, composed")
            _close(loss.detach(), loss2.detach(), key + ": loss, composed")
        want = torch.from_numpy(oor.penalized(grads["plain"].cpu().numpy(), s["y"], c)).to(DEV)
        _same_bits(grads["on"], want, "grad, non-contiguous (B, C, T)")
        _same_bits(grads["both"], want * w.to(DEV).unsqueeze(1), "weighted grad, non-contiguous (B, C, T)")
        # (c) the low-level call
        y = y_dev
        d0, d1 = torch.empty_like(y), torch.empty_like(y)
        compute_chain_objf_and_deriv(g, sup, y, ChainResults().data, d0, None, 1e-3, 1e-5, 0.0)
        compute_chain_objf_and_deriv(g, sup, y, ChainResults().data, d1, None, 1e-3, 1e-5, 0.0, out_of_range_regularize=c)
        _same_bits(-d1, torch.from_numpy(oor.penalized((-d0).cpu().numpy(), s["y"], c)).to(DEV), "low-level deriv")


# ---- against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("layout", ["2d", "3d"])
@pytest.mark.parametrize("spec", ["SMALL", "MEDIUM"])
def test_oracle_plus_the_numpy_term(oracle, spec, layout, kind):
    """-g' against the oracle's derivative minus t, matrix-wise: 1e-4 * max(max |oracle|, weight)."""
    s = _small(spec, kind)
    S, T, P = s["S"], s["T"], s["fst"].num_pdfs
    want = oracle.compute_chain_objf_and_deriv(oracle.DenGraph(s["fst"]), s["synth_sup"], s["y"], 0.0, 1e-5)
    assert not oor.took_soft_failure(want["objf"], want["weight"])
    x = to3d(s["y"], S, T, P).requires_grad_(True) if layout == "3d" else torch.from_numpy(s["y"]).to(DEV).requires_grad_(True)
    loss, res = chain_loss(x, s["graph"], s["sup"], 0.0, 1e-5, out_of_range_regularize=C)
    loss.backward()
    got = res.data.numpy()
    assert abs(got[0] - want["objf"]) <= REL * abs(want["objf"]) and got[2] == want["weight"]
    grad = from3d(x.grad, S, T, P) if layout == "3d" else x.grad.cpu().numpy()
    target = want["deriv"].astype(np.float64) - oor.term(s["y"], C).astype(np.float64)
    err = rel_err(-grad, target, floor=float(want["weight"]) / (S * T))
    print("%s %s %s: rel err %.3e, max |oracle + term| %.3e" % (spec, layout, kind, err, np.abs(target).max()))
    assert err <= REL


# ---- no effect where it should have none --------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_is_the_call_without_the_keyword(dtype, layout):
    s = _small("MEDIUM", "sparse")
    outs, launches = [], []
    for c in (None, 0.0, None):
        x, xe = _layout(s["y"], s["S"], s["T"], layout, dtype), _layout(s["xe"], s["S"], s["T"], layout, dtype)
        before = [lib.tc_debug_counter(k) for k in _COUNTERS]
        outs.append(_run(x, xe, s["graph"], s["sup"], True, 1e-3, 1e-5, w=_weights(s["S"], s["T"], 8), c=c))
        launches.append([lib.tc_debug_counter(k) - b for k, b in zip(_COUNTERS, before)])
    for i, what in ((0, "loss"), (1, "results"), (3, "grad"), (4, "xent grad")):
        _same_bits(outs[0][i], outs[1][i], what)
    assert outs[0][2] == outs[1][2]
    assert launches[0] == launches[1] == launches[2] and launches[0][0] == 1


@pytest.mark.parametrize("kind", ["none", "edge"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_out_of_range_changes_nothing(dtype, layout, kind):
    """N(0, 1) outputs, and outputs with elements at exactly +-30 (p = 0): every gradient bit is the c = 0 call's."""
    s = _small("MEDIUM", kind)
    assert s["n"] == 0
    for xent in (None, False):
        got, base = _check(s["graph"], s["sup"], s["S"], s["T"], s["y"], s["xe"], dtype, layout, xent, c=0.5,
                           w=_weights(s["S"], s["T"], 9) if xent is None else None)
        _same_bits(got[3], base[3], "grad")


@pytest.mark.parametrize("layout", ["3d", "2d"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_no_grad_accepts_the_option_and_does_nothing(dtype, layout):
    s = _small("MEDIUM", "dense")
    kw = dict(l2_regularize=1e-3, leaky_hmm_coefficient=1e-5, xent_regularize=0.1, kaldi_way=True)
    x, xe = _layout(s["y"], s["S"], s["T"], layout, dtype), _layout(s["xe"], s["S"], s["T"], layout, dtype)
    with torch.no_grad():
        loss0, res0 = chain_loss(x, s["graph"], s["sup"], xent_input=xe, **kw)
        loss1, res1 = chain_loss(x, s["graph"], s["sup"], xent_input=xe, out_of_range_regularize=C, **kw)
        with pytest.raises(ValueError):
            chain_loss(x, s["graph"], s["sup"], xent_input=xe, out_of_range_regularize=-1.0, **kw)
    _same_bits(loss0, loss1, "loss")
    _same_bits(res0.data, res1.data, "results")
    assert res0.xent_objf == res1.xent_objf
    assert x.grad is None and xe.grad is None and not loss1.requires_grad


# ---- soft failure -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kaldi_way", [True, False])
def test_soft_failure_gradient_is_penalised_then_weighted(dtype, layout, kaldi_way):
    """A numerical failure with l2 != 0 (an inf in the matrix the objective runs on, as tests/test_gpu_deriv_weights.py builds
    it): the gradient is w * (l2 * weight * y + t), the xent gradient 0; NaN and +-inf outputs get p = 0."""
    s = _small("MEDIUM", "sparse")
    S, T = s["S"], s["T"]
    y, xe = s["y"].copy(), s["xe"].copy()
    (y if kaldi_way else xe)[17, 5] = np.inf
    y[3, 7], y[4, 9], y[5, 11] = -np.inf, np.nan, np.inf  # (chain outputs that are not finite: no term there)
    w = _weights(S, T, 10)
    w[[3, 4, 5, 17]] = 0.5  # (no 0 * inf)
    l2 = 1e-3
    got, base = _check(s["graph"], s["sup"], S, T, y, xe, dtype, layout, kaldi_way, w=w, l2=l2, succeeded=False)
    assert float(got[1][0]) == -10.0 * S * T and float(got[1][2]) == S * T
    assert torch.count_nonzero(got[4]) == 0 and got[2] == 0.0
    # (base is the reset's own gradient, w * l2 * weight * y of the matrix the objective ran on: tests/test_gpu_deriv_weights.py)
    x = _layout(y, S, T, layout, dtype).detach().float()
    out = ((x.abs() > 30) & torch.isfinite(x)).cpu()
    weighted = (_in_layout(w, S, T, layout == "3d") != 0).expand_as(x).cpu()  # (a row of weight 0 is 0 either way)
    changed = _bits(got[3]) != _bits(base[3])
    assert bool((out & weighted).any()) and bool(changed[out & weighted].all())  # the term reaches every out-of-range element
    assert not bool(changed[~out].any())                                          # ... and no other


# ---- it restores range --------------------------------------------------------------------------------------------------
def test_sgd_on_the_outputs_comes_back_into_range():
    """SGD on the raw outputs, l2 = 0.  Some elements start at -45 and some at +45, at pdfs no numerator arc uses (so the
    numerator cannot push them outwards).  lr * 2c = 0.2 < 1: the penalty cannot overshoot."""
    s = _small("MEDIUM", "none")
    S, T, P = s["S"], s["T"], s["fst"].num_pdfs
    unused = np.setdiff1d(np.arange(P), np.unique(s["synth_sup"].ilabel) - 1)
    assert len(unused) >= 8
    rng = np.random.default_rng(21)
    rows = rng.choice(S * T, size=12, replace=False)
    cols = rng.choice(unused, size=12)
    start = s["y"].copy()
    start[rows[:6], cols[:6]] = -45.0
    start[rows[6:], cols[6:]] = 45.0
    lo = (torch.from_numpy(rows[:6]).to(DEV), torch.from_numpy(cols[:6]).to(DEV))
    both = (torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV))
    lr, c, steps = 2.0, 0.05, 6
    traj = {}
    for key, cc in (("on", c), ("off", 0.0)):
        y = torch.from_numpy(start).to(DEV)
        seen = [y[both].abs().clone()]
        for _ in range(steps):
            x = y.clone().requires_grad_(True)
            loss, res = chain_loss(x, s["graph"], s["sup"], 0.0, 1e-5, out_of_range_regularize=cc)
            loss.backward()
            assert not oor.took_soft_failure(float(res.data[0]), float(res.data[2]))
            y = y - lr * x.grad
            seen.append(y[both].abs().clone())
        traj[key] = (torch.stack(seen), y)
    on, off = traj["on"][0], traj["off"][0]
    for k in range(steps):  # |y| falls at every step while it is above 30
        above = on[k] > 30.0
        assert bool((on[k + 1][above] < on[k][above]).all()), k
    assert bool((on[-1] < off[-1]).all())  # ... and ends smaller than without the penalty, element by element
    first_step = (on[0] - on[1])[:6]
    drift_off = (off[0] - off[-1]).abs()[:6]
    assert bool((drift_off < first_step).all()), (drift_off, first_step)
    assert bool((traj["off"][1][lo] < -30.0).all())  # (without it the -45 elements are still out of range)


# ---- operator, capture, data parallel, recipe ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["3d", "2d"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_registered_operator(dtype, layout):
    from torchain_amd.ops import chain_loss_op
    s = _small("MEDIUM", "sparse")
    outs = []
    for fn in (chain_loss, chain_loss_op):
        a, b = _layout(s["y"], s["S"], s["T"], layout, dtype), _layout(s["xe"], s["S"], s["T"], layout, dtype)
        outs.append(_run(a, b, s["graph"], s["sup"], True, 1e-3, 1e-5, w=_weights(s["S"], s["T"], 11), c=C, fn=fn))
    for i, what in ((0, "loss"), (1, "results"), (3, "grad"), (4, "xent grad")):
        _same_bits(outs[0][i], outs[1][i], what)
    assert outs[0][2] == outs[1][2]
    with pytest.raises(ValueError):
        chain_loss_op(a, s["graph"], s["sup"], out_of_range_regularize=float("nan"))


def test_registered_operator_traces_as_one_node():
    from torchain_amd import ops  # noqa: F401
    s = _small("MEDIUM", "sparse")
    x = torch.from_numpy(s["y"]).to(DEV)
    gp, sp = int(s["graph"].ptr.value), int(s["sup"].ptr.value)

    def step(a):
        out, _grad, _xgrad = torch.ops.torchain_amd.chain_step_penalized(a, a.new_empty((0,)), gp, sp, 0.0, 1e-5, 0.0, True, True,
                                                                         None, C)
        return out[3]

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    a = x.clone().requires_grad_(True)
    loss = torch.compile(step, backend=backend, fullgraph=True)(a)
    loss.backward()
    calls = [n for g in graphs for n in g.graph.nodes if n.op == "call_function" and "chain_step_penalized" in str(n.target)]
    assert len(graphs) == 1 and len(calls) == 1
    b = x.clone().requires_grad_(True)
    ref_loss, _ = chain_loss(b, s["graph"], s["sup"], 0.0, 1e-5, out_of_range_regularize=C)
    ref_loss.backward()
    _same_bits(a.grad, b.grad, "grad")
    torch.library.opcheck(torch.ops.torchain_amd.chain_step_penalized.default,
                          (x.clone().requires_grad_(True), x.new_empty((0,)), gp, sp, 0.0, 1e-5, 0.0, True, True, None, C),
                          test_utils=("test_schema", "test_faketensor"))


@pytest.mark.parametrize("layout", ["3d", "2d"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_step_replays_on_new_outputs(dtype, layout):
    s = _small("MEDIUM", "sparse")
    S, T = s["S"], s["T"]
    kw = dict(l2_regularize=1e-3, leaky_hmm_coefficient=1e-5, xent_regularize=0.1, kaldi_way=True, out_of_range_regularize=C)
    x = _layout(s["y"], S, T, layout, dtype)
    xe = _layout(s["xe"], S, T, layout, dtype)

    def step():
        loss, results = chain_loss(x, s["graph"], s["sup"], xent_input=xe, **kw)
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
    for kind in ("dense", "none", "sparse"):
        with torch.no_grad():
            x.copy_(_layout(_small("MEDIUM", kind)["y"], S, T, layout, dtype))
        cg.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        want = step()
        for g, w_, what in zip(got, want, ("loss", "grad", "xent grad")):
            _same_bits(g, w_, what + " after replay on " + kind)
    torch.cuda.synchronize()


def _dp_worker(rank, world, port, S, T, P, out_dir):
    """One rank: its shard of the sequences through parallel.chain_loss_data_parallel on cuda:0 (both ranks share the GPU of the
    test box; the collective travels over gloo), as tests/test_gpu_parallel.py."""
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        d = np.load(os.path.join(out_dir, "inputs.npz"))
        fst = synth.random_den_fst(120, 5, P, seed=71)
        sup = synth.SupFst(float(d["w"]), S, T, P, int(d["nst"]), d["arc_begin"], d["ilabel"], d["arc_weight"], d["nextstate"], d["final"])
        lo, hi = parallel.shard_range(S, rank, world)
        y_local = np.ascontiguousarray(parallel.shard_rows(torch.from_numpy(d["y"]), S, lo, hi).numpy())
        den, hsup = io.DenominatorGraph(fst, P), io.Supervision.from_synth(parallel.shard_supervision_fst(sup, lo, hi))
        B = hi - lo
        x = to3d(y_local, B, T, P).requires_grad_(True)
        loss, res = parallel.chain_loss_data_parallel(x, den, hsup, 1e-3, 0.1, out_of_range_regularize=float(d["c"]))
        loss.backward()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), res=res.data.numpy(), loss=float(loss), grad=from3d(x.grad, B, T, P))
    finally:
        dist.destroy_process_group()


def test_data_parallel_two_ranks(tmp_path):
    import torch.multiprocessing as mp

    world, S, T, P = 2, 5, 12, 64  # uneven shards: 3 + 2 sequences
    fst = synth.random_den_fst(120, 5, P, seed=71)
    sup = synth.random_supervision(fst, S, T, 1, seed=72, weight=0.5)  # 1 path: single boundary states
    y, n = oor.overwrite(synth.random_nnet_output(S, T, P, seed=73), "sparse")
    assert n > 0
    np.savez(str(tmp_path / "inputs.npz"), y=y, c=C, w=sup.weight, nst=sup.num_states, arc_begin=sup.arc_begin,
             ilabel=sup.ilabel, arc_weight=sup.arc_weight, nextstate=sup.nextstate, final=sup.final)
    mp.spawn(_dp_worker, args=(world, free_port(), S, T, P, str(tmp_path)), nprocs=world, join=True)
    den, hsup = io.DenominatorGraph(fst, P), io.Supervision.from_synth(sup)
    single = {}
    for key, c in (("on", C), ("off", 0.0)):
        x = to3d(y, S, T, P).requires_grad_(True)
        loss, res = chain_loss(x, den, hsup, 1e-3, 0.1, out_of_range_regularize=c)
        loss.backward()
        single[key] = (res.data.numpy().copy(), from3d(x.grad, S, T, P))
    assert not oor.took_soft_failure(single["on"][0][0], single["on"][0][2])
    r = [np.load(str(tmp_path / ("rank%d.npz" % k))) for k in range(world)]
    np.testing.assert_array_equal(r[0]["res"], r[1]["res"])
    want = single["on"][0]
    assert abs(r[0]["res"][0] - want[0]) <= REL * abs(want[0]) and r[0]["res"][2] == want[2]
    out = np.abs(y) > 30
    for k in range(world):
        lo, hi = parallel.shard_range(S, k, world)
        g = parallel.shard_rows(torch.from_numpy(single["on"][1]), S, lo, hi).numpy()
        g_off = parallel.shard_rows(torch.from_numpy(single["off"][1]), S, lo, hi).numpy()
        m = parallel.shard_rows(torch.from_numpy(out), S, lo, hi).numpy()
        assert rel_err(r[k]["grad"], g, floor=0.5) <= REL
        # the term itself is per element: a rank's penalised elements differ from the unpenalised single call's by exactly t
        assert rel_err((r[k]["grad"] - g_off)[m], (g - g_off)[m], floor=1e-3) <= REL and m.any()


def test_recipe_loop_with_the_option_on(tmp_path):
    """io.RandExample -> the recipe's network (plus a fixed offset that drives a few outputs past +-30) -> chain_loss with the
    penalty: parameter gradients equal those of the unpenalised loss with the term added by a hook on the outputs, the loss
    stays finite and falls."""
    import copy

    import kaldi_egs_writer as kw_
    import recipe_fixture as rf
    P, L = 32, 20
    fst = synth.random_den_fst(120, 4, P, seed=3)
    emb = np.random.default_rng(1234).standard_normal((P, rf.FEAT)).astype(np.float32)
    keyed = [("oor%03d-%d" % (i, L), rf.learnable_example(fst, L, seed=300 + i, emb=emb)) for i in range(32)]
    ark, scp = str(tmp_path / "oor.ark"), str(tmp_path / "oor.scp")
    kw_.write_ark(ark, keyed, scp_path=scp)
    with open(scp + ".len", "w") as f:
        f.write("".join("%s %d\n" % (k, L) for k, _ in keyed))
    graph = io.DenominatorGraph(fst, P).prepare(DEV)
    egs = io.RandExample(scp, seed=1, batchsize=8)
    torch.manual_seed(0)
    model = rf.TwoLayerTdnn(P).to(DEV)
    hooked = copy.deepcopy(model)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
    kw = dict(l2_regularize=5e-5, leaky_hmm_coefficient=0.1, xent_regularize=0.1, kaldi_way=True)
    losses, compared, active = [], 0, 0
    for epoch in range(6):
        egs.reset()
        for (feats, ivec), sup in egs:
            feats, ivec = feats.to(DEV), ivec.to(DEV)
            mmi, xe = model(feats, ivec)
            offset = torch.zeros_like(mmi[0])
            offset[3, 1::7], offset[11, 2::5] = 40.0, -40.0
            mmi = mmi + offset
            loss, res = chain_loss(mmi, graph, sup, xent_input=xe, out_of_range_regularize=C, **kw)
            loss.backward()
            active += int((mmi.detach().abs() > 30).sum())
            if epoch == 0:
                hooked.load_state_dict(model.state_dict())
                hooked.zero_grad(set_to_none=True)
                hm, hx = hooked(feats, ivec)
                hm = hm + offset
                t = torch.from_numpy(oor.term(hm.detach().cpu().numpy(), C)).to(DEV)
                hm.register_hook(lambda g, t=t: g + t)
                hloss, _ = chain_loss(hm, graph, sup, xent_input=hx, **kw)
                hloss.backward()
                for (name, p), q in zip(model.named_parameters(), hooked.parameters()):
                    np.testing.assert_allclose(p.grad.cpu().numpy(), q.grad.cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg=name)
                compared += 1
            opt.step()
            opt.zero_grad(set_to_none=False)
            losses.append(float(res.loss))
    assert compared >= 2 and active > 0
    assert np.isfinite(losses).all()
    assert np.mean(losses[-4:]) < np.mean(losses[:4]), losses
