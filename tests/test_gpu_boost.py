"""Boosted LF-MMI on the GPU (``chain_loss(..., boost=b, boost_ref= / boost_accuracy=)``, ``tc_chain_step_boosted``,
``tc_boost_rows``): the denominator runs on ``y_b = fl32(y32 - fl32(b32 * a))`` and nothing else does.

The pass alone is held bit for bit to torch's ``y.float() - b32 * a`` in every layout and dtype; the step to the float64 and
the float32-oracle compositions of ``boost_reference`` under the project's ``REL`` (matrix-wise, no entry left out; one case
element-wise), on a graph of the tied kernels and on one forced onto the general kernel, with regular, ragged and end-to-end
handles.  Also: which part of the step saw the boost, no effect where there should be none, layouts and dtypes, the shift by
a constant accuracy, failures, refusals, no host synchronisation, stream capture, and that the margin does what it is for.
Shapes are small: every element is compared."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import independent_f64 as ind
from torchain_amd import io, synth
from torchain_amd._lib import TC_DTYPE_BF16, TC_DTYPE_F16, TC_DTYPE_F32, TC_LAYOUT_BCT, TC_LAYOUT_CHANNEL_LAST, TC_LAYOUT_ROWS, check, lib
from torchain_amd.functions import chain_loss

import boost_reference as br
import e2e_reference as e2e
from helpers import REL, elementwise, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 24
LEAKY = 0.05
WEIGHT = 0.8
BOOST = 1.25
_DT = {torch.float32: TC_DTYPE_F32, torch.bfloat16: TC_DTYPE_BF16, torch.float16: TC_DTYPE_F16}
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def _bits(t):
    return t.detach().contiguous().view(_BITS[t.dtype]).cpu()


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    diff = _bits(a) != _bits(b)
    assert not bool(diff.any()), "%s: %d of %d elements differ" % (what, int(diff.sum()), diff.numel())


def _counter(name):
    return lib.tc_debug_counter(name.encode())


# ---- the pass alone ------------------------------------------------------------------------------------------------------
def _boost_rows(x, layout, S, Cn, T, b, ref=None, cls=None, acc=None, frames=None, out_pad=0):
    """tc_boost_rows on device tensors where they lie; returns the (T*S, Cn) float32 result."""
    wide = torch.full((S * T, Cn + out_pad), 7.0, device=DEV)
    out = wide[:, :Cn]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    row_stride = sb = st = 0
    if layout == TC_LAYOUT_ROWS:
        row_stride = x.stride(0)
    elif layout == TC_LAYOUT_CHANNEL_LAST:
        sb, st = x.stride(0), x.stride(2)
    check(lib.tc_boost_rows(p(x), _DT[x.dtype], layout, S, Cn, T, row_stride, sb, st, p(frames), float(b), p(ref), p(cls), p(acc),
                            acc.stride(0) if acc is not None else 0, p(out), out.stride(0), 0,
                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tc_boost_rows")
    torch.cuda.synchronize()
    if out_pad:
        assert bool((wide[:, Cn:] == 7.0).all())
    return out


def _views(y2d, S, T, dtype):
    """The (T*S, Cn) values in every layout the step takes: name -> (tensor, TC_LAYOUT_*)."""
    Cn = y2d.shape[1]
    y = y2d.to(DEV).to(dtype)
    lane = 4 if dtype == torch.float32 else 8
    strided = torch.zeros(S * T, Cn + lane + 1, dtype=dtype, device=DEV)
    strided[:, :Cn] = y
    padded = torch.zeros(S * T, (Cn + 7) // 8 * 8 + 8, dtype=dtype, device=DEV)  # (16-byte rows, whatever Cn: lanes and a tail)
    padded[:, :Cn] = y
    off = torch.zeros(S * T * Cn + 1, dtype=dtype, device=DEV)  # (a base that is not 16-byte aligned)
    off[1:] = y.reshape(-1)
    bct = y.view(T, S, Cn).permute(1, 2, 0).contiguous()
    batch_first = y.view(T, S, Cn).permute(1, 0, 2).contiguous()  # (B, T, C)
    return {
        "rows": (y.contiguous(), TC_LAYOUT_ROWS),
        "rows_strided": (strided[:, :Cn], TC_LAYOUT_ROWS),
        "rows_padded": (padded[:, :Cn], TC_LAYOUT_ROWS),
        "rows_unaligned": (off[1:].view(S * T, Cn), TC_LAYOUT_ROWS),
        "bct": (bct, TC_LAYOUT_BCT),
        "batch_first": (batch_first.transpose(1, 2), TC_LAYOUT_CHANNEL_LAST),
    }


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("Cn", [24, 13, 64 + 19])
def test_boost_rows_is_torchs_two_roundings_in_every_layout(dtype, Cn):
    S, T, b = 5, 7, -0.7
    rng = np.random.default_rng(Cn)
    y2d = torch.from_numpy((3.0 * rng.normal(size=(S * T, Cn))).astype(np.float32))
    y2d[0, 0] = -0.0
    ref_np = rng.integers(-1, Cn + 1, size=(S, T))  # (-1 and Cn: frames that score nothing)
    cls_np = rng.integers(0, 4, size=Cn)
    ref = torch.from_numpy(ref_np.astype(np.int32)).to(DEV)
    cls = torch.from_numpy(cls_np.astype(np.int32)).to(DEV)
    dense_wide = torch.zeros(S * T, (Cn + 3) // 4 * 4 + 4, device=DEV)  # (a row stride that keeps the rows 16-byte aligned)
    dense = dense_wide[:, :Cn]
    dense.copy_(torch.from_numpy(rng.normal(size=(S * T, Cn)).astype(np.float32)))
    b32 = torch.tensor(b, dtype=torch.float32, device=DEV)
    forms = {
        "hard": (dict(ref=ref), torch.from_numpy(br.indicator(ref_np, None, Cn)).to(DEV)),
        "classes": (dict(ref=ref, cls=cls), torch.from_numpy(br.indicator(ref_np, cls_np, Cn)).to(DEV)),
        "dense_strided": (dict(acc=dense), dense),
    }
    for name, (x, layout) in _views(y2d, S, T, dtype).items():
        y32 = y2d.to(DEV).to(dtype).float()
        for form, (kw, a) in forms.items():
            want = y32 - b32 * a
            got = _boost_rows(x, layout, S, Cn, T, b, out_pad=3 if form == "hard" else 0, **kw)
            _same(got, want, "%s %s" % (name, form))
            if form != "dense_strided":  # the hard form IS the dense form on the float32 indicator
                _same(_boost_rows(x, layout, S, Cn, T, b, acc=a.contiguous()), got, "%s %s as indicator" % (name, form))
            assert np.array_equal(got.cpu().numpy(), br.boosted(y32.cpu().numpy(), b, a.cpu().numpy()))


def test_boost_rows_reads_no_padding_of_a_ragged_batch():
    S, T, Cn, b = 4, 9, 13, 2.0
    frames_np = np.array([9, 5, 1, 8], np.int32)
    rng = np.random.default_rng(3)
    y2d = torch.from_numpy(rng.normal(size=(S * T, Cn)).astype(np.float32))
    live = torch.from_numpy((np.arange(T)[:, None] < frames_np[None, :]).reshape(-1)).to(DEV)  # row t*S + s
    ref_np = rng.integers(0, Cn, size=(S, T))
    a_hard = torch.from_numpy(br.indicator(ref_np, None, Cn)).to(DEV)
    ref_np = np.where(np.arange(T)[None, :] < frames_np[:, None], ref_np, 3)  # (garbage that WOULD score in the padding)
    dense = torch.from_numpy(rng.normal(size=(S * T, Cn)).astype(np.float32)).to(DEV)
    dense_nan = torch.where(live[:, None], dense, torch.full_like(dense, float("nan")))
    frames = torch.from_numpy(frames_np).to(DEV)
    ref = torch.from_numpy(ref_np.astype(np.int32)).to(DEV)
    for name, (x, layout) in _views(y2d, S, T, torch.float32).items():
        y32 = y2d.to(DEV)
        for kw, a in ((dict(ref=ref), a_hard), (dict(acc=dense_nan), dense)):
            want = torch.where(live[:, None], y32 - torch.tensor(b, device=DEV) * a, y32)
            _same(_boost_rows(x, layout, S, Cn, T, b, frames=frames, **kw), want, name)


# ---- workloads: graph family x handle --------------------------------------------------------------------------------------------------
_cache = {}


def _graph(family, kernel_family):
    if family not in _cache:
        if family == "general":
            kernel_family("force_general")  # (read when the graph is built)
        fst = synth.random_den_fst(60, 3, P, seed=21)
        graph = io.DenominatorGraph(fst, P).prepare(DEV)
        assert graph.stats()["tied"] == (1 if family == "tied" else 0), graph.stats()
        _cache[family] = (fst, graph)
    return _cache[family]


def _handle(kind, oracle):
    """(S, Tmax, frames, handle, host supervisions) of a regular uniform, a regular ragged or an end-to-end minibatch."""
    key = ("handle", kind)
    if key not in _cache:
        fst = synth.random_den_fst(60, 3, P, seed=21)
        pi = oracle.DenGraph(fst).initial_probs()
        if kind == "uniform":
            S, T = 4, 9
            host = synth.random_supervision(fst, S, T, 2, seed=5, weight=WEIGHT, initial_probs=pi)
            _cache[key] = (S, T, [T] * S, io.Supervision.from_synth(host), host)
        elif kind == "ragged":
            frames = [9, 6, 4, 8]
            host = [synth.random_supervision(fst, 1, n, 2, seed=40 + s, weight=WEIGHT, initial_probs=pi) for s, n in enumerate(frames)]
            _cache[key] = (len(frames), max(frames), frames, io.Supervision.from_sequences(host), host)
        else:
            S, T = 3, 20
            host = e2e.batch("chain", S, P, seed=11)
            _cache[key] = (S, T, [T] * S, io.Supervision.from_e2e_fsts(WEIGHT, T, P, host), host)
    return _cache[key]


def _inputs(S, T, frames, form, seed=7, out_of_range=False):
    """y, xent_input (T*S, P) and the accuracy in the given form: (kwargs for chain_loss on DEV, the float32 matrix a)."""
    rng = np.random.default_rng(seed)
    y = synth.random_nnet_output(S, T, P, seed=seed)
    if out_of_range:
        y[::5, 3] = 31.5
        y[2::7, 11] = -33.0
    xe = synth.random_nnet_output(S, T, P, seed=seed + 1)
    live = (np.arange(T)[:, None] < np.asarray(frames)[None, :]).reshape(-1)  # row t*S + s
    ref = rng.integers(-1, P, size=(S, T))
    cls = rng.integers(0, 5, size=P)
    if form == "dense":
        a = rng.random(size=(S * T, P)).astype(np.float32)
        dev = torch.from_numpy(np.where(live[:, None], a, np.float32("nan"))).to(DEV)  # (NaN in the padding rows: unread)
        kw = dict(boost_accuracy=dev)
    else:
        a = br.indicator(ref, cls if form == "classes" else None, P)
        garbage = np.where(np.arange(T)[None, :] < np.asarray(frames)[:, None], ref, 2)
        kw = dict(boost_ref=torch.from_numpy(garbage).to(DEV))  # (int64, as numpy draws them)
        if form == "classes":
            kw["boost_pdf_class"] = torch.from_numpy(cls.astype(np.int32)).to(DEV)
    a = np.where(live[:, None], a, np.float32(0.0))
    return y, xe, kw, a


def _references(kind, fst, oracle, host, S, T, frames, y, b, a, l2):
    """The float64 and the float32-oracle compositions: dicts of objf, l2_term, weight, deriv, xent_deriv, rows t*S + s."""
    og = oracle.DenGraph(fst)
    pi = og.initial_probs()
    if kind == "uniform":
        return br.float64(fst, pi, host, y, b, a, l2, LEAKY), br.oracle32(oracle, og, host, y, b, a, l2, LEAKY)
    if kind == "ragged":
        outs = []
        for fn in (lambda *r: br.float64(fst, pi, *r), lambda *r: br.oracle32(oracle, og, *r)):
            tot = dict(objf=0.0, l2_term=0.0, weight=0.0, deriv=np.zeros((T * S, P)), xent_deriv=np.zeros((T * S, P)))
            for s, n in enumerate(frames):
                rows = np.arange(n) * S + s
                one = fn(host[s], y[rows], b, a[rows], l2, LEAKY)
                for k in ("objf", "l2_term", "weight"):
                    tot[k] += one[k]
                tot["deriv"][rows] = one["deriv"]
                tot["xent_deriv"][rows] = one["xent_deriv"]
            outs.append(tot)
        return tuple(outs)
    logz, gamma = e2e.num_logz(host, y.astype(np.float64), T)
    assert np.isfinite(logz).all()
    yb = br.boosted(y, b, a)
    y64 = y.astype(np.float64)
    l2_term = -0.5 * WEIGHT * l2 * float((y64 * y64).sum())
    den, gden = ind.den_logprob_and_deriv(fst, pi, np.clip(yb.astype(np.float64), -30, 30), S, LEAKY)
    f64 = dict(objf=WEIGHT * (float(logz.sum()) - den), l2_term=l2_term, weight=WEIGHT * S * T,
               deriv=WEIGHT * gamma - WEIGHT * gden - WEIGHT * l2 * y64, xent_deriv=WEIGHT * gamma)
    d32 = oracle.den_forward_backward(og, yb, S, leaky=LEAKY, deriv_weight=-WEIGHT)
    o32 = dict(objf=WEIGHT * float(logz.sum()) - WEIGHT * d32["logprob"], l2_term=l2_term, weight=WEIGHT * S * T,
               deriv=WEIGHT * gamma + d32["deriv"].astype(np.float64) - WEIGHT * l2 * y64, xent_deriv=WEIGHT * gamma)
    return f64, o32


def _lay(y2d, S, T, layout, dtype=torch.float32, grad=True):
    y = torch.as_tensor(y2d).to(DEV).to(dtype)
    if layout == "3d":
        x = y.view(T, S, P).permute(1, 2, 0).contiguous()
    elif layout == "2d":
        x = y.clone()
    elif layout == "2d_strided":
        wide = torch.zeros(S * T, P + 5, dtype=dtype, device=DEV)
        wide[:, :P] = y
        x = wide[:, :P]
    elif layout == "batch_first":
        x = y.view(T, S, P).permute(1, 0, 2).contiguous().transpose(1, 2)
    else:
        assert layout == "time_major"
        x = y.view(T, S, P).clone().permute(1, 2, 0)
    return x.detach().requires_grad_(grad)


def _rows(g, S, T):
    """A gradient in the input's layout as (T*S, P) float64 numpy rows."""
    if g.dim() == 3:
        g = g.permute(2, 0, 1).reshape(T * S, P)
    return g.detach().double().cpu().numpy()


def _step(x, graph, sup, xe=None, **kw):
    loss, res = chain_loss(x, graph, sup, xent_input=xe, leaky_hmm_coefficient=LEAKY, **kw)
    g = gx = None
    if x.requires_grad:
        grads = torch.autograd.grad(loss, (x,) if xe is None else (x, xe))
        g, gx = grads[0], (grads[1] if xe is not None else None)
    return dict(loss=loss.detach(), res=res, g=g, gx=gx)


# ---- against the references ------------------------------------------------------------------------------------------------------------
COMBOS = [  # form, layout, xent, deriv_weights, penalty
    ("hard", "3d", False, False, 0.0),
    ("classes", "2d", True, True, 0.01),
    ("dense", "3d", True, False, 0.01),
    ("dense", "2d_strided", False, True, 0.0),
]


@pytest.mark.parametrize("l2", [0.0, 5e-5])
@pytest.mark.parametrize("kind", ["uniform", "ragged", "e2e"])
@pytest.mark.parametrize("family", ["tied", "general"])
def test_step_against_the_float64_and_oracle_compositions(oracle, kernel_family, family, kind, l2):
    fst, graph = _graph(family, kernel_family)
    S, T, frames, sup, host = _handle(kind, oracle)
    xreg = 0.1
    for form, layout, xent, weighted, c in COMBOS:
        y, xe_np, akw, a = _inputs(S, T, frames, form, out_of_range=c > 0)
        f64, o32 = _references(kind, fst, oracle, host, S, T, frames, y, BOOST, a, l2)
        x = _lay(y, S, T, layout)
        xe = _lay(xe_np, S, T, layout) if xent else None
        w = torch.from_numpy(np.random.default_rng(1).choice(np.array([0.0, 0.5, 1.0, 1.0, 2.25], np.float32), size=S * T)).to(DEV)
        kw = dict(l2_regularize=l2, boost=BOOST, out_of_range_regularize=c, **akw)
        if xent:
            kw.update(xent_regularize=xreg, kaldi_way=True)
        if weighted:
            kw.update(deriv_weights=w)
        launches = _counter("boost_launches")
        got = _step(x, graph, sup, xe, **kw)
        assert _counter("boost_launches") - launches == (3 if l2 else 1)
        data = got["res"].data.numpy().astype(np.float64)
        g = _rows(got["g"], S, T)
        live = (np.arange(T)[:, None] < np.asarray(frames)[None, :]).reshape(-1)
        assert not g[~live].any() and not np.signbit(g[~live]).any()  # padding gradients are +0
        y64 = y.astype(np.float64)
        pen = np.where(y64 > 30, y64 - 30, np.where(y64 < -30, y64 + 30, 0.0)) * float(np.float32(2 * c))
        wr = w.double().cpu().numpy()[:, None] if weighted else 1.0
        what = (family, kind, l2, form, layout)
        for name, r in (("float64", f64), ("oracle", o32)):
            print(what, name, "objf %.7g vs %.7g" % (data[0], r["objf"]), "l2 %.6g vs %.6g" % (data[1], r["l2_term"]),
                  "grad rel err %.3g" % rel_err(g, (-r["deriv"] + pen * live[:, None]) * wr, floor=WEIGHT))
            assert abs(data[0] - r["objf"]) <= REL * abs(r["objf"]), (what, name)
            assert abs(data[1] - r["l2_term"]) <= REL * abs(r["l2_term"]), (what, name)
            assert abs(data[2] - r["weight"]) <= 1e-6 * r["weight"], (what, name)
            assert abs(float(got["loss"]) + r["objf"] / r["weight"]) <= REL * abs(r["objf"] / r["weight"]), (what, name)
            assert rel_err(g, (-r["deriv"] + pen * live[:, None]) * wr, floor=WEIGHT) <= REL, (what, name)
            if xent:
                assert rel_err(_rows(got["gx"], S, T), -xreg * r["xent_deriv"] * wr, floor=WEIGHT * xreg) <= REL, (what, name)
                want_x = float((xe_np.astype(np.float64) * r["xent_deriv"]).sum())
                assert abs(got["res"].xent_objf - want_x) <= REL * abs(want_x), (what, name)


def test_gradient_element_by_element(oracle, kernel_family):
    """helpers.elementwise on the uniform case (its classes > 1e-3 and > 1e-4 are non-empty for the float64 gradient itself:
    elementwise asserts that), hard reference with classes, l2 = 5e-5, (B, C, T)."""
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, host = _handle("uniform", oracle)
    y, _, akw, a = _inputs(S, T, frames, "classes")
    f64, _ = _references("uniform", fst, oracle, host, S, T, frames, y, BOOST, a, 5e-5)
    got = _step(_lay(y, S, T, "3d"), graph, sup, l2_regularize=5e-5, boost=BOOST, **akw)
    elementwise(_rows(got["g"], S, T), -f64["deriv"], "boosted gradient")


# ---- the denominator saw exactly y_b, and only the denominator ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "ragged"])
@pytest.mark.parametrize("form", ["hard", "classes", "dense"])
def test_only_the_denominator_sees_the_boost(oracle, kernel_family, kind, form):
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, _ = _handle(kind, oracle)
    y, xe_np, akw, a = _inputs(S, T, frames, form)
    kw = dict(l2_regularize=0.0, xent_regularize=0.1, kaldi_way=True, per_sequence=True)
    x, xe = _lay(y, S, T, "3d"), _lay(xe_np, S, T, "3d")
    got = _step(x, graph, sup, xe, boost=BOOST, **akw, **kw)
    a_bct = torch.from_numpy(a).to(DEV).view(T, S, P).permute(1, 2, 0)
    xb = (x.detach().float() - torch.tensor(BOOST, dtype=torch.float32, device=DEV) * a_bct).contiguous().requires_grad_(True)
    on_yb = _step(xb, graph, sup, _lay(xe_np, S, T, "3d"), **kw)
    plain = _step(_lay(y, S, T, "3d"), graph, sup, _lay(xe_np, S, T, "3d"), **kw)
    seq, seq_b, seq_p = got["res"].per_sequence, on_yb["res"].per_sequence, plain["res"].per_sequence
    _same(seq.den_logprob, seq_b.den_logprob, "den_logprob: the plain call on the boosted tensor")
    _same(seq.num_logprob, seq_p.num_logprob, "num_logprob: the plain call on y")
    _same(seq.xent_sum, seq_p.xent_sum, "xent_sum")
    _same(got["gx"], plain["gx"], "xent gradient")
    assert got["res"].xent_objf == plain["res"].xent_objf
    assert not torch.equal(seq.den_logprob, seq_p.den_logprob) and not seq.status.any()
    # (with l2 == 0 the MMI gradient is the numerator's on y minus the denominator's on y_b: also a plain call's bits apart)
    assert float((got["g"] - plain["g"]).abs().max()) > 1e-4


# ---- no effect where there should be none --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["3d", "2d", "batch_first"])
def test_no_boost_is_the_plain_call(oracle, kernel_family, layout):
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, _ = _handle("uniform", oracle)
    y, xe_np, akw, _ = _inputs(S, T, frames, "hard")
    kw = dict(l2_regularize=5e-5, xent_regularize=0.1, kaldi_way=True, per_sequence=True)
    plain = _step(_lay(y, S, T, layout), graph, sup, _lay(xe_np, S, T, layout), **kw)
    launches = _counter("boost_launches")
    for opt in (dict(boost=0.0, **akw), dict(boost=BOOST), dict(boost=0.0)):
        got = _step(_lay(y, S, T, layout), graph, sup, _lay(xe_np, S, T, layout), **opt, **kw)
        for k in ("loss", "g", "gx"):
            _same(got[k], plain[k], k)
        _same(got["res"].data, plain["res"].data, "results")
        assert got["res"].xent_objf == plain["res"].xent_objf
        _same(got["res"].per_sequence.den_logprob, plain["res"].per_sequence.den_logprob, "den_logprob")
    assert _counter("boost_launches") == launches


def test_a_reference_that_scores_nothing_is_the_plain_call(oracle, kernel_family):
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, _ = _handle("uniform", oracle)
    y, _, _, _ = _inputs(S, T, frames, "hard")
    ref = torch.full((S, T), -1, dtype=torch.int32, device=DEV)
    plain = _step(_lay(y, S, T, "3d"), graph, sup, l2_regularize=0.0)
    launches = _counter("boost_launches")
    got = _step(_lay(y, S, T, "3d"), graph, sup, l2_regularize=0.0, boost=BOOST, boost_ref=ref)
    assert _counter("boost_launches") == launches + 1
    _same(got["g"], plain["g"], "grad")
    _same(got["loss"], plain["loss"], "loss")
    _same(got["res"].data, plain["res"].data, "results")


# ---- layouts and dtypes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "ragged"])
@pytest.mark.parametrize("form", ["classes", "dense"])
def test_views_give_the_bits_of_the_contiguous_call(oracle, kernel_family, kind, form):
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, _ = _handle(kind, oracle)
    y, xe_np, akw, _ = _inputs(S, T, frames, form, out_of_range=True)
    kw = dict(l2_regularize=5e-5, xent_regularize=0.1, kaldi_way=True, boost=BOOST, out_of_range_regularize=0.01, **akw)
    for layout in ("batch_first", "time_major"):
        x, xe = _lay(y, S, T, layout), _lay(xe_np, S, T, layout)
        got = _step(x, graph, sup, xe, **kw)
        xc, xec = x.detach().contiguous().requires_grad_(True), xe.detach().contiguous().requires_grad_(True)
        want = _step(xc, graph, sup, xec, **kw)
        for k in ("loss", "g", "gx"):
            _same(got[k].contiguous(), want[k], "%s %s" % (layout, k))
        _same(got["res"].data, want["res"].data, "results")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("layout", ["3d", "2d_strided", "batch_first"])
def test_sixteen_bit_inputs_are_the_float32_call_rounded_once(oracle, kernel_family, dtype, layout):
    """The project's 16-bit contract (test_gpu_half.py): results of the call on ``x.float()``, gradients its ``.to(dtype)``."""
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, _ = _handle("ragged", oracle)
    y, xe_np, akw, _ = _inputs(S, T, frames, "dense")
    kw = dict(l2_regularize=5e-5, xent_regularize=0.1, kaldi_way=True, boost=BOOST, **akw)
    x, xe = _lay(y, S, T, layout, dtype), _lay(xe_np, S, T, layout, dtype)
    got = _step(x, graph, sup, xe, **kw)
    xf = x.detach().float().contiguous().requires_grad_(True)
    xef = xe.detach().float().contiguous().requires_grad_(True)
    want = _step(xf, graph, sup, xef, **kw)
    assert got["g"].dtype == dtype and got["loss"].dtype == dtype
    _same(got["res"].data, want["res"].data, "results")
    _same(got["loss"], want["loss"].to(dtype), "loss")
    gw, gxw = want["g"].to(dtype), want["gx"].to(dtype)
    if dtype == torch.float16 and layout == "batch_first":  # (up to the sign of an exactly zero element: the existing contract)
        assert torch.equal(got["g"].float(), gw.float()) and torch.equal(got["gx"].float(), gxw.float())
    else:
        _same(got["g"].contiguous(), gw.contiguous(), "grad")
        _same(got["gx"].contiguous(), gxw.contiguous(), "xent grad")


# ---- shift -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one_class", "dense_ones"])
def test_constant_accuracy_shifts_the_objective(oracle, kernel_family, form):
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, _ = _handle("ragged", oracle)
    y, _, _, _ = _inputs(S, T, frames, "hard")
    if form == "one_class":  # every pdf in the reference's class
        akw = dict(boost_ref=torch.zeros(S, T, dtype=torch.int32, device=DEV), boost_pdf_class=torch.zeros(P, dtype=torch.int64, device=DEV))
    else:
        akw = dict(boost_accuracy=torch.ones(S * T, P, device=DEV))
    plain = _step(_lay(y, S, T, "3d"), graph, sup, l2_regularize=5e-5)
    got = _step(_lay(y, S, T, "3d"), graph, sup, l2_regularize=5e-5, boost=BOOST, **akw)
    p, q = plain["res"].data.numpy().astype(np.float64), got["res"].data.numpy().astype(np.float64)
    want = p[0] + WEIGHT * BOOST * sum(frames)
    assert abs(q[0] - want) <= REL * abs(want), (q, p)
    assert abs(q[1] - p[1]) <= REL * abs(p[1]) and q[2] == p[2]
    assert rel_err(_rows(got["g"], S, T), _rows(plain["g"], S, T), floor=WEIGHT) <= REL


# ---- failures and refusals ----------------------------------------------------------------------------------------------------------------
def test_a_nan_accuracy_fails_its_sequence_alone(oracle, kernel_family):
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, _ = _handle("ragged", oracle)
    y, xe_np, akw, _ = _inputs(S, T, frames, "dense")
    bad = akw["boost_accuracy"].clone()
    bad[2 * S + 1, 5] = float("nan")  # frame 2 of sequence 1
    kw = dict(l2_regularize=5e-5, xent_regularize=0.1, kaldi_way=True, boost=BOOST)
    clean = _step(_lay(y, S, T, "3d"), graph, sup, _lay(xe_np, S, T, "3d"), on_failure="sequence", boost_accuracy=akw["boost_accuracy"], **kw)
    got = _step(_lay(y, S, T, "3d"), graph, sup, _lay(xe_np, S, T, "3d"), on_failure="sequence", boost_accuracy=bad, **kw)
    assert got["res"].failed.tolist() == [1] and clean["res"].failed.tolist() == []
    others = [0, 2, 3]
    for k in ("g", "gx"):
        assert not _bits(got[k][1]).any(), k  # the failed sequence's rows: +0
        _same(got[k][others], clean[k][others], k)
    seq, seq_c = got["res"].per_sequence, clean["res"].per_sequence
    _same(seq.den_logprob[others], seq_c.den_logprob[others], "den_logprob")
    _same(seq.num_logprob, seq_c.num_logprob, "num_logprob")
    assert float(got["res"].data[2]) == pytest.approx(WEIGHT * (sum(frames) - frames[1]))
    whole = _step(_lay(y, S, T, "3d"), graph, sup, _lay(xe_np, S, T, "3d"), boost_accuracy=bad, **kw)
    data = whole["res"].data
    assert bool(data[0] == torch.tensor(-10.0) * data[2]) and float(data[2]) == pytest.approx(WEIGHT * sum(frames))  # the whole-minibatch route
    assert not _bits(whole["gx"]).any()


def test_kaldi_way_false_with_the_xent_branch_is_refused(oracle, kernel_family):
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, _ = _handle("uniform", oracle)
    y, xe_np, akw, _ = _inputs(S, T, frames, "hard")
    launches = _counter("den_launches")
    with pytest.raises(ValueError):
        chain_loss(_lay(y, S, T, "3d"), graph, sup, xent_regularize=0.1, xent_input=_lay(xe_np, S, T, "3d"), kaldi_way=False,
                   boost=BOOST, **akw)
    with pytest.raises(ValueError):
        chain_loss(_lay(y, S, T, "3d"), graph, sup, boost=BOOST, boost_accuracy=torch.zeros(S * T, P))  # (on the CPU)
    assert _counter("den_launches") == launches
    # (without the xent branch kaldi_way decides nothing)
    chain_loss(_lay(y, S, T, "3d"), graph, sup, kaldi_way=False, boost=BOOST, **akw)


def test_evaluation_step_is_boosted_too(oracle, kernel_family):
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, _ = _handle("ragged", oracle)
    y, _, akw, _ = _inputs(S, T, frames, "classes")
    for layout in ("3d", "2d"):
        train = _step(_lay(y, S, T, layout), graph, sup, l2_regularize=5e-5, boost=BOOST, **akw)
        backward = _counter("den_backward_launches")
        with torch.no_grad():
            got = _step(_lay(y, S, T, layout, grad=False), graph, sup, l2_regularize=5e-5, boost=BOOST, **akw)
        assert _counter("den_backward_launches") == backward
        _same(got["res"].data, train["res"].data, "results")
        _same(got["loss"], train["loss"], "loss")


# ---- no sync, capturable ------------------------------------------------------------------------------------------------------------------
def test_no_host_synchronisation_and_capture(oracle, kernel_family):
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, _ = _handle("ragged", oracle)
    y, xe_np, akw, _ = _inputs(S, T, frames, "classes")
    ref = akw["boost_ref"].to(torch.int32)  # (read where it lies: a replay sees its current values)
    akw = dict(akw, boost_ref=ref)
    x, xe = _lay(y, S, T, "3d"), _lay(xe_np, S, T, "3d")
    kw = dict(l2_regularize=5e-5, xent_regularize=0.1, kaldi_way=True, boost=BOOST, **akw)
    seen = []

    def step():
        loss, res = chain_loss(x, graph, sup, xent_input=xe, leaky_hmm_coefficient=LEAKY, **kw)
        g, gx = torch.autograd.grad(loss, (x, xe))
        seen.append(res)
        return loss.detach(), g, gx

    step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    side.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        captured = step()
    captured_results = seen[-1]
    first = [t.clone() for t in captured]
    live = torch.from_numpy(np.arange(T)[None, :] < np.asarray(frames)[:, None]).to(DEV)
    ref.copy_(torch.where(live, (ref + 7) % P, ref))
    launches = _counter("boost_launches")
    cg.replay()
    torch.cuda.synchronize()
    assert _counter("boost_launches") == launches  # (no library call: the graph's own nodes ran)
    got = [t.clone() for t in captured]
    captured_results.invalidate()
    got_data = captured_results.data.clone()
    want = step()
    torch.cuda.synchronize()
    for u, v in zip(got, want):
        _same(u, v, "replay")
    _same(got_data, seen[-1].data, "results")
    assert float((got[1] - first[1]).abs().max()) > 1e-4  # (the changed reference changed the gradient)


# ---- it does what it is for ------------------------------------------------------------------------------------------------------------------
SGD = dict(steps=8, lr=0.5, boost=2.0)


def _sgd_error_f64(fst, pi, host, y0, ref_np, b, S, T):
    a = br.indicator(ref_np, None, P)
    y = y0.astype(np.float64).copy()
    for _ in range(SGD["steps"]):
        r = br.float64(fst, pi, host, y.astype(np.float32), b, a, 0.0, LEAKY)
        y = y.astype(np.float32).astype(np.float64) + SGD["lr"] * r["deriv"]
    _, gden = ind.den_logprob_and_deriv(fst, pi, np.clip(y, -30, 30), S, LEAKY)
    return S * T - float((gden * a).sum())


def test_the_margin_lowers_the_expected_frame_error(oracle, kernel_family):
    """Eight SGD steps on y itself (lr 0.5, ascent on objf) from one start, with boost = 2 and without, against the hard
    reference that the supervision's own best path gives: the boosted run must end with the lower expected frame error
    T - E[A] under the (unboosted) denominator.  The same steps in float64 on the CPU (_sgd_error_f64, against the same
    reference) end at 6.2500 frames of 36 without the boost and 1.6367 with it: a gap of 4.6 frames, where float32 rounding
    moves an expected accuracy by some 1e-4.  The test asserts that gap to be more than one frame before it looks at the GPU's
    figures (6.249999 and 1.636669 when it was written)."""
    fst, graph = _graph("tied", kernel_family)
    S, T, frames, sup, host = _handle("uniform", oracle)
    y0 = synth.random_nnet_output(S, T, P, seed=7)
    ref, _ = sup.best_path(torch.from_numpy(y0).to(DEV))
    ref_np = ref.cpu().numpy()
    pi = oracle.DenGraph(fst).initial_probs()
    f64 = {b: _sgd_error_f64(fst, pi, host, y0, ref_np, b, S, T) for b in (0.0, SGD["boost"])}
    print("float64: expected frame error %.6f without the boost, %.6f with it" % (f64[0.0], f64[SGD["boost"]]))
    assert f64[0.0] - f64[SGD["boost"]] > 1.0, f64  # (the case shows the effect well clear of rounding)
    errs = {}
    for b in (0.0, SGD["boost"]):
        x = torch.from_numpy(y0).to(DEV).requires_grad_(True)
        for _ in range(SGD["steps"]):
            loss, _ = chain_loss(x, graph, sup, leaky_hmm_coefficient=LEAKY, boost=b, boost_ref=ref)
            (g,) = torch.autograd.grad(loss, x)
            x = (x.detach() - SGD["lr"] * g).requires_grad_(True)
        acc, _ = graph.expected_accuracy(x.detach(), ref, leaky_hmm_coefficient=LEAKY, n_batch=S)
        errs[b] = S * T - float(acc.sum())
        print("boost %g: expected frame error %.6f" % (b, errs[b]))
    assert errs[SGD["boost"]] < errs[0.0], errs
