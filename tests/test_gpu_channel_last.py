"""Channel-last views on the GPU: ``chain_loss`` on the ``(B, C, T)`` views a batch-first or time-major model hands over
(``tests/channel_last_cases.py``) without a copy made contiguous first -- ``tc_chain_step_strided`` in
``TC_LAYOUT_CHANNEL_LAST``, or for a time-major view the 2-D step on the memory where it lies.

The acceptance rule costs no tolerance: loss, results, ``xent_objf`` and every gradient element are bit for bit those of the
one call on the contiguous copy of the same values -- the ``(B, C, T)`` step, or for a view that is 2-D rows in memory
(time-major, or one sequence) the 2-D step on the copied rows.  The copy kernels are held to their numpy statement on their
own, every byte around what they address included; counters show which route ran."""
import ctypes as C

import numpy as np
import pytest
import torch

from torchain_amd import functions, io, synth
from torchain_amd._lib import TC_DTYPE_BF16, TC_DTYPE_F16, TC_DTYPE_F32, lib
from torchain_amd.functions import chain_loss

import channel_last_cases as clc
import e2e_reference as ref
import out_of_range_cases as oor
from helpers import REL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
_TC = {torch.float32: TC_DTYPE_F32, torch.bfloat16: TC_DTYPE_BF16, torch.float16: TC_DTYPE_F16}
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
XENT = [None, True, False]  # no cross-entropy branch, kaldi_way=True, kaldi_way=False
L2, LEAKY, XREG = 5e-4, 0.05, 0.1
SENTINEL = 7.0


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.detach().contiguous().view(_BITS[t.dtype]).cpu()


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, a.dtype, b.dtype, a.shape, b.shape)
    diff = _bits(a) != _bits(b)
    assert not bool(diff.any()), "%s: %d of %d elements differ" % (what, int(diff.sum()), diff.numel())


def _counter(key):
    return int(lib.tc_debug_counter(key))


def _weights(rows, seed):
    pool = np.array([0.0, 1.0 / 255, 128.0 / 255, 1.0, 1.0, 1.5, 3.25], np.float32)
    w = np.random.default_rng(seed).choice(pool, size=rows)
    w[:min(rows, len(pool))] = pool[:min(rows, len(pool))]
    return torch.from_numpy(w.astype(np.float32))


# ---- 1. the copy kernels alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,B,T", clc.SHAPES)
def test_rows_gather_and_scatter_are_their_numpy_statement(P, B, T, dtype):
    """tc_rows_gather / tc_rows_scatter on every view, exactly; the 2-D side has a row stride of P + 4; every byte outside the
    addressed elements -- the 2-D matrix's padding columns, guards either side of the dense gradient, the view itself --
    is what it was."""
    rng = np.random.default_rng(P * 100 + B * 10 + T)
    y, n = oor.overwrite(rng.normal(size=(T * B, P)).astype(np.float32) * 3.0, "dense")
    assert n > 0
    g_host = np.full((T * B, P + 4), 1e30, np.float32)  # (a scatter that reads a padding column shows)
    g_host[:, :P] = rng.normal(size=(T * B, P)).astype(np.float32)
    g_host[0, :3] = [0.0, -0.0, 1e-30]
    g2d = torch.from_numpy(g_host).to(DEV)
    w_host = _weights(T * B, 3).numpy()
    w = torch.from_numpy(w_host).to(DEV)
    N, G = B * T * P, 64
    for kind in clc.VIEWS:
        leaf = clc.make_leaf(kind, y, B, T, DEV, dtype).detach()
        before = leaf.clone()
        v = clc.region(kind, leaf, P)
        sb, st = v.stride(0), v.stride(2)
        out = torch.full((T * B, P + 4), SENTINEL, device=DEV)
        assert lib.tc_rows_gather(_ptr(v), _TC[dtype], B, P, T, sb, st, _ptr(out), P + 4, 0, _stream()) == 0, kind
        flat = leaf.reshape(-1).float().cpu().numpy()
        want = clc.gather_np(flat, v.storage_offset(), B, T, P, sb, st, P + 4, SENTINEL)
        _same_bits(out, torch.from_numpy(want), "gather, " + kind)
        y_btp = v.permute(0, 2, 1).float().cpu().numpy()
        for ww, c in ((None, 0.0), (w, 0.0), (None, 0.25), (w, 0.25)):
            buf = torch.full((G + N + G,), SENTINEL, dtype=dtype, device=DEV)
            dense = buf[G:G + N]
            rc = lib.tc_rows_scatter(_ptr(g2d), P + 4, _TC[dtype], B, P, T, -1.0, _ptr(ww), c, _ptr(v), sb, st, _ptr(dense), 0,
                                     _stream())
            assert rc == 0, (kind, c)
            f32 = clc.scatter_np(g_host, B, T, P, -1.0, w=w_host if ww is not None else None, c=c, y_btp=y_btp)
            _same_bits(dense.view(B, T, P), torch.from_numpy(f32).to(DEV).to(dtype), "scatter, %s, w %s, c %g" % (kind, ww is not None, c))
            guards = torch.cat([buf[:G], buf[G + N:]])
            assert bool((guards == SENTINEL).all()), (kind, "the scatter wrote outside the dense gradient")
        _same_bits(leaf, before, "the view's leaf, " + kind)


# ---- 2. chain_loss on each view against chain_loss on the contiguous copy ------------------------------------------------
_graphs = {}


def _workload(P, B, T):
    key = (P, B, T)
    if key not in _graphs:
        fst = synth.random_den_fst(40, 4, P, seed=6)
        graph = io.DenominatorGraph(fst, P).prepare(DEV)
        ssup = synth.random_supervision(fst, B, T, 2, seed=1)
        y, n = oor.overwrite(synth.random_nnet_output(B, T, P, seed=1), "dense")
        assert n > 0
        xe = synth.random_nnet_output(B, T, P, seed=2)
        _graphs[key] = dict(fst=fst, graph=graph, sup=io.Supervision.from_synth(ssup), ssup=ssup, y=y, xe=xe)
    return _graphs[key]


def _views(pair, y, xe, B, T, dtype):
    """(input view, xent_input view, grads(), leaf_grads()) of one pair of clc.PAIRS.  grads(): the gradients that reach the
    two views, as backward returned them.  leaf_grads(): the same regions of the leaves' own .grad -- for a joint head ONE
    leaf, into which autograd has added the two halves' gradients (an addition of zeros, which turns a -0 into +0: equal
    values, not always equal bits)."""
    P = y.shape[1]
    if pair in ("head", "head_swapped"):  # ONE leaf (B, T, 2P): the chain output in one half, the xent output in the other
        first, second = ("head_lo", "head_hi") if pair == "head" else ("head_hi", "head_lo")
        leaf = clc.make_leaf(first, y, B, T, DEV, dtype).detach()
        clc.region(second, leaf, P).copy_(torch.as_tensor(xe).reshape(T, B, P).permute(1, 2, 0).to(DEV).to(dtype))
        leaf.requires_grad_(True)
        x, xv = clc.region(first, leaf, P), clc.region(second, leaf, P)
        leaf_grads = lambda: (clc.region(first, leaf.grad, P), clc.region(second, leaf.grad, P))  # noqa: E731
    else:
        a, b = clc.make_leaf(pair, y, B, T, DEV, dtype), clc.make_leaf(pair, xe, B, T, DEV, dtype)
        x, xv = clc.region(pair, a, P), clc.region(pair, b, P)
        leaf_grads = lambda: (clc.region(pair, a.grad, P), clc.region(pair, b.grad, P) if b.grad is not None else None)  # noqa: E731
    x.retain_grad()
    xv.retain_grad()
    return x, xv, (lambda: (x.grad, xv.grad)), leaf_grads


def _call(x, xe, graph, sup, xent, w=None, c=0.0, l2=L2, leaky=LEAKY, fn=chain_loss):
    kw = dict(l2_regularize=l2, leaky_hmm_coefficient=leaky, deriv_weights=w, out_of_range_regularize=c)
    if xent is not None:
        kw.update(xent_regularize=XREG, xent_input=xe, kaldi_way=xent)
    loss, res = fn(x, graph, sup, **kw)
    loss.sum().backward()
    return loss.detach(), res.data.clone(), res.xent_objf


def _is_rows(pair, B):
    """Whether a pair of clc.PAIRS is 2-D rows in memory, from how it was built (not from the predicate under test): the
    time-major leaves, and any leaf of one sequence, whose frames are a run of rows whatever the layout."""
    return pair in clc.TIME_MAJOR or B == 1


def _copies(x, xe, rows):
    """The contiguous copies the acceptance rule names: (B, C, T), or (``rows``) 2-D rows t*B + b for a view that is 2-D rows
    in memory; and the way back for a gradient of such a copy."""
    B, P, T = x.shape

    def copy(v):
        v = v.detach()
        return (v.permute(2, 0, 1).reshape(T * B, P) if rows else v).contiguous().requires_grad_(True)

    def back(g):
        return g.view(T, B, P).permute(1, 2, 0) if rows else g
    return copy(x), (copy(xe) if xe is not None else None), back


def _reference(x, xe, graph, sup, xent, rows, **kw):
    """The existing one call on the contiguous copy.  Returns (loss, results, xent_objf, grad, xent grad) with the gradients
    in (B, C, T)."""
    xc, xec, back = _copies(x, xe if xent is not None else None, rows)
    assert functions._one_call(xc)
    out = _call(xc, xec, graph, sup, xent, **kw)
    return out + (back(xc.grad), back(xec.grad) if xec is not None else None)


def _compare(x, xe, grads, graph, sup, xent, what, rows, **kw):
    """``rows`` (``_is_rows``): the view is 2-D rows in memory, so it is held to the 2-D call on the copied rows and must not
    count as a channel-last step; otherwise to the (B, C, T) call, and it must."""
    steps = _counter(b"channel_last_steps")
    got = _call(x, xe, graph, sup, xent, **kw)
    assert _counter(b"channel_last_steps") - steps == (0 if rows else 1), what
    want = _reference(x, xe, graph, sup, xent, rows, **kw)
    _same_bits(got[0], want[0], what + ": loss")
    _same_bits(got[1], want[1], what + ": results")
    assert got[2] == want[2], (what, got[2], want[2])
    g, xg = grads()
    assert g.dtype == x.dtype and tuple(g.shape) == tuple(x.shape)
    _same_bits(g, want[3], what + ": grad")
    if xent is not None:
        _same_bits(xg, want[4], what + ": xent grad")
        assert got[2] is not None and np.isfinite(got[2])
    return got, want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,B,T", clc.SHAPES)
def test_chain_loss_on_a_view_is_chain_loss_on_its_contiguous_copy(P, B, T, dtype):
    """Every pair of views x {no xent, kaldi_way, the reference's way} x {plain, deriv_weights and the penalty}, on outputs of
    which three whole rows lie beyond +-30."""
    s = _workload(P, B, T)
    w = _weights(B * T, 4)
    for pair in clc.PAIRS:
        for xent in XENT:
            for opts in (dict(), dict(w=w, c=0.25)):
                x, xe, grads, leaf_grads = _views(pair, s["y"], s["xe"], B, T, dtype)
                got, _ = _compare(x, xe, grads, s["graph"], s["sup"], xent, "%s xent=%s %s" % (pair, xent, sorted(opts)),
                                  _is_rows(pair, B), **opts)
                for g, lg in zip(grads(), leaf_grads()):  # ... and they are what the leaves receive
                    assert (g is None and xent is None) or torch.equal(g, lg), (pair, xent)
                assert not oor.took_soft_failure(float(got[1][0]), float(got[1][2])), got[1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_medium_workload(dtype):
    """700 states, P = 300, 4 x 30 (out_of_range_cases.MEDIUM): more rows than one pass of the copy kernels' waves per block,
    several 16-byte lanes per row."""
    fst, ssup, y, n = oor.workload(oor.MEDIUM, "sparse")
    S, T, P = oor.MEDIUM["S"], oor.MEDIUM["T"], fst.num_pdfs
    graph, sup = io.DenominatorGraph(fst, P).prepare(DEV), io.Supervision.from_synth(ssup)
    xe = synth.random_nnet_output(S, T, P, seed=5)
    assert n > 0
    for pair, xent in (("dense", True), ("head_swapped", False), ("batch_pad", None), ("time_major_pad", True)):
        x, xv, grads, _ = _views(pair, y, xe, S, T, dtype)
        _compare(x, xv, grads, graph, sup, xent, pair, _is_rows(pair, S), w=_weights(S * T, 5), c=0.25, l2=1e-3, leaky=1e-5)


def test_float16_exact_zero_gradients():
    """l2 = 0 and three pdfs that no arc of the denominator graph and no supervision carries: their gradient elements are exact
    zeros, the one place where a float16 channel-last step may differ from the (B, C, T) step in bits.  Pinned: the view's
    gradient is, bit for bit, the float32 step's gradient on the same view ``.to(float16)`` (a zero's sign included: the
    scatter rounds the float32 value -1 * g); against the float16 (B, C, T) step, whose copy back fuses the product into the
    conversion on some of its paths and then returns +0 for -1 * (+0), it is equal in value everywhere and differs in bits
    only where both are zero.  float32 and bfloat16 views have the (B, C, T) step's bits there too."""
    P, B, T, unused = 24, 2, 6, 3
    fst = synth.random_den_fst(40, 4, P - unused, seed=6)._replace(num_pdfs=P)
    graph = io.DenominatorGraph(fst, P).prepare(DEV)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, B, T, 2, seed=1))
    y = synth.random_nnet_output(B, T, P, seed=1).astype(np.float16).astype(np.float32)  # (exact in every dtype but bfloat16)
    grads = {}
    for pair in ("dense", "head_hi_only"):
        kind = "dense" if pair == "dense" else "head_hi"
        for dtype in DTYPES:
            leaf = clc.make_leaf(kind, y, B, T, DEV, dtype)
            x = clc.region(kind, leaf, P)
            x.retain_grad()
            steps = _counter(b"channel_last_steps")
            res = _call(x, None, graph, sup, None, l2=0.0, leaky=1e-5)
            assert _counter(b"channel_last_steps") == steps + 1
            assert not oor.took_soft_failure(float(res[1][0]), float(res[1][2]))
            xc = x.detach().contiguous().requires_grad_(True)
            _call(xc, None, graph, sup, None, l2=0.0, leaky=1e-5)
            g, gc = x.grad, xc.grad
            grads[dtype] = g
            assert bool((g[:, P - unused:, :] == 0).all()) and bool((g[:, :P - unused, :] != 0).any())
            assert torch.equal(g, gc), (pair, dtype)
            differ = _bits(g) != _bits(gc)
            if dtype == torch.float16:
                assert bool(((g == 0) & (gc == 0)).cpu()[differ].all()), "bits differ somewhere other than an exact zero"
            else:
                assert not bool(differ.any()), (pair, dtype)
        _same_bits(grads[torch.float16], grads[torch.float32].to(torch.float16), pair + ": float16 is the float32 gradient cast once")


# ---- 3. which route ran -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,B,T", [(24, 2, 6), (21, 3, 5)])
def test_counters_show_the_route(P, B, T):
    s = _workload(P, B, T)
    keys = (b"channel_last_steps", b"layout_launches", b"den_launches")

    def run(x, xe=None, xent=None, grad=True):
        before = [_counter(k) for k in keys]
        if grad:
            _call(x, xe, s["graph"], s["sup"], xent)
        else:
            with torch.no_grad():
                chain_loss(x, s["graph"], s["sup"], L2, LEAKY)
        return [_counter(k) - b for k, b in zip(keys, before)]
    for pair in ("dense", "head", "head_swapped", "batch_pad"):
        x, xe, _, _ = _views(pair, s["y"], s["xe"], B, T, torch.float32)
        assert run(x) == [1, 2, 1], pair                      # one gather, one scatter
        x, xe, _, _ = _views(pair, s["y"], s["xe"], B, T, torch.bfloat16)
        assert run(x, xe, True) == [1, 4, 1], pair            # two of each with the xent branch
        assert run(x.detach(), grad=False) == [1, 1, 1], pair  # evaluation: the gather alone
    # contiguous (B, C, T): its two transposes, no channel-last step; 2-D rows: no layout launch at all
    x, _, _, _ = _views("dense", s["y"], s["xe"], B, T, torch.float32)
    assert run(x.detach().contiguous().requires_grad_(True)) == [0, 2, 1]
    assert run(torch.from_numpy(s["y"]).to(DEV).requires_grad_(True)) == [0, 0, 1]
    # a time-major view is the 2-D layout where it lies: no copy kernel of any kind, for any dtype, with or without xent
    for pair in clc.TIME_MAJOR:
        for dtype in DTYPES:
            x, xe, _, _ = _views(pair, s["y"], s["xe"], B, T, dtype)
            assert run(x) == [0, 0, 1], (pair, dtype)
            assert run(x, xe, False) == [0, 0, 1], (pair, dtype)
            assert run(x.detach(), grad=False) == [0, 0, 1], (pair, dtype)


# ---- 4. against the CPU oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_dense_batch_first_view_against_the_oracle(oracle, kind):
    """float32, (B, T, P).transpose(1, 2), xent branch on, the penalty on: scalars within 1e-4 relative, -grad against the
    oracle's derivative minus the numpy term and -xent_grad / xent_regularize against its xent derivative, matrix-wise
    1e-4 * max(max |oracle|, weight).  The cross-entropy objective is a scalar: 1e-4 relative to the
    oracle's sum(xent_output * xent_deriv)."""
    fst, ssup, y, n = oor.workload(oor.MEDIUM, kind)
    S, T, P = oor.MEDIUM["S"], oor.MEDIUM["T"], fst.num_pdfs
    assert n > 0
    want = oracle.compute_chain_objf_and_deriv(oracle.DenGraph(fst), ssup, y, 0.0, 1e-5, want_xent=True)
    assert not oor.took_soft_failure(want["objf"], want["weight"])
    graph, sup = io.DenominatorGraph(fst, P).prepare(DEV), io.Supervision.from_synth(ssup)
    xe_rows = synth.random_nnet_output(S, T, P, seed=5)
    x, xe, grads, _ = _views("dense", y, xe_rows, S, T, torch.float32)
    before = _counter(b"channel_last_steps")
    loss, res = chain_loss(x, graph, sup, 0.0, 1e-5, xent_regularize=XREG, xent_input=xe, kaldi_way=True, out_of_range_regularize=0.01)
    loss.backward()
    assert _counter(b"channel_last_steps") == before + 1
    got = res.data.numpy()
    assert abs(got[0] - want["objf"]) <= REL * abs(want["objf"]) and got[2] == want["weight"]
    assert abs(float(loss.detach()) + want["objf"] / want["weight"]) <= REL * abs(want["objf"] / want["weight"])
    g, xg = (t.permute(2, 0, 1).reshape(S * T, P).cpu().numpy() for t in grads())
    floor = float(want["weight"]) / (S * T)
    target = want["deriv"].astype(np.float64) - oor.term(y, 0.01).astype(np.float64)
    err, xerr = rel_err(-g, target, floor=floor), rel_err(-xg / XREG, want["xent_deriv"], floor=floor)
    want_xent = float((xe_rows.astype(np.float64) * want["xent_deriv"]).sum())
    print("%s: rel err grad %.3e, xent grad %.3e; xent objf %.6g against %.6g" % (kind, err, xerr, res.xent_objf, want_xent))
    assert err <= REL and xerr <= REL
    assert abs(res.xent_objf - want_xent) <= REL * abs(want_xent)


# ---- 5. the other numerators --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_end_to_end_supervision(dtype):
    S, T, P = 4, 20, 24
    graph = io.DenominatorGraph(synth.random_den_fst(60, 4, P, seed=31), P).prepare(DEV)
    sup = io.Supervision.from_e2e_fsts(0.9, T, P, ref.batch("chain", S, P, seed=11))
    rng = np.random.default_rng(12)
    y, n = oor.overwrite((rng.normal(size=(S * T, P)) * 2.0).astype(np.float32), "sparse")
    xe = rng.normal(size=(S * T, P)).astype(np.float32)
    for pair, xent in (("dense", True), ("head", False), ("time_major", True)):
        x, xv, grads, _ = _views(pair, y, xe, S, T, dtype)
        _compare(x, xv, grads, graph, sup, xent, "e2e " + pair, _is_rows(pair, S), w=_weights(S * T, 6), c=0.25, l2=1e-4, leaky=1e-5)


def test_level_windowed_numerator():
    P, B, T = 24, 2, 6
    s = _workload(P, B, T)
    assert lib.tc_debug_set(b"force_num_windowed", 1) == 0
    try:
        before = _counter(b"num_windowed_launches")
        for pair, xent in (("dense", True), ("head_swapped", False)):
            x, xv, grads, _ = _views(pair, s["y"], s["xe"], B, T, torch.float32)
            _compare(x, xv, grads, s["graph"], s["sup"], xent, "windowed " + pair, _is_rows(pair, B))
        assert _counter(b"num_windowed_launches") > before
    finally:
        lib.tc_debug_set(b"force_num_windowed", 0)


# ---- 6. evaluation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_evaluation_under_no_grad(dtype):
    P, B, T = 20, 3, 5
    s = _workload(P, B, T)
    kw = dict(l2_regularize=L2, leaky_hmm_coefficient=LEAKY, xent_regularize=XREG)
    for pair in clc.PAIRS:
        for kaldi_way in (True, False):
            x, xe, _, _ = _views(pair, s["y"], s["xe"], B, T, dtype)
            back = _counter(b"den_backward_launches")
            with torch.no_grad():
                loss, res = chain_loss(x, s["graph"], s["sup"], xent_input=xe, kaldi_way=kaldi_way, **kw)
                xc, xec, _ = _copies(x, xe, _is_rows(pair, B))
                lossc, resc = chain_loss(xc.detach(), s["graph"], s["sup"], xent_input=xec.detach(), kaldi_way=kaldi_way, **kw)
            assert _counter(b"den_backward_launches") == back
            _same_bits(loss, lossc, pair + ": loss")
            _same_bits(res.data, resc.data, pair + ": results")
            assert res.xent_objf == resc.xent_objf and np.isfinite(res.xent_objf)
            assert not loss.requires_grad and x.grad is None and xe.grad is None
            # ... and they are the training step's
            want = _reference(x, xe, s["graph"], s["sup"], kaldi_way, _is_rows(pair, B))
            _same_bits(res.data, want[1], pair + ": results of the training step")


# ---- 7. soft failure ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kaldi_way", [True, False])
def test_soft_failure(dtype, kaldi_way):
    """A NaN in the matrix the objective runs on: objf = -10 * weight and the reset gradient (l2 * weight * y, weighted; xent 0),
    the bits of the contiguous call."""
    P, B, T = 24, 2, 6
    s = _workload(P, B, T)
    y, xe = s["y"].copy(), s["xe"].copy()
    (y if kaldi_way else xe)[7, 5] = np.nan
    w = _weights(B * T, 8)
    w[7] = 0.5
    for pair in ("dense", "head", "batch_pad", "time_major_pad"):
        x, xv, grads, _ = _views(pair, y, xe, B, T, dtype)
        got, _ = _compare(x, xv, grads, s["graph"], s["sup"], kaldi_way, "soft failure " + pair, _is_rows(pair, B), w=w, c=0.25, l2=1e-2)
        assert float(got[1][0]) == -10.0 * B * T and float(got[1][2]) == B * T
        g, xg = grads()
        assert torch.count_nonzero(xg) == 0 and got[2] == 0.0
        assert torch.count_nonzero(torch.nan_to_num(g.float())) > 0  # (l2 != 0: the reset gradient is not zero)


# ---- 8. mixed inputs keep their routes and their values -----------------------------------------------------------------
def test_mixed_inputs_take_the_routes_they_took():
    """Pairs that do not go to the step together are made contiguous and take the one call: all five outputs are bit for bit
    those of ``chain_loss`` on the contiguous copies (what the planner makes of them).  float32 pairs, which went through
    ``_ChainLoss3d`` before, are held to that class as well, called directly on the contiguous copies: ``results`` and both
    gradients bit for bit (but for the sign of the xent gradient's exact zeros: ``torch.equal``, as
    ``test_one_call_step_equals_the_multi_call_wrappers`` compares the two routes), ``loss`` and ``xent_objf`` within the 1e-6
    relative the two routes are documented to differ by.
    No channel-last step is counted."""
    from composed_step import _ChainLoss3d
    from torchain_amd.functions import ChainResults
    P, B, T = 20, 3, 5
    s = _workload(P, B, T)
    w = _weights(B * T, 9)

    def through_3d(x, graph, sup, l2_regularize, leaky_hmm_coefficient, deriv_weights, out_of_range_regularize, xent_regularize,
                   xent_input, kaldi_way):
        res = ChainResults()
        return _ChainLoss3d.apply(x, xent_input, res, graph, sup, l2_regularize, leaky_hmm_coefficient, xent_regularize, kaldi_way,
                                  deriv_weights, out_of_range_regularize), res

    def check(x, xe, leaves, what, dtype):
        assert functions._step_plan(x, xe) is None, what
        steps = _counter(b"channel_last_steps")
        got = _call(x, xe, s["graph"], s["sup"], True, w=w, c=0.25)
        assert _counter(b"channel_last_steps") == steps, what
        gx, gxe = leaves()
        ops = functions.plan_step_inputs(functions._spec(x), functions._spec(xe))
        assert set(ops[0] + ops[1]) == {"contiguous"} and ops[2] == ("bct", 0, 0), (what, ops)
        xc, xec = x.detach().contiguous().requires_grad_(True), xe.detach().contiguous().requires_grad_(True)
        want = _call(xc, xec, s["graph"], s["sup"], True, w=w, c=0.25)  # the normalised copies
        _same_bits(got[0], want[0], what + ": loss")
        _same_bits(got[1], want[1], what + ": results")
        assert got[2] == want[2], what
        _same_bits(gx, xc.grad, what + ": grad")
        _same_bits(gxe, xec.grad, what + ": xent grad")
        if dtype != torch.float32:
            return
        xc, xec = x.detach().contiguous().requires_grad_(True), xe.detach().contiguous().requires_grad_(True)
        want = _call(xc, xec, s["graph"], s["sup"], True, w=w, c=0.25, fn=through_3d)  # the composed step
        _same_bits(got[1], want[1], what + ": results, composed")
        _same_bits(gx, xc.grad, what + ": grad, composed")
        # (where the numerator has no posterior the one call leaves the +0 it cleared the gradient with; _ChainLoss3d scaled
        # that zero by -xent_regularize on its way back: -0.  Every other element has the same bits.)
        differ = _bits(gxe) != _bits(xec.grad)
        assert torch.equal(gxe, xec.grad) and not bool((gxe.cpu()[differ] != 0).any()), what + ": xent grad, composed"
        assert abs(float(got[0]) - float(want[0])) <= 1e-6 * abs(float(want[0])), (what, got[0], want[0])
        assert abs(got[2] - want[2]) <= 1e-6 * abs(want[2]), (what, got[2], want[2])

    def bct(rows, dtype):
        return torch.as_tensor(rows).reshape(T, B, P).permute(1, 2, 0).to(DEV).to(dtype).contiguous()

    for dtype in (torch.float32, torch.bfloat16):
        # channel-last input with a contiguous (B, C, T) xent_input
        x, _, g1, _ = _views("dense", s["y"], s["xe"], B, T, dtype)
        xe = bct(s["xe"], dtype).requires_grad_(True)
        check(x, xe, lambda: (g1()[0], xe.grad), "channel-last + contiguous", dtype)
        # a channel-last pair with different strides
        x, _, g1, _ = _views("dense", s["y"], s["xe"], B, T, dtype)
        xe_leaf = clc.make_leaf("batch_pad", s["xe"], B, T, DEV, dtype)
        xe = clc.region("batch_pad", xe_leaf, P)
        assert functions._step_view(x) and functions._step_view(xe)
        check(x, xe, lambda: (g1()[0], clc.region("batch_pad", xe_leaf.grad, P)), "different strides", dtype)
        # a time-major input with a batch-first xent_input
        x, _, g1, _ = _views("time_major", s["y"], s["xe"], B, T, dtype)
        xe_leaf2 = clc.make_leaf("dense", s["xe"], B, T, DEV, dtype)
        xe = clc.region("dense", xe_leaf2, P)
        check(x, xe, lambda: (g1()[0], clc.region("dense", xe_leaf2.grad, P)), "time-major + batch-first", dtype)
        # a 3-D view whose channel stride is not 1
        wide = torch.zeros(B, P, 2 * T, dtype=dtype, device=DEV)
        wide[:, :, ::2] = bct(s["y"], dtype)
        wide.requires_grad_(True)
        x = wide[:, :, ::2]
        assert not functions._step_view(x) and functions.classify_layout(x.shape, x.stride()) == ("other", 0, 0)
        xe = bct(s["xe"], dtype).requires_grad_(True)
        check(x, xe, lambda: (wide.grad[:, :, ::2], xe.grad), "frame stride 2", dtype)


# ---- 9. the C ABI -------------------------------------------------------------------------------------------------------
def _abi_step(entry, s, B, T, P, x, layout_args, grad, ws, dtype=TC_DTYPE_F32, xe=None, xgrad=None):
    out = torch.zeros(6, dtype=torch.float32, device=DEV)
    rc = entry(s["graph"].ptr, s["sup"].ptr, _ptr(x), _ptr(xe), *layout_args, L2, LEAKY, XREG if xe is not None else 0.0, 1,
               _ptr(grad), _ptr(xgrad), C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 12),
               C.c_void_p(out.data_ptr() + 16) if xe is not None else None, None, 0.0, dtype, _ptr(ws), ws.numel(), 0, _stream())
    torch.cuda.synchronize()
    return rc, out


def test_c_abi():
    P, B, T = 24, 2, 6
    s = _workload(P, B, T)
    gp = s["graph"].ptr
    # the workspace of a channel-last step is the (B, C, T) one
    for dtype in (TC_DTYPE_F32, TC_DTYPE_BF16, TC_DTYPE_F16):
        for xent in (0, 1):
            a = lib.tc_chain_step_strided_workspace_bytes(gp, B, T, 2, xent, dtype)
            assert a == lib.tc_chain_step_typed_workspace_bytes(gp, B, T, 1, xent, dtype) > 0
    ws = torch.zeros(int(lib.tc_chain_step_strided_workspace_bytes(gp, B, T, 2, 1, TC_DTYPE_F32)), dtype=torch.uint8, device=DEV)
    rows = torch.from_numpy(s["y"]).to(DEV)
    xrows = torch.from_numpy(s["xe"]).to(DEV)
    bct, xbct = (r.view(T, B, P).permute(1, 2, 0).contiguous() for r in (rows, xrows))
    # layouts 0 and 1 are tc_chain_step_penalized, byte for byte
    for layout, x, xe, row_stride in ((0, rows, xrows, P), (1, bct, xbct, 0)):
        outs = []
        for entry, args in ((lib.tc_chain_step_penalized, (layout, row_stride)), (lib.tc_chain_step_strided, (layout, row_stride, -5, -7))):
            grad, xgrad = torch.full_like(x, SENTINEL), torch.full_like(x, SENTINEL)
            rc, out = _abi_step(entry, s, B, T, P, x, args, grad, ws, xe=xe, xgrad=xgrad)
            assert rc == 0
            outs.append((out, grad, xgrad))
        for a, b, what in zip(outs[0], outs[1], ("scalars", "grad", "xent grad")):
            _same_bits(a, b, "layout %d: %s" % (layout, what))
        assert bool((outs[1][1] != SENTINEL).any())
    # layout 2 on a batch-first tensor: dense (B, T, C) gradients, the (B, C, T) call's values
    btc, xbtc = bct.transpose(1, 2).contiguous(), xbct.transpose(1, 2).contiguous()
    grad, xgrad = torch.full_like(btc, SENTINEL), torch.full_like(btc, SENTINEL)
    steps = _counter(b"channel_last_steps")
    rc, out = _abi_step(lib.tc_chain_step_strided, s, B, T, P, btc, (2, 0, T * P, P), grad, ws, xe=xbtc, xgrad=xgrad)
    assert rc == 0 and _counter(b"channel_last_steps") == steps + 1
    _same_bits(out, outs[0][0], "layout 2: scalars")
    _same_bits(grad.transpose(1, 2), outs[0][1], "layout 2: grad")
    _same_bits(xgrad.transpose(1, 2), outs[0][2], "layout 2: xent grad")
    # bad strides: refused, nothing written
    for sb, st in [(T * P, P - 1), (T * P - 1, P), (-T * P, P), (T * P, -P), (0, P), (P, 0), (P - 1, B * P)]:
        grad, xgrad = torch.full_like(btc, SENTINEL), torch.full_like(btc, SENTINEL)
        ws.fill_(3)
        rc, out = _abi_step(lib.tc_chain_step_strided, s, B, T, P, btc, (2, 0, sb, st), grad, ws, xe=xbtc, xgrad=xgrad)
        assert rc == -1, (sb, st)
        assert bool((grad == SENTINEL).all()) and bool((xgrad == SENTINEL).all()) and bool((out == 0).all()) and bool((ws == 3).all())
    assert _counter(b"channel_last_steps") == steps + 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_c_abi_single_sequence(dtype):
    """B = 1 (21 pdfs, 4 frames: the element-wise paths).  ``chain_loss`` hands a view of one sequence to the 2-D step, so the
    channel-last step of a single sequence is reached through the C entry: a padded (1, T + 2, C) tensor in layout 2 against
    ``tc_chain_step_penalized`` on the contiguous (1, C, T) copy, bit for bit."""
    P, B, T = 21, 1, 4
    s = _workload(P, B, T)
    ws = torch.zeros(int(lib.tc_chain_step_strided_workspace_bytes(s["graph"].ptr, B, T, 2, 1, _TC[dtype])), dtype=torch.uint8,
                     device=DEV)
    leaf, xleaf = (clc.make_leaf("batch_pad", r, B, T, DEV, dtype).detach() for r in (s["y"], s["xe"]))
    x, xe = leaf[:, :T], xleaf[:, :T]                                   # (1, T, C) in a (1, T + 2, C) tensor
    bct, xbct = x.transpose(1, 2).contiguous(), xe.transpose(1, 2).contiguous()
    grad, xgrad = torch.full_like(bct, SENTINEL), torch.full_like(bct, SENTINEL)
    rc, want = _abi_step(lib.tc_chain_step_penalized, s, B, T, P, bct, (1, 0), grad, ws, dtype=_TC[dtype], xe=xbct, xgrad=xgrad)
    assert rc == 0
    dense, xdense = torch.full((B, T, P), SENTINEL, dtype=dtype, device=DEV), torch.full((B, T, P), SENTINEL, dtype=dtype, device=DEV)
    steps = _counter(b"channel_last_steps")
    # (the batch stride of a single sequence is ignored: any value)
    rc, out = _abi_step(lib.tc_chain_step_strided, s, B, T, P, x, (2, 0, -1, x.stride(1)), dense, ws, dtype=_TC[dtype], xe=xe,
                        xgrad=xdense)
    assert rc == 0 and _counter(b"channel_last_steps") == steps + 1
    _same_bits(out, want, "scalars")
    _same_bits(dense.transpose(1, 2), grad, "grad")
    _same_bits(xdense.transpose(1, 2), xgrad, "xent grad")
