"""End-to-end supervisions beyond the resident numerator kernel's limits on the GPU (num_e2e_large_kernels.hip through
``io.Supervision.from_e2e_fsts(..., any_size=True)``): against the float64 reference of tests/e2e_reference.py with the
tolerances of tests/test_gpu_e2e.py (scalars 1e-4 relative, derivatives max |diff| <= 1e-4 * max(max |ref|, w)), and bit for
bit against the resident kernel on handles that fit both (``tc_debug_set("force_num_e2e_large", 1)``).  Every test that should
reach the large kernel asserts that ``num_e2e_large_launches`` moved; cases and references: tests/e2e_large_cases.py."""
import numpy as np
import pytest
import torch

from torchain_amd import io
from torchain_amd._lib import lib
from torchain_amd.functions import ChainResults, chain_loss, compute_chain_objf_and_deriv

import best_path_reference as bp
import den_compose_cases as dc
import e2e_large_cases as lc
import e2e_reference as ref
import ragged_cases as rc
from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 60
REL = 1e-4


def _counter(name):
    return int(lib.tc_debug_counter(name.encode()))


def _large():
    return _counter("num_e2e_large_launches")


_graphs = {}


def _den(P=P):
    if P not in _graphs:
        _graphs[P] = io.DenominatorGraph(lc.den_fst(P), P).prepare(0)
    return _graphs[P]


def _y(S, T, P=P, seed=1, scale=2.0):
    return (np.random.default_rng(seed).normal(size=(S * T, P)) * scale).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _hip(sup, y, l2=lc.L2, leaky=lc.LEAKY, graph=None):
    """The 2-D objective with both derivatives: (results, deriv, xent_deriv) as numpy."""
    graph = graph or _den(y.shape[1])
    yt = torch.from_numpy(np.array(y, copy=True)).to(DEV)  # (the cases' arrays are read-only)
    deriv = torch.full(yt.shape, 7.0, device=DEV)
    xd = torch.full(yt.shape, 7.0, device=DEV)
    res = ChainResults()
    compute_chain_objf_and_deriv(graph, sup, yt, res.data, deriv, xd, l2, leaky, 0.1)
    torch.cuda.synchronize()
    return res.data.numpy().copy(), deriv.cpu().numpy(), xd.cpu().numpy()


def _step(sup, y, xe, graph=None, grad=True, **kw):
    """chain_loss on 2-D inputs, with the cross-entropy branch unless ``xe`` is None: ((loss, results, xent objective, grad,
    xent grad) as numpy, the ChainResults)."""
    graph = graph or _den(y.shape[1])
    x = torch.from_numpy(np.array(y, copy=True)).to(DEV).requires_grad_(grad)
    opts = dict(l2_regularize=lc.L2, leaky_hmm_coefficient=lc.LEAKY)
    xx = None
    if xe is not None:
        xx = torch.from_numpy(xe).to(DEV).requires_grad_(grad)
        opts.update(xent_regularize=0.1, xent_input=xx, kaldi_way=True)
    opts.update(kw)
    with torch.set_grad_enabled(grad):
        loss, res = chain_loss(x, graph, sup, **opts)
    if grad:
        loss.backward()
    torch.cuda.synchronize()
    return (loss.detach().cpu().numpy(), res.data.numpy().copy(), None if xx is None else np.float64(res.xent_objf),
            x.grad.cpu().numpy() if grad else None, xx.grad.cpu().numpy() if grad and xx is not None else None), res


def _same(a, b, what):
    for i, (x, z) in enumerate(zip(a, b)):
        assert (x is None and z is None) or np.array_equal(np.atleast_1d(x).view(np.uint8), np.atleast_1d(z).view(np.uint8)), (what, i)


# ---- against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [True, False], ids=["staged", "in-line"])
@pytest.mark.parametrize("name", list(lc.CASES))
def test_objective_and_derivatives_match_float64(name, overlap, kernel_family):
    """One past each resident limit, the new limit (8192 states, 40000 arcs, 4096 planted pdfs) and a 3000-state FST over 300
    frames, each beside a 5-state FST, with l2, leaky 0.1 and the cross-entropy derivative; on the side stream (staged
    posteriors + scatter) and in line."""
    if not overlap:
        kernel_family("no_num_overlap")
    size, T, PL = lc.CASES[name]
    fsts = list(lc.fsts(name))
    assert lc.sizes(fsts[0]) == size
    sup = io.Supervision.from_e2e_fsts(lc.WEIGHT, T, PL, fsts, any_size=True)
    assert sup.e2e_stats()["kernel"] == "large"
    large, staged = _large(), _counter("num_e2e_staged_launches")
    res, d, xd = _hip(sup, lc.nnet_output(name))
    assert _large() == large + 1
    assert _counter("num_e2e_staged_launches") - staged == (1 if overlap else 0)
    want = lc.reference(name)
    print("%s: objf %.9g (float64 %.9g), deriv %.3g, xent deriv %.3g" % (name, res[0], want["objf"],
          rel_err(d, want["deriv"], floor=lc.WEIGHT), rel_err(xd, want["xent_deriv"], floor=lc.WEIGHT)))
    assert abs(res[0] - want["objf"]) <= REL * abs(want["objf"]), (res, want["objf"])
    assert abs(res[1] - want["l2_term"]) <= REL * abs(want["l2_term"]), (res, want["l2_term"])
    assert res[2] == np.float32(want["weight"])
    assert rel_err(d, want["deriv"], floor=lc.WEIGHT) <= REL
    assert rel_err(xd, want["xent_deriv"], floor=lc.WEIGHT) <= REL


def test_largest_states_and_largest_pdfs_in_two_sequences():
    """10108 states / 4 pdfs beside 8192 states / 7680 pdfs: each sequence at the LDS rule, the two maxima together far beyond
    it.  The numerator against float64, and the best path."""
    fsts, T, PL = list(lc.mixed_fsts()), lc.MIXED_T, lc.MIXED_P
    assert tuple(lc.sizes(f) for f in fsts) == lc.MIXED
    y = lc.nnet_output("mixed")
    sup = io.Supervision.from_e2e_fsts(lc.WEIGHT, T, PL, fsts, any_size=True)
    large = _large()
    res, d, xd = _hip(sup, y)
    assert _large() == large + 1
    want = lc.mixed_reference()
    print("mixed: objf %.9g (float64 %.9g), deriv %.3g, xent deriv %.3g" % (res[0], want["objf"],
          rel_err(d, want["deriv"], floor=lc.WEIGHT), rel_err(xd, want["xent_deriv"], floor=lc.WEIGHT)))
    assert abs(res[0] - want["objf"]) <= REL * abs(want["objf"])
    assert rel_err(d, want["deriv"], floor=lc.WEIGHT) <= REL
    assert rel_err(xd, want["xent_deriv"], floor=lc.WEIGHT) <= REL
    before = _counter("best_path_launches")
    pdfs, scores = (t.cpu().numpy() for t in sup.best_path(torch.from_numpy(np.array(y, copy=True)).to(DEV)))
    assert _counter("best_path_launches") == before + 1
    for s in range(2):
        ys = y[np.arange(T) * 2 + s]
        best, emitted = bp.best_score64(fsts[s], ys), bp.path_score64(fsts[s], ys, pdfs[s])
        eps = T * 2.0 ** -23 * bp.magnitude(fsts[s], ys)
        assert np.isfinite(best) and abs(scores[s] - emitted) <= eps and emitted >= best - 2 * eps, (s, scores[s], emitted, best)


# ---- bit for bit with the resident kernel ------------------------------------------------------------------------------------
def _forced(make, run, kernel_family):
    """``run(make())`` on the resident kernel and, on a fresh handle staged under the switch, on the large one."""
    large = _large()
    a = run(make())
    assert _large() == large  # (a handle that fits does not reach the large kernel on its own)
    kernel_family("force_num_e2e_large")
    b = run(make())
    assert _large() > large
    return a, b


@pytest.mark.parametrize("overlap", [True, False], ids=["staged", "in-line"])
@pytest.mark.parametrize("S,T", [(1, 1), (7, 37), (64, 150)])
@pytest.mark.parametrize("kind", ["chain", "random"])
def test_forced_large_kernel_gives_the_resident_kernels_bits(kind, S, T, overlap, kernel_family):
    """Loss, results, xent objective, gradient and xent gradient; and the same call twice gives the same bits."""
    if not overlap:
        kernel_family("no_num_overlap")
    # (the chain family's shortest path is up to 9 arcs: at T = 1, one word of one phone and no silence, one arc)
    kw = dict(words=1, max_phones=1, silence=False) if kind == "chain" and T < 12 else {}
    fsts = ref.batch(kind, S, P, seed=S * 1000 + T, **kw)
    assert all(ref.shortest_path_arcs(f) <= T for f in fsts)
    y, xe = _y(S, T, seed=S + T), _y(S, T, seed=S + T + 1, scale=1.0)
    staged = _counter("num_e2e_staged_launches")
    a, b = _forced(lambda: io.Supervision.from_e2e_fsts(0.7, T, P, fsts, any_size=True), lambda sup: _step(sup, y, xe)[0],
                   kernel_family)
    assert _counter("num_e2e_staged_launches") - staged == (2 if overlap else 0)
    assert np.isfinite(a[0]) and np.isfinite(a[2]) and a[2] != 0.0
    _same(a, b, "forced")
    sup = io.Supervision.from_e2e_fsts(0.7, T, P, fsts)
    large = _large()
    _same(_step(sup, y, xe)[0], b, "again, on a handle of the default entry")
    _same(_step(sup, y, xe)[0], b, "twice")
    assert _large() == large + 2


def test_forced_large_kernel_log_softmax_and_forward_only(kernel_family):
    S, T = 7, 37
    fsts = ref.batch("chain", S, P, seed=41)
    y, xe = _y(S, T, seed=42), _y(S, T, seed=43, scale=1.0)
    make = lambda: io.Supervision.from_e2e_fsts(0.7, T, P, fsts, any_size=True)  # noqa: E731

    def run(sup):
        soft = _step(sup, y, xe, xent_log_softmax=True)[0]
        before = _counter("num_backward_launches")
        ev = _step(sup, y, None, grad=False)[0]  # (no derivative, no xent: the forward recursion alone)
        assert _counter("num_backward_launches") == before
        return soft + ev

    a, b = _forced(make, run, kernel_family)
    _same(a, b, "log-softmax / forward only")
    plain = _step(make(), y, xe)[0]
    assert plain[2] != a[2]  # (the log-softmax route did run)


# ---- ragged ---------------------------------------------------------------------------------------------------------------
def test_ragged_batch_with_one_large_sequence(kernel_family):
    """Lengths (37, 1, 20, 5), the third sequence one state past the resident limit; NaN in the padding."""
    lens = (37, 1, 20, 5)
    S, T, w = len(lens), max(lens), 0.7
    small = ref.batch("random", S, P, seed=61)
    fsts = [small[0], small[1], lc.planted(lc.MAX_STATES + 1, 6000, P, P, seed=62), small[3]]
    clean = _y(S, T, seed=63)
    y = rc.with_padding(clean, np.asarray(lens), np.nan)
    sup = io.Supervision.from_e2e_fsts(w, list(lens), P, fsts, any_size=True)
    assert sup.is_ragged and sup.e2e_stats()["kernel"] == "large"
    large = _large()
    res, d, xd = _hip(sup, y)
    assert _large() == large + 1
    want = rc.ragged_objective(rc.oracle_graph(), fsts, lens, clean, weight=w, l2=lc.L2, leaky=lc.LEAKY)
    assert want["all_ok"]
    assert abs(res[0] - want["objf"]) <= REL * abs(want["objf"])
    pad = rc.padding_rows(lens)
    assert not _bits(d[pad]).any() and not _bits(xd[pad]).any()  # exactly +0
    assert rel_err(d[~pad], want["deriv"][~pad], floor=w) <= REL
    assert rel_err(xd[~pad], want["xent_deriv"][~pad], floor=w) <= REL
    # every sequence: the bits of the call on it alone (the one-workgroup denominator form a ragged batch takes)
    kernel_family("no_phase_split")
    for s, Ts in enumerate(lens):
        rows = rc.valid_rows(lens, s)
        large = _large()
        one = _hip(io.Supervision.from_e2e_fsts(w, Ts, P, [fsts[s]], any_size=True), clean[rows])
        assert _large() - large == (1 if s == 2 else 0)
        assert np.array_equal(_bits(d[rows]), _bits(one[1])), s
        assert np.array_equal(_bits(xd[rows]), _bits(one[2])), s


# ---- 16-bit inputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_inputs_equal_the_float32_path(dtype):
    """DESIGN 4.8 on a large handle: results, loss and xent objective of the (B, C, T) 16-bit call are those of the float32 call
    on ``out.float()``, and every gradient is that call's, rounded once."""
    S, T = 2, 20
    fsts = [lc.planted(lc.MAX_STATES + 1, 6000, P, P, seed=62), ref.random_fst(5, 12, P, np.random.default_rng(71))]
    sup = io.Supervision.from_e2e_fsts(0.9, T, P, fsts, any_size=True)

    def bct(m):
        return torch.from_numpy(m).to(DEV).to(dtype).view(T, S, P).permute(1, 2, 0).contiguous()

    x16, xe16 = bct(_y(S, T, seed=72)), bct(_y(S, T, seed=73, scale=1.0))
    kw = dict(l2_regularize=1e-4, leaky_hmm_coefficient=0.1, xent_regularize=0.1, kaldi_way=True)
    out = []
    large = _large()
    for conv in (lambda t: t.clone(), lambda t: t.float()):
        x, xx = conv(x16).requires_grad_(True), conv(xe16).requires_grad_(True)
        loss, res = chain_loss(x, _den(), sup, xent_input=xx, **kw)
        loss.backward()
        out.append((loss.detach(), res.data.clone(), res.xent_objf, x.grad, xx.grad))
    assert _large() == large + 2
    got, want = out
    assert got[0].dtype == dtype and torch.equal(got[0], want[0].to(dtype))
    assert torch.equal(got[1], want[1]) and got[2] == want[2] and got[2] != 0.0
    for g, wg in ((got[3], want[3]), (got[4], want[4])):
        assert g.dtype == dtype and torch.equal(g.view(torch.int16), wg.to(dtype).view(torch.int16))
        assert bool((g != 0).any())


# ---- failures -----------------------------------------------------------------------------------------------------------------
def test_an_infeasible_large_sequence():
    """Beside feasible ones: by default the whole minibatch takes the soft-failure route; with ``on_failure="sequence"`` only
    that sequence is failed, its rows are +0 and the others keep the bits of the healthy batch."""
    S, T, w, bad = 4, 20, 0.8, 2
    good = ref.batch("random", S, P, seed=81)
    healthy = good[:bad] + [lc.planted(lc.MAX_STATES + 1, 6000, P, P, seed=62)] + good[bad + 1:]
    broken = good[:bad] + [lc.no_path(lc.MAX_STATES + 1, 6000, P, seed=82)] + good[bad + 1:]
    y, xe = _y(S, T, seed=83), _y(S, T, seed=84, scale=1.0)
    large = _large()
    res, d, xd = _hip(io.Supervision.from_e2e_fsts(w, T, P, broken, any_size=True), y, l2=1e-3)
    assert _large() == large + 1
    assert res[0] == np.float32(-10.0 * w * S * T)
    np.testing.assert_allclose(d, -w * 1e-3 * y, rtol=1e-6, atol=0)
    assert not xd.any()
    (_, _, _, gb, gxb), rb = _step(io.Supervision.from_e2e_fsts(w, T, P, healthy, any_size=True), y, xe, per_sequence=True)
    assert rb.per_sequence.status.tolist() == [0] * S
    (loss, data, _, g, gx), r = _step(io.Supervision.from_e2e_fsts(w, T, P, broken, any_size=True), y, xe, on_failure="sequence")
    assert _large() == large + 3
    assert r.per_sequence.status.tolist() == [1 if s == bad else 0 for s in range(S)] and r.failed.tolist() == [bad]
    assert r.per_sequence.num_logprob[bad].item() == float("-inf")
    assert np.isfinite(loss) and np.isfinite(data).all()
    for a, b in ((g, gb), (gx, gxb)):
        a, b = a.reshape(T, S, P), b.reshape(T, S, P)
        for s in range(S):
            if s == bad:
                assert not _bits(a[:, s]).any()
            else:
                assert np.array_equal(_bits(a[:, s]), _bits(b[:, s])) and a[:, s].any()


# ---- best path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["states", "arcs", "pdfs", "limit"])
def test_best_path_on_large_handles(name):
    """The header's bound: the score is within T * 2^-23 * max(|y| + |cost|) of the emitted path's float64 score, and the
    emitted path within twice that of the best one.  A sequence without a path gets -inf and -1."""
    size, T, PL = lc.CASES[name]
    fsts = list(lc.fsts(name)) + [lc.no_path(lc.MAX_STATES + 1, 6000, PL, seed=91)]
    S = len(fsts)
    y = _y(S, T, P=PL, seed=92)
    sup = io.Supervision.from_e2e_fsts(1.0, T, PL, fsts, any_size=True)
    before = _counter("best_path_launches")
    pdfs, scores = sup.best_path(torch.from_numpy(y).to(DEV))
    torch.cuda.synchronize()
    assert _counter("best_path_launches") == before + 1
    pdfs, scores = pdfs.cpu().numpy(), scores.cpu().numpy()
    assert pdfs.shape == (S, T) and scores.shape == (S,)
    for s in range(S):
        ys = y[np.arange(T) * S + s]
        best = bp.best_score64(fsts[s], ys)
        if s == S - 1:
            assert best == -np.inf and scores[s] == -np.inf and (pdfs[s] == -1).all()
            continue
        assert np.isfinite(best) and (pdfs[s] >= 0).all()
        emitted = bp.path_score64(fsts[s], ys, pdfs[s])
        eps = T * 2.0 ** -23 * bp.magnitude(fsts[s], ys)
        print("%s seq %d: score %.17g emitted %.17g best %.17g eps %.3g" % (name, s, scores[s], emitted, best, eps))
        assert emitted > -np.inf
        assert abs(scores[s] - emitted) <= eps
        assert emitted >= best - 2 * eps


def test_training_step_is_the_same_after_best_path():
    name = "states"
    _, T, PL = lc.CASES[name]
    sup = io.Supervision.from_e2e_fsts(lc.WEIGHT, T, PL, list(lc.fsts(name)), any_size=True)
    y = lc.nnet_output(name)
    first = _hip(sup, y)
    sup.best_path(torch.from_numpy(_y(2, T, P=PL, seed=93)).to(DEV))
    large = _large()
    _same(first, _hip(sup, y), "after best_path")
    assert _large() == large + 1


# ---- composed with a denominator graph -----------------------------------------------------------------------------------------
def test_composed_acceptor_end_to_end():
    """The host test's acceptor, 60 states before and more than 2048 after ``den_graph=``: chain_loss + backward, an objective
    bounded by 0, and the float64 reference on the composed FST."""
    name, T = lc.COMPOSED_GRAPH, lc.COMPOSED_T
    fst = lc.composed_input()
    host = dc.graph(name)
    composed, info = host.normalize_fsts([fst], e2e=True)
    assert info["states_out"][0] > lc.MAX_STATES
    graph = io.DenominatorGraph(dc.den_fst(name), dc.P).prepare(DEV)
    sup = io.Supervision.from_e2e_fsts(1.0, T, dc.P, [fst], den_graph=graph, any_size=True)
    assert sup.e2e_stats()["kernel"] == "large"
    y = dc.nnet_output(7, lens=(T,), scale=2.0)
    x = torch.from_numpy(y).to(DEV).requires_grad_(True)
    large = _large()
    loss, res = chain_loss(x, graph, sup, dc.L2, dc.LEAKY)
    loss.backward()
    torch.cuda.synchronize()
    assert _large() == large + 1
    want = dc.reference(name, composed, (T,), y, e2e=True)
    objf = float(res.data[0])
    print("composed: objf %.9g (float64 %.9g)" % (objf, want["total"]))
    assert objf <= 0.0 and want["total"] <= 0.0
    assert abs(objf - want["total"]) <= REL * abs(want["total"])
    # (chain_loss's gradient is minus the objective's derivative, as tests/test_gpu_den_compose.py takes it)
    assert rel_err(-x.grad.cpu().numpy(), want["deriv"], floor=1.0) <= REL


# ---- warm calls -----------------------------------------------------------------------------------------------------------------
def test_warm_steps_on_a_large_handle_do_not_allocate():
    name = "arcs"
    _, T, PL = lc.CASES[name]
    y = lc.nnet_output(name)
    sup = io.Supervision.from_e2e_fsts(lc.WEIGHT, T, PL, list(lc.fsts(name)), any_size=True)
    first = _hip(sup, y)
    before, large = _counter("pool_device_allocs"), _large()
    _same(first, _hip(sup, y), "second step")
    assert _counter("pool_device_allocs") == before
    # and fresh handles of the same size every step take the slot this one gives back
    del sup
    for _ in range(2):
        _hip(io.Supervision.from_e2e_fsts(lc.WEIGHT, T, PL, list(lc.fsts(name)), any_size=True), y)
    assert _counter("pool_device_allocs") == before and _large() == large + 3
