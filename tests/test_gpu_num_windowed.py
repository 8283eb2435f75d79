"""The level-windowed numerator kernel (``csrc/num_windowed_kernels.hip``) on the GPU: regular supervisions whose sequences
do not fit the resident kernel's LDS (``tests/wide_supervisions.py``).

Two references.  The CPU oracle, under the project's matrix-wise ``REL``, on the supervisions that only the windowed kernel
can run; and the resident kernel, bit for bit, on supervisions that fit both (``tc_debug_set("force_num_windowed", 1)``): the
two kernels form every value through the same device functions in the same order.  Every case states its size through
``Supervision.stats()`` and asserts the kernel it expects, and the launch counter shows which kernel ran."""
import numpy as np
import pytest
import torch

from torchain_amd import io, parallel, synth
from torchain_amd._lib import lib
from torchain_amd.functions import ChainResults, chain_loss, compute_chain_objf_and_deriv

import wide_supervisions as ws
from helpers import REL, check_full, from3d, hip_chain, hip_num, rel_err, to3d

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = ws.P
FORMS = [("2d", torch.float32), ("3d", torch.float32), ("3d", torch.bfloat16), ("3d", torch.float16)]
FORM_IDS = ["2d-f32", "3d-f32", "3d-bf16", "3d-f16"]
XENT = [None, True, False]  # no cross-entropy branch, kaldi_way=True, kaldi_way=False
L2, LEAKY = 5e-5, 0.1
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
_cache = {}


def _windowed():
    return lib.tc_debug_counter(b"num_windowed_launches")


def _graph():
    if "graph" not in _cache:
        _cache["graph"] = io.DenominatorGraph(ws.den_fst(), P).prepare(DEV)
    return _cache["graph"]


def _sup(name, expect):
    """The case's handle; its size and the kernel it will take, stated and asserted."""
    if name not in _cache:
        _cache[name] = io.Supervision.from_synth(ws.supervision(name))
    st = _cache[name].stats()
    print(name, st)
    assert st["kernel"] == expect == ws.expected_kernel(name), st
    return _cache[name]


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    diff = a.detach().contiguous().view(_BITS[a.dtype]).cpu() != b.detach().contiguous().view(_BITS[b.dtype]).cpu()
    assert not bool(diff.any()), "%s: %d of %d elements differ" % (what, int(diff.sum()), diff.numel())


def _layout(y2d, S, T, layout, dtype):
    y = torch.as_tensor(y2d).to(DEV).to(dtype)
    if layout == "3d":
        return y.view(T, S, -1).permute(1, 2, 0).contiguous().requires_grad_(True)
    return y.clone().requires_grad_(True)


def _rows(g, S, T, layout):
    """A gradient in the caller's layout -> frame-major (T*S, P) float64 numpy."""
    g = g.detach().float()
    return (from3d(g, S, T, P) if layout == "3d" else g.cpu().numpy()).astype(np.float64)


def _run(x, xe, sup, xent, w=None, c=None, l2=L2):
    kw = dict(l2_regularize=l2, leaky_hmm_coefficient=LEAKY)
    if xent is not None:
        kw.update(xent_regularize=0.1, xent_input=xe, kaldi_way=xent)
    if w is not None:
        kw.update(deriv_weights=w)
    if c is not None:
        kw.update(out_of_range_regularize=c)
    loss, res = chain_loss(x, _graph(), sup, **kw)
    loss.sum().backward()
    return [loss.detach(), res.data.clone(), torch.tensor(float(res.xent_objf) if xent is not None else 0.0, dtype=torch.float64), x.grad,
            xe.grad if xent is not None else torch.zeros(1)]


def _weights(S, T, seed):
    pool = np.array([0.0, 1.0 / 255, 128.0 / 255, 1.0, 1.0, 1.0, 1.5, 3.25], np.float32)
    w = np.random.default_rng(seed).choice(pool, size=S * T)
    w[:len(pool)] = pool
    return torch.from_numpy(w.astype(np.float32))


def _check_against_oracle(oracle, sup, y, l2, leaky):
    """helpers.check_full's comparison, for a supervision that is given."""
    fst, S, T, weight = ws.den_fst(), sup.num_sequences, sup.frames_per_sequence, sup.weight
    ref = oracle.compute_chain_objf_and_deriv(oracle.DenGraph(fst), sup, y, l2, leaky, want_xent=True)
    out = hip_chain(fst, sup, y, l2=l2, leaky=leaky, xent=True, graph=_graph())
    res = out["results"]
    assert abs(res[0] - ref["objf"]) <= REL * abs(ref["objf"]), (res, ref["results"])
    assert abs(res[1] - ref["l2_term"]) <= REL * max(abs(ref["l2_term"]), 1e-30), (res, ref["results"])
    assert res[2] == ref["weight"] == np.float32(weight * S * T)
    assert rel_err(out["deriv"], ref["deriv"], floor=weight) <= REL
    assert rel_err(out["xent_deriv"], ref["xent_deriv"], floor=weight) <= REL
    return out, ref


# ---- 1. parity with the oracle on what the resident kernel refuses ------------------------------------------------------
@pytest.mark.parametrize("name", ws.WIDE)
def test_numerator_matches_the_oracle(oracle, name):
    """tc_num_forward_backward: log-prob and derivative, and the forward-only call (no history is written)."""
    _sup(name, ws.WINDOWED)
    sup, y = ws.supervision(name), ws.nnet_output(name)
    ref = oracle.num_forward_backward(sup, y)
    before = _windowed()
    out = hip_num(sup, y)
    fwd = hip_num(sup, y, want_deriv=False)
    assert _windowed() - before == 2
    err = rel_err(out["deriv"], ref["deriv"], floor=sup.weight)
    rows = out["deriv"].sum(axis=1, dtype=np.float64) / sup.weight
    print("%s: log-prob %.6f (oracle %.6f), deriv rel err %.3e, |row sum - 1| %.3e" % (
        name, out["logprob_weighted"], ref["logprob_weighted"], err, np.abs(rows - 1).max()))
    assert abs(out["logprob_weighted"] - ref["logprob_weighted"]) <= REL * abs(ref["logprob_weighted"])
    assert fwd["logprob_weighted"] == out["logprob_weighted"] and fwd["deriv"] is None
    assert err <= REL
    assert np.abs(rows - 1).max() <= 1e-4  # posteriors of a frame sum to one


def test_full_objective_trie_of_64_paths(oracle):
    """helpers.check_full itself, with paths=64 at T = 150: objf, l2 term, weight, derivative, xent derivative."""
    fst, S, T = ws.den_fst(), 2, 150
    g = oracle.DenGraph(fst)
    sup = synth.random_supervision(fst, S, T, 64, seed=5 + 2, weight=1.0, initial_probs=g.initial_probs())
    st = io.Supervision.from_synth(sup).stats()
    print(st)
    assert st["kernel"] == ws.WINDOWED and st["max_states"] > 9000
    before = _windowed()
    check_full(oracle, fst, S, T, l2=L2, leaky=LEAKY, paths=64)
    assert _windowed() - before == 1


@pytest.mark.parametrize("name", ["lattice_wide", "lattice_mixed", "lattice_pinch", "trie_600x16"])
def test_full_objective_matches_the_oracle(oracle, name):
    """The same comparison for lattice-like supervisions (in-arc lists longer than one, entries that sum many arcs; a
    weight other than 1 and distinct final weights), for a minibatch of one wide and three narrow sequences, and for a level
    of one state between wide ones."""
    _sup(name, ws.WINDOWED)
    before = _windowed()
    _check_against_oracle(oracle, ws.supervision(name), ws.nnet_output(name), L2, LEAKY)
    assert _windowed() - before == 1


# ---- 2. forced against resident, bit for bit ----------------------------------------------------------------------------
def _both(fn, kernel_family):
    """fn() on the resident kernel, then with the windowed kernel forced; the counter shows which ran."""
    kernel_family("force_num_windowed", 0)
    before = _windowed()
    a = fn()
    assert _windowed() == before
    kernel_family("force_num_windowed", 1)
    b = fn()
    assert _windowed() > before
    kernel_family("force_num_windowed", 0)
    return a, b


@pytest.mark.parametrize("name", ws.FITTING)
def test_forced_numerator_alone_gives_the_resident_bits(kernel_family, name):
    _sup(name, ws.RESIDENT)
    sup, y = ws.supervision(name), ws.nnet_output(name)
    for want_deriv in (True, False):
        a, b = _both(lambda: hip_num(sup, y, want_deriv=want_deriv), kernel_family)
        assert a["logprob_weighted"] == b["logprob_weighted"]
        if want_deriv:
            assert np.array_equal(a["deriv"].view(np.int32), b["deriv"].view(np.int32))


@pytest.mark.parametrize("serial", [0, 1], ids=["beside_den", "no_num_overlap"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", ws.FITTING)
def test_forced_chain_loss_gives_the_resident_bits(kernel_family, name, form, serial):
    """loss, results, xent objective, gradient, xent gradient; without the cross-entropy branch and with it both ways of
    kaldi_way; direct and beside the denominator."""
    hsup = _sup(name, ws.RESIDENT)
    sup, (layout, dtype) = ws.supervision(name), form
    S, T = sup.num_sequences, sup.frames_per_sequence
    y, xe = ws.nnet_output(name), ws.nnet_output(name, seed=6)
    kernel_family("no_num_overlap", serial)
    for xent in XENT:
        fn = lambda: _run(_layout(y, S, T, layout, dtype), _layout(xe, S, T, layout, dtype), hsup, xent)  # noqa: E731
        a, b = _both(fn, kernel_family)
        for u, v, what in zip(a, b, ("loss", "results", "xent objective", "grad", "xent grad")):
            _same_bits(u, v, "%s %s xent=%s: %s" % (name, form, xent, what))
        assert float(a[1][0]) != -10.0 * float(a[1][2])  # (not the soft failure: the gradients are the numerator's)


@pytest.mark.parametrize("form", [FORMS[0], FORMS[2]], ids=[FORM_IDS[0], FORM_IDS[2]])
@pytest.mark.parametrize("name", ws.FITTING)
def test_forced_with_the_options_gives_the_resident_bits(kernel_family, name, form):
    """deriv_weights, out_of_range_regularize, both, and torch.no_grad()."""
    hsup = _sup(name, ws.RESIDENT)
    sup, (layout, dtype) = ws.supervision(name), form
    S, T = sup.num_sequences, sup.frames_per_sequence
    y, xe = ws.nnet_output(name).copy(), ws.nnet_output(name, seed=6)
    y[::5, ::7] *= 12.0  # (some outputs beyond +-30)
    assert (np.abs(y) > 30).any()
    w = _weights(S, T, 3).to(DEV)
    for kw in (dict(w=w), dict(c=0.01), dict(w=w, c=0.25)):
        fn = lambda: _run(_layout(y, S, T, layout, dtype), _layout(xe, S, T, layout, dtype), hsup, True, **kw)  # noqa: E731
        a, b = _both(fn, kernel_family)
        for u, v, what in zip(a, b, ("loss", "results", "xent objective", "grad", "xent grad")):
            _same_bits(u, v, "%s %s %s: %s" % (name, form, sorted(kw), what))

    def evaluate():
        with torch.no_grad():
            loss, res = chain_loss(_layout(y, S, T, layout, dtype), _graph(), hsup, L2, LEAKY, 0.1,
                                   _layout(xe, S, T, layout, dtype), True)
        return loss, res.data.clone(), res.xent_objf

    a, b = _both(evaluate, kernel_family)
    _same_bits(a[0], b[0], "loss under no_grad")
    _same_bits(a[1], b[1], "results under no_grad")
    assert a[2] == b[2]


# ---- 3. chain_loss + backward on wide supervisions ------------------------------------------------------------------------
@pytest.mark.parametrize("xent", XENT, ids=["mmi", "kaldi_way", "xent"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", ["trie_150x64", "lattice_wide"])
def test_chain_loss_on_a_wide_supervision(oracle, name, form, xent):
    """Runs, equals itself bit for bit on a second run, and matches the oracle on the values the call saw: float32 within REL;
    a 16-bit call's gradient is the float32 call's on the widened values, rounded once."""
    hsup = _sup(name, ws.WINDOWED)
    sup, (layout, dtype) = ws.supervision(name), form
    S, T = sup.num_sequences, sup.frames_per_sequence
    y, xe = ws.nnet_output(name), ws.nnet_output(name, seed=6)
    before = _windowed()
    a = _run(_layout(y, S, T, layout, dtype), _layout(xe, S, T, layout, dtype), hsup, xent, l2=0.0)
    b = _run(_layout(y, S, T, layout, dtype), _layout(xe, S, T, layout, dtype), hsup, xent, l2=0.0)
    assert _windowed() - before == (4 if xent is False else 2)  # (kaldi_way=False runs the objective twice a call)
    for u, v, what in zip(a, b, ("loss", "results", "xent objective", "grad", "xent grad")):
        _same_bits(u, v, "second run: " + what)
    seen = torch.as_tensor(y).to(dtype).float()  # (what the call saw)
    seen_xe = torch.as_tensor(xe).to(dtype).float()
    on = seen_xe if xent is False else seen  # (kaldi_way=False: the objective is run again on the cross-entropy output)
    ref = oracle.compute_chain_objf_and_deriv(oracle.DenGraph(ws.den_fst()), sup, on.numpy(), 0.0, LEAKY, want_xent=True)
    res = a[1].numpy()
    assert abs(res[0] - ref["objf"]) <= REL * abs(ref["objf"]) and res[2] == ref["weight"]
    if dtype == torch.float32:
        assert rel_err(-_rows(a[3], S, T, layout), ref["deriv"], floor=sup.weight) <= REL
        if xent is not None:
            assert rel_err(-_rows(a[4], S, T, layout) / 0.1, ref["xent_deriv"], floor=sup.weight) <= REL
    else:
        f = _run(_layout(seen, S, T, layout, torch.float32), _layout(seen_xe, S, T, layout, torch.float32), hsup, xent, l2=0.0)
        _same_bits(a[3], f[3].to(dtype), "grad against the float32 call's, rounded once")


# ---- 5. soft failure --------------------------------------------------------------------------------------------------------
def test_numerical_failure_is_soft_on_a_wide_supervision():
    """After test_numerical_failure_is_soft (tests/test_gpu_objective.py): a NaN output makes the denominator fail; the call
    returns -10 * weight, a zero derivative (l2 = 0) and a zero xent derivative, whatever the windowed kernel had added."""
    name = "lattice_wide"
    _sup(name, ws.WINDOWED)
    sup, y = ws.supervision(name), ws.nnet_output(name).copy()
    S, T = sup.num_sequences, sup.frames_per_sequence
    y[3, 5] = np.nan
    before = _windowed()
    out = hip_chain(ws.den_fst(), sup, y, l2=0.0, leaky=1e-5, xent=True, graph=_graph())
    assert _windowed() - before == 1
    assert out["results"][0] == np.float32(-10.0 * sup.weight * S * T)
    assert out["results"][2] == np.float32(sup.weight * S * T)
    assert np.all(out["deriv"][np.isfinite(y)] == 0) and np.all(out["xent_deriv"] == 0)


# ---- 6. the pool ------------------------------------------------------------------------------------------------------------
def test_fresh_wide_supervision_every_step_allocates_nothing_after_warmup(oracle):
    """After test_fresh_supervision_every_step_allocates_nothing_after_warmup: the history lives in the supervision's pool
    slot, so a new wide supervision every step stops allocating once the pool is warm."""
    fst, S, T = ws.den_fst(), 2, 150
    g = oracle.DenGraph(fst)
    sups = [synth.random_supervision(fst, S, T, 64, seed=62 + i, initial_probs=g.initial_probs()) for i in range(3)]
    y_np = synth.random_nnet_output(S, T, P, seed=63)
    refs = [oracle.compute_chain_objf_and_deriv(g, sp, y_np, 0.0, 0.1)["objf"] for sp in sups]
    y = torch.from_numpy(y_np).to(DEV)
    deriv = torch.empty_like(y)
    allocs, objfs = [], []
    before = _windowed()
    for step in range(30):
        h = io.Supervision.from_synth(sups[step % 3])
        if step == 0:
            assert h.stats()["kernel"] == ws.WINDOWED
        res = ChainResults()
        compute_chain_objf_and_deriv(_graph(), h, y, res.data, deriv, None, 0.0, 0.1, 0.0)
        objfs.append(float(res.data[0]))
        del h
        allocs.append(lib.tc_debug_counter(b"pool_device_allocs"))
    assert _windowed() - before == 30
    assert allocs[-1] == allocs[9], allocs  # nothing allocated after the first ten steps
    for step, v in enumerate(objfs):
        assert abs(v - refs[step % 3]) <= REL * abs(refs[step % 3])


# ---- 7. readers and shards --------------------------------------------------------------------------------------------------
def test_wide_supervision_through_the_egs_reader(oracle, tmp_path):
    """Two one-sequence wide lattices written as Kaldi chain egs, read back and merged by io.RandExample: the merged supervision
    takes the windowed kernel and chain_loss matches the oracle on the merged FST."""
    import kaldi_egs_writer as kw
    from fixtures import make_example

    fst, T = ws.den_fst(), 150
    keyed = []
    for i in range(2):
        eg = make_example(fst, T, seed=40 + i)
        eg["outputs"][0]["supervision"] = ws.lattice_supervision(1, T, P, lambda q, t, r: r.integers(40, 121), 3, seed=50 + i,
                                                                 final_weights=True)
        keyed.append(("wide%02d" % i, eg))
    ark, scp = str(tmp_path / "egs.ark"), str(tmp_path / "egs.scp")
    kw.write_ark(ark, keyed, scp_path=scp)
    rd = io.RandExample(scp, seed=1, batchsize=2)
    n = 0
    for (mfcc, ivec), sup in rd:
        B, T_, P_ = sup.shape
        st = sup.stats()
        print(st)
        assert (B, T_, P_) == (2, T, P) and st["kernel"] == ws.WINDOWED
        merged = rd._cur["outputs"][0]["supervision"]
        y = synth.random_nnet_output(B, T, P, seed=90)
        ref = oracle.compute_chain_objf_and_deriv(oracle.DenGraph(fst), merged, y, 1e-4, 0.1)
        x = to3d(y, B, T, P).requires_grad_(True)
        before = _windowed()
        loss, res = chain_loss(x, _graph(), sup, l2_regularize=1e-4, leaky_hmm_coefficient=0.1)
        loss.backward()
        assert _windowed() - before == 1
        assert abs(float(res.data[0]) - ref["objf"]) <= REL * abs(ref["objf"])
        assert rel_err(from3d(x.grad, B, T, P), -ref["deriv"], floor=1.0) <= REL
        n += 1
    assert n == 1


def test_shards_of_a_wide_supervision_sum_to_the_whole():
    """parallel.shard_supervision_fst (one boundary state between sequences: the lattices end in one state): each shard is
    wide itself, and the shards' objectives and gradients are the unsharded call's."""
    S, T = 4, 150
    sup = ws.lattice_supervision(S, T, P, lambda q, t, r: 1 if t == T else r.integers(40, 121), 3, seed=9)
    y = synth.random_nnet_output(S, T, P, seed=10)
    whole = io.Supervision.from_synth(sup)
    assert whole.stats()["kernel"] == ws.WINDOWED
    x = to3d(y, S, T, P).requires_grad_(True)
    loss, res = chain_loss(x, _graph(), whole, 0.0, LEAKY)
    loss.backward()
    want_objf, want_grad = float(res.data[0]), from3d(x.grad, S, T, P)
    objf = 0.0
    for rank in range(2):
        lo, hi = parallel.shard_range(S, rank, 2)
        part = io.Supervision.from_synth(parallel.shard_supervision_fst(sup, lo, hi))
        assert part.stats()["kernel"] == ws.WINDOWED and part.n_batch == hi - lo
        y_local = np.ascontiguousarray(parallel.shard_rows(torch.from_numpy(y), S, lo, hi).numpy())
        xl = to3d(y_local, hi - lo, T, P).requires_grad_(True)
        before = _windowed()
        l_, r_ = chain_loss(xl, _graph(), part, 0.0, LEAKY)
        l_.backward()
        assert _windowed() - before == 1
        objf += float(r_.data[0])
        g = parallel.shard_rows(torch.from_numpy(want_grad), S, lo, hi).numpy()
        assert rel_err(from3d(xl.grad, hi - lo, T, P), g, floor=1.0) <= REL
    assert abs(objf - want_objf) <= REL * abs(want_objf)


# ---- 8. stream capture ------------------------------------------------------------------------------------------------------
def test_training_step_with_a_wide_supervision_replays_from_a_captured_graph():
    """After test_training_step_replays_from_a_captured_graph (tests/test_gpu_step.py): chain_loss with the xent branch + the
    backward on a wide supervision, captured once and replayed on new activations: loss and both gradients bit-identical to the
    direct call's."""
    name = "trie_150x64"
    hsup = _sup(name, ws.WINDOWED)
    sup = ws.supervision(name)
    S, T = sup.num_sequences, sup.frames_per_sequence
    kw = dict(l2_regularize=5e-5, leaky_hmm_coefficient=LEAKY, xent_regularize=0.1, kaldi_way=True)
    x = to3d(ws.nnet_output(name), S, T, P).clone().requires_grad_(True)
    xe = (0.5 * x.detach()).clone().requires_grad_(True)

    def step():
        loss, results = chain_loss(x, _graph(), hsup, xent_input=xe, **kw)
        g, gx = torch.autograd.grad(loss, (x, xe))
        return loss.detach(), g, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()  # warm-up outside the capture: tables, pools, side streams
    side.synchronize()
    before = _windowed()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        captured = step()
    assert _windowed() - before == 1  # (captured, not run)
    for seed in (21, 22):
        fresh = torch.randn(x.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
        with torch.no_grad():
            x.copy_(fresh)
            xe.copy_(0.25 * fresh)
        before = _windowed()
        cg.replay()
        torch.cuda.synchronize()
        assert _windowed() == before  # no library call: the graph's own nodes ran
        got = [t.clone() for t in captured]
        want = step()
        torch.cuda.synchronize()
        for g, w_, what in zip(got, want, ("loss", "grad", "xent grad")):
            _same_bits(g, w_, what + " after replay")
    torch.cuda.synchronize()
