"""``chain_loss(..., per_sequence=True, on_failure="sequence")`` on the GPU (``tc_chain_step_per_sequence``; cases
and the host restatement: ``tests/per_sequence_cases.py``).

1 the report against the oracle on each sequence alone, ``results.data`` reproduced bitwise from it, everything else
untouched; 2 the switch on with nothing failing, bit for bit the default call in every layout, dtype and option; 3 an
end-to-end sequence without a path; 4 NaN / +inf activations in one sequence through every denominator family and numerator
kernel; 5 non-finite values in padding frames only; 6 every sequence failed; 7 the evaluation step; 8 a captured step replayed
on inputs that fail different sequences; 9 ``chain_loss_data_parallel`` with a failed sequence on one rank.

Tolerance of the comparisons with the oracle: ``helpers.REL`` (1e-4 relative), what the existing per-batch log-prob and
objective comparisons use.  Everything else is compared bit for bit; a float16 gradient in case 2 up to the sign of an exactly
zero element, the allowance DESIGN 4.11 makes for the default route."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from torchain_amd import io
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss

import per_sequence_cases as ps
import ragged_cases as rc
import row_contract_cases as rcc
from helpers import REL, free_port

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAYOUTS = ("rows", "time_major", "bct", "batch_first")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_dtype_id = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


def _counter(name):
    return int(lib.tc_debug_counter(name.encode()))


@pytest.fixture(autouse=True)
def _fixed_kernel_choice(kernel_family):
    kernel_family("no_tune")  # (no timing launches: the graphs of this module take the kernel their switches name)


_graphs = {}


def _graph(build=()):
    """The module's denominator graph, once per set of build-time switches (set by the caller's ``kernel_family``)."""
    if build not in _graphs:
        _graphs[build] = io.DenominatorGraph(ps.den_fst(), ps.P)
    return _graphs[build].prepare(0)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int16))


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _as_layout(y2d, S, T, layout, dtype):
    """The (T * S, P) matrix as chain_loss input of the layout; returns (tensor, function: its gradient -> (T, S, P))."""
    t = torch.from_numpy(np.ascontiguousarray(y2d)).to(DEV).view(T, S, -1)
    if layout == "rows":
        return t.reshape(T * S, -1).to(dtype), lambda g: g.view(T, S, -1)
    if layout == "bct":
        return t.permute(1, 2, 0).contiguous().to(dtype), lambda g: g.permute(2, 0, 1)
    if layout == "batch_first":
        return t.permute(1, 0, 2).contiguous().to(dtype).permute(0, 2, 1), lambda g: g.permute(2, 0, 1)
    assert layout == "time_major"
    return t.contiguous().to(dtype).permute(1, 2, 0), lambda g: g.permute(2, 0, 1)


Out = namedtuple("Out", "loss data xent g gx seq failed results")


def _step(y, sup, graph, S, T, layout="rows", dtype=torch.float32, xent=True, kaldi_way=True, dw=None, oor=0.0, grad=True, **opts):
    """One chain_loss step; the gradients come back as (T, S, P) tensors of the input's dtype."""
    y = np.array(y, np.float32)  # (a copy: the cases' arrays are read-only)
    x, back = _as_layout(y, S, T, layout, dtype)
    xx, _ = _as_layout((0.5 * y).astype(np.float32), S, T, layout, dtype)
    kw = dict(l2_regularize=ps.L2, leaky_hmm_coefficient=ps.LEAKY)
    if xent:
        kw.update(xent_regularize=ps.XREG, kaldi_way=kaldi_way)
    if dw is not None:
        kw["deriv_weights"] = torch.from_numpy(dw).to(DEV)
    if oor:
        kw["out_of_range_regularize"] = oor
    kw.update(opts)
    if not grad:
        with torch.no_grad():
            loss, res = chain_loss(x, graph, sup, xent_input=xx if xent else None, **kw)
        torch.cuda.synchronize()
        return Out(loss.clone(), res.data.clone(), res.xent_objf, None, None, res.per_sequence, res.failed, res)
    x.requires_grad_(True)
    xx.requires_grad_(True)
    loss, res = chain_loss(x, graph, sup, xent_input=xx if xent else None, **kw)
    grads = torch.autograd.grad(loss, (x, xx) if xent else (x,))
    torch.cuda.synchronize()
    return Out(loss.detach().clone(), res.data.clone(), res.xent_objf, back(grads[0]).contiguous(),
               back(grads[1]).contiguous() if xent else None, res.per_sequence, res.failed, res)


def _dims(name):
    lens = ps.lengths(name)
    return len(lens), max(lens)


def _same_outputs(a, b, f16_zero_sign=False):
    """loss, results, xent objective and both gradients bit for bit (a float16 gradient: in value)"""
    assert _same(a.loss, b.loss) and _same(a.data, b.data), (a.loss, b.loss, a.data, b.data)
    assert a.xent == b.xent or (a.xent != a.xent and b.xent != b.xent)
    for ga, gb in ((a.g, b.g), (a.gx, b.gx)):
        assert (ga is None) == (gb is None)
        if ga is None:
            continue
        if f16_zero_sign and ga.dtype == torch.float16:
            assert torch.equal(ga, gb)
        else:
            assert _same(ga, gb)


def _scale(out_xent_regularize=ps.XREG):
    return 1.0 / -float(out_xent_regularize)


# ---- 1. reporting ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ps.HEALTHY)
def test_report(name):
    S, T = _dims(name)
    lens = np.asarray(ps.lengths(name))
    y = rc.with_padding(ps.nnet_output(name), lens, np.nan)
    graph = _graph()
    plain = _step(y, ps.handle(name), graph, S, T)
    got = _step(y, ps.handle(name), graph, S, T, per_sequence=True)
    assert plain.seq is None and plain.failed is None
    seq = got.seq
    want = ps.oracle_rows(name)
    for s in range(S):
        print("%s seq %d: num %.9g (oracle %.9g) den %.9g (%.9g)" % (name, s, seq.num_logprob[s], want[s, 0], seq.den_logprob[s],
                                                                     want[s, 1]))
    assert (np.abs(seq.num_logprob.numpy() - want[:, 0]) <= REL * np.abs(want[:, 0])).all()
    assert (np.abs(seq.den_logprob.numpy() - want[:, 1]) <= REL * np.abs(want[:, 1])).all()
    assert (np.abs(seq.sum_y2.numpy() - want[:, 2]) <= REL * want[:, 2]).all()
    assert seq.frames.tolist() == [float(n) for n in lens] and seq.status.tolist() == [0] * S and got.failed.numel() == 0
    w32 = float(np.float32(ps.WEIGHT))  # (the handle's weight is a float32)
    assert np.array_equal(seq.objf.numpy(), w32 * (seq.num_logprob.numpy() - seq.den_logprob.numpy()))
    # results.data, the loss and the xent objective bitwise from the report
    re = ps.finalize_from(seq, ps.WEIGHT, ps.L2, T, not ps.uniform(name), isolate=False)
    assert re["results"].tobytes() == got.data.numpy().tobytes(), (re["results"], got.data)
    assert np.float32(re["loss"]).tobytes() == got.loss.cpu().numpy().tobytes()
    assert got.xent == re["xent"] * _scale()
    # everything else: the call without the keyword
    _same_outputs(got, plain)


# ---- 2. the switch on, nothing failing ------------------------------------------------------------------------------------------
MODES = ("plain", "xent_kaldi", "xent_reference", "weights_and_penalty")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dtype_id.get)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["reg_uniform", "e2e_ragged"])
def test_nothing_failed_is_the_default_call(name, layout, dtype, mode):
    S, T = _dims(name)
    lens = np.asarray(ps.lengths(name))
    y = np.array(ps.nnet_output(name), copy=True)
    kw = dict(xent=mode != "plain", kaldi_way=mode != "xent_reference")
    if mode == "weights_and_penalty":
        y[0 * S + 0, 3], y[1 * S + (S - 1), 7] = 33.0, -35.0  # valid frames beyond +-30
        kw.update(dw=np.random.default_rng(9).uniform(0.0, 2.0, size=T * S).astype(np.float32), oor=0.01)
    y = rc.with_padding(y, lens, 40.0)
    graph = _graph()
    off = _step(y, ps.handle(name), graph, S, T, layout, dtype, **kw)
    on = _step(y, ps.handle(name), graph, S, T, layout, dtype, on_failure="sequence", **kw)
    assert on.seq.status.tolist() == [0] * S and on.failed.numel() == 0
    assert bool(torch.isfinite(off.data).all()) and float(off.data[0]) != -10.0 * float(off.data[2])
    _same_outputs(on, off, f16_zero_sign=True)


# ---- 3. an end-to-end sequence without a path -----------------------------------------------------------------------------------
def _check_isolated(iso, run_b, bad, lens, T, ragged, what, strict=True, weight=ps.WEIGHT):
    """The isolating run against run B (the healthy batch): statuses, the failed sequences' rows all-zero bit patterns, the
    survivors' rows and per-sequence values run B's bits, the scalars the host restatement of run B's report with the failed
    sequences masked out.  ``strict`` False (a family DESIGN 4.13 lists as not isolating strictly): whichever sequences are
    reported ok hold finite values equal to run B's, and at least the broken one is reported."""
    S = len(lens)
    status = iso.seq.status.tolist()
    failed = [s for s in range(S) if status[s] != 0]
    print("%s: status %s results %s loss %s" % (what, status, iso.data.tolist(), iso.loss.tolist()))
    assert bad in failed, (what, status)
    if strict:
        assert failed == [bad], (what, status)
    assert 0 < len(failed) < S and iso.failed.tolist() == failed
    for g, gb in ((iso.g, run_b.g), (iso.gx, run_b.gx)):
        if g is None:
            continue
        for s in range(S):
            if s in failed:
                assert not _bits(g[:, s]).any(), (what, "rows of failed sequence", s)
            else:
                assert _same(g[:, s], gb[:, s]), (what, "rows of surviving sequence", s)
                assert bool(torch.isfinite(g[:lens[s], s].float()).all())
    alive = [s for s in range(S) if s not in failed]
    for field in ("num_logprob", "den_logprob", "sum_y2", "xent_sum", "frames"):
        a, b = getattr(iso.seq, field), getattr(run_b.seq, field)
        assert _same(a[alive], b[alive]) and bool(torch.isfinite(a[alive]).all()), (what, field)
    re = ps.finalize_from(run_b.seq, weight, ps.L2, T, ragged, isolate=True, mask=failed)
    assert re["masked"] and re["fail"] == 0
    assert re["results"].tobytes() == iso.data.numpy().tobytes(), (what, re["results"], iso.data)
    assert np.isfinite(float(iso.loss)) and _same(iso.loss.cpu(), torch.tensor([re["loss"]]).to(iso.loss.dtype))
    if iso.xent is not None:
        assert iso.xent == re["xent"] * _scale()


@pytest.mark.parametrize("dtype", DTYPES, ids=_dtype_id.get)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_end_to_end_sequence_without_a_path(layout, dtype):
    name = "e2e_ragged"
    S, T = _dims(name)
    lens = ps.lengths(name)
    bad = ps.BAD[name]
    y = rc.with_padding(ps.nnet_output(name), np.asarray(lens), np.nan)
    graph = _graph()
    broken = {bad: ps.no_path_fst(lens[bad])}
    # today's behaviour, pinned: the whole minibatch fails
    default = _step(y, ps.handle(name, broken), graph, S, T, layout, dtype)
    w_all = np.float32(ps.WEIGHT) * np.float32(sum(lens))
    assert default.data[0].item() == np.float32(-10.0) * w_all and default.data[2].item() == w_all
    assert abs(float(default.loss) - 10.0) <= 1e-5
    assert not _bits(default.gx).any() and default.xent == 0.0
    valid = torch.from_numpy(~rc.padding_rows(lens)).view(T, S).to(DEV)
    assert bool((default.g.float()[valid] != 0).any()) and not _bits(default.g[~valid]).any()
    # run B: the same batch with a good FST in its place
    run_b = _step(y, ps.handle(name), graph, S, T, layout, dtype, per_sequence=True)
    iso = _step(y, ps.handle(name, broken), graph, S, T, layout, dtype, on_failure="sequence")
    assert iso.seq.status.tolist() == [1 if s == bad else 0 for s in range(S)]
    assert iso.seq.num_logprob[bad].item() == float("-inf")
    _check_isolated(iso, run_b, bad, lens, T, True, "%s %s %s" % (name, layout, dtype))


# ---- 4. non-finite activations in one sequence: every denominator family, every numerator kernel --------------------------------
Inputs = namedtuple("Inputs", "key S T lens ragged handle y carried uncarried bad weight")


def _case_inputs(name):
    S, T = _dims(name)
    bad = ps.BAD[name]
    return Inputs(name, S, T, ps.lengths(name), not ps.uniform(name), lambda: ps.handle(name), ps.nnet_output(name),
                  ps.carried_pdf(name, bad), ps.uncarried_pdf(name, bad), bad, ps.WEIGHT)


def _planes_inputs():
    """The plane-wise kernel at the smallest graph its tests use (``row_contract_cases``: 17000 states, 3 x 7)."""
    fam = rcc.BY_NAME["planes_fused"]
    S, T, bad = fam.S, fam.T, 1
    sup = rcc.supervision(fam.graph, S, T)
    mask = rcc.carried(sup).reshape(T, S, -1)
    carried = int(np.flatnonzero(mask[1, bad])[0])
    uncarried = int(np.flatnonzero(~mask[:, bad].any(axis=0))[0])
    return Inputs("planes", S, T, (T,) * S, False, lambda: io.Supervision.from_synth(sup), rcc.nnet_output(fam.graph, S, T),
                  (1, carried), uncarried, bad, float(sup.weight))


# id -> (inputs, build-time switches, launch-time switches, stats()["tied"], counter that must move, strict isolation)
FAMILIES = {
    "fused_ragged": ("reg_ragged", (), ("no_phase_split",), 1, None, True),
    "fused_uniform_e2e": ("e2e_uniform", (), ("no_phase_split",), 1, None, True),
    "pair": ("reg_uniform", (), ("force_pair",), 1, None, True),
    "two_cu_ragged8": ("reg_ragged8", (), (), 1, "ragged_two_cu_launches", True),
    "two_cu_ragged8_e2e": ("e2e_ragged8", (), (), 1, "ragged_two_cu_launches", True),
    "mitm_uniform8": ("e2e_uniform8", (), ("force_mitm",), 1, None, True),
    "two_pass_uniform8": ("reg_uniform8", (), ("no_mitm",), 1, None, True),
    "general_ragged": ("reg_ragged", ("force_general",), (), 0, None, True),
    "general_uniform_e2e": ("e2e_uniform", ("force_general",), (), 0, None, True),
    "streamed": ("reg_uniform", ("force_streamed", "slab_narrow"), (), 2, None, True),
    "planes_fused": ("planes", (), ("no_phase_split",), 1, None, True),
    "planes_two_cu": ("planes", (), (), 1, None, True),
    "num_windowed_ragged": ("reg_ragged", (), ("no_phase_split", "force_num_windowed"), 1, "num_windowed_launches", True),
    "num_windowed_uniform": ("reg_uniform", (), ("no_phase_split", "force_num_windowed"), 1, "num_windowed_launches", True),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_non_finite_activations_in_one_sequence(family, kernel_family):
    key, build, launch, tied, counter, strict = FAMILIES[family]
    for switch in build + launch:
        kernel_family(switch)
    inp = _planes_inputs() if key == "planes" else _case_inputs(key)
    graph = rcc.den_graph(rcc.BY_NAME["planes_fused" if "no_phase_split" in launch else "planes_two_cu"], kernel_family).prepare(0) \
        if key == "planes" else _graph(build)
    assert graph.stats()["tied"] == tied
    S, T, bad = inp.S, inp.T, inp.bad
    clean = rc.with_padding(inp.y, np.asarray(inp.lens), np.nan) if inp.ragged else np.array(inp.y, copy=True)
    before = _counter(counter) if counter else 0
    run_b = _step(clean, inp.handle(), graph, S, T, per_sequence=True)
    if counter:
        assert _counter(counter) > before, counter
    assert run_b.seq.status.tolist() == [0] * S
    t, pdf = inp.carried
    for value in (np.nan, np.inf):
        for where, column in (("carried", pdf), ("uncarried", inp.uncarried)):
            y = np.array(clean, copy=True)
            assert t < inp.lens[bad]
            y[t * S + bad, column] = value
            iso = _step(y, inp.handle(), graph, S, T, on_failure="sequence")
            what = "%s %s %s %s" % (inp.key, family, value, where)
            assert iso.seq.status[bad].item() & 2, (what, iso.seq.status.tolist())  # the denominator reads every column
            _check_isolated(iso, run_b, bad, inp.lens, T, inp.ragged, what, strict=strict, weight=inp.weight)


# ---- 5. non-finite values in padding frames only ---------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("name", ["reg_ragged", "e2e_ragged", "reg_ragged8"])
def test_padding_values_fail_nothing(name, value):
    S, T = _dims(name)
    lens = np.asarray(ps.lengths(name))
    graph = _graph()
    clean = _step(ps.nnet_output(name), ps.handle(name), graph, S, T, on_failure="sequence")
    dirty = _step(rc.with_padding(ps.nnet_output(name), lens, value), ps.handle(name), graph, S, T, on_failure="sequence")
    assert dirty.seq.status.tolist() == [0] * S and clean.seq.status.tolist() == [0] * S
    _same_outputs(dirty, clean)
    for field in ("num_logprob", "den_logprob", "sum_y2", "xent_sum", "frames"):
        assert _same(getattr(dirty.seq, field), getattr(clean.seq, field)), field


# ---- 6. every sequence failed ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype", [("rows", torch.float32), ("bct", torch.bfloat16), ("batch_first", torch.float16)])
@pytest.mark.parametrize("name", ["reg_uniform", "e2e_ragged"])
def test_every_sequence_failed_is_the_default_route(name, layout, dtype):
    """(Survivors that miss the alpha-beta sum check while each of their own values is finite cannot be built from inputs:
    that route is covered by the host restatement's special cases.)"""
    S, T = _dims(name)
    y = rc.with_padding(ps.nnet_output(name), np.asarray(ps.lengths(name)), 1.0)
    for s in range(S):
        y[0 * S + s, 5 + s] = np.nan
    graph = _graph()
    off = _step(y, ps.handle(name), graph, S, T, layout, dtype)
    on = _step(y, ps.handle(name), graph, S, T, layout, dtype, on_failure="sequence")
    assert all(st != 0 for st in on.seq.status.tolist()) and on.failed.tolist() == list(range(S))
    assert off.data[0].item() == np.float32(-10.0) * off.data[2].item() and abs(float(off.loss) - 10.0) <= 0.1
    _same_outputs(on, off)


# ---- 7. the evaluation step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["e2e_ragged", "reg_ragged"])
def test_evaluation_step(name):
    S, T = _dims(name)
    lens = ps.lengths(name)
    bad = ps.BAD[name]
    y = rc.with_padding(ps.nnet_output(name), np.asarray(lens), np.nan)
    t, pdf = ps.carried_pdf(name, bad)
    y[t * S + bad, pdf] = np.inf
    graph = _graph()
    train = _step(y, ps.handle(name), graph, S, T, xent=False, on_failure="sequence")
    _step(y, ps.handle(name), graph, S, T, xent=False, grad=False, on_failure="sequence")  # (warm: workspace, tables)
    keys = ("den_backward_launches", "num_backward_launches", "layout_launches")
    before = [_counter(k) for k in keys]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    ev = _step(y, ps.handle(name), graph, S, T, xent=False, grad=False, on_failure="sequence")
    peak = torch.cuda.max_memory_allocated() - held
    assert [_counter(k) for k in keys] == before  # forward recursions only, nothing moved or zeroed
    # no gradient tensor: the step's own allocations are the inputs, the 24-byte outputs and the report
    inputs = 2 * S * T * ps.P * 4
    assert peak < inputs + S * T * ps.P * 4, (peak, inputs)
    assert ev.g is None and not ev.loss.requires_grad
    assert [s for s in range(S) if ev.seq.status[s].item() != 0] == [bad] == ev.failed.tolist()
    print("%s: training %s loss %s, evaluation %s loss %s" % (name, train.data.tolist(), train.loss.tolist(), ev.data.tolist(),
                                                             ev.loss.tolist()))
    assert _same(ev.data, train.data) and _same(ev.loss, train.loss)
    assert np.isfinite(float(ev.loss)) and float(ev.data[2]) == np.float32(ps.WEIGHT) * np.float32(sum(lens) - lens[bad])


# ---- 8. stream capture ------------------------------------------------------------------------------------------------------------
def test_captured_step_follows_the_input():
    name = "e2e_ragged"
    S, T = _dims(name)
    lens = ps.lengths(name)
    graph, sup = _graph(), ps.handle(name)
    clean = torch.from_numpy(rc.with_padding(ps.nnet_output(name), np.asarray(lens), 0.0)).to(DEV)
    x = clean.clone().requires_grad_(True)
    xe = (0.5 * clean).clone().requires_grad_(True)
    kw = dict(l2_regularize=ps.L2, leaky_hmm_coefficient=ps.LEAKY, xent_regularize=ps.XREG, kaldi_way=True, on_failure="sequence")
    seen = []

    def step():
        loss, results = chain_loss(x, graph, sup, xent_input=xe, **kw)
        g, gx = torch.autograd.grad(loss, (x, xe))
        seen.append(results)
        return loss.detach(), g, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    side.synchronize()
    before = _counter("den_launches")
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        captured = step()
    assert _counter("den_launches") == before + 1  # (captured, not run)
    results = seen[-1]
    for fails in (1, 3):
        t, pdf = ps.carried_pdf(name, fails)
        with torch.no_grad():
            x.copy_(clean)
            xe.copy_(0.5 * clean)
            x[t * S + fails, pdf] = float("nan")
        cg.replay()
        torch.cuda.synchronize()
        results.invalidate()
        got = [c.clone() for c in captured]
        got_data, got_xent = results.data.clone(), results.xent_objf
        status = results.per_sequence.status.tolist()
        assert [s for s in range(S) if status[s] != 0] == [fails] == results.failed.tolist(), status
        want = step()  # the direct call on the same input
        torch.cuda.synchronize()
        assert _same(got_data, seen[-1].data) and got_xent == seen[-1].xent_objf
        assert seen[-1].per_sequence.status.tolist() == status
        for a, b in zip(got, want):
            assert _same(a, b)
        for g in got[1:]:
            rows = g.view(T, S, -1)
            assert not _bits(rows[:, fails]).any()
            assert all(bool((rows[:lens[s], s] != 0).any()) for s in range(S) if s != fails)
        assert bool(torch.isfinite(got[0]).all()) and np.isfinite(got_data.numpy()).all()


# ---- 9. data parallel -------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out_dir):
    """One rank of two on the one device: its shard of ``e2e_ragged`` (the broken sequence is on rank 0) through a small
    model under DistributedDataParallel and ``chain_loss_data_parallel`` with isolation; and, for the test, the same shard
    through ``chain_loss`` alone."""
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel

    from torchain_amd import parallel

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        name = "e2e_ragged"
        lens = ps.lengths(name)
        S = len(lens)
        bad = ps.BAD[name]
        lo, hi = parallel.shard_range(S, rank, world)
        mine = list(range(lo, hi))
        fsts = [ps.no_path_fst(lens[s]) if s == bad else ps.pieces(name)[s] for s in mine]
        my_lens = np.asarray([lens[s] for s in mine], np.int32)
        Tm = int(my_lens.max())
        y = ps.nnet_output(name).reshape(max(lens), S, ps.P)[:Tm, lo:hi]
        feats = torch.from_numpy(np.ascontiguousarray(y)).to(DEV)  # (Tm, B, P): a time-major "network input"
        graph = io.DenominatorGraph(ps.den_fst(), ps.P)
        torch.manual_seed(5)
        model = torch.nn.Linear(ps.P, ps.P).to(DEV)
        ddp = DistributedDataParallel(model, device_ids=[0])

        def handle():
            return io.Supervision.from_e2e_fsts(ps.WEIGHT, my_lens, ps.P, fsts)

        out = ddp(feats).permute(1, 2, 0)  # (B, C, T) view, time-major
        loss, res = parallel.chain_loss_data_parallel(out, graph, handle(), ps.L2, ps.LEAKY, on_failure="sequence")
        loss.backward()
        with torch.no_grad():
            local_out = model(feats).permute(1, 2, 0)
        _, local = chain_loss(local_out, graph, handle(), ps.L2, ps.LEAKY, on_failure="sequence")
        torch.cuda.synchronize()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), res=res.data.numpy(), loss=float(loss.detach()), local=local.data.numpy(),
                 status=res.per_sequence.status.numpy(), wgrad=model.weight.grad.cpu().numpy(), bgrad=model.bias.grad.cpu().numpy())
    finally:
        dist.destroy_process_group()


def test_data_parallel_with_a_failed_sequence_on_one_rank(tmp_path):
    import torch.multiprocessing as mp

    from torchain_amd import parallel

    name, world = "e2e_ragged", 2
    lens = ps.lengths(name)
    S, bad = len(lens), ps.BAD[name]
    assert parallel.shard_range(S, 0, world)[0] <= bad < parallel.shard_range(S, 0, world)[1]
    mp.spawn(_dp_worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [np.load(str(tmp_path / ("rank%d.npz" % k))) for k in range(world)]
    assert r[0]["res"].tobytes() == r[1]["res"].tobytes() and r[0]["loss"] == r[1]["loss"]
    total = r[0]["local"].astype(np.float64) + r[1]["local"].astype(np.float64)
    assert np.array_equal(r[0]["res"], total.astype(np.float32)), (r[0]["res"], total)
    assert r[0]["status"].tolist() == [1 if s == bad else 0 for s in range(*parallel.shard_range(S, 0, world))]
    assert r[1]["status"].tolist() == [0] * (S - parallel.shard_range(S, 0, world)[1])  # the report stays local to the rank
    assert abs(r[0]["res"][2] - ps.WEIGHT * (sum(lens) - lens[bad])) <= 1e-6 * r[0]["res"][2]  # the survivors' frames
    assert np.isfinite(r[0]["loss"]) and abs(r[0]["loss"] + r[0]["res"][0] / r[0]["res"][2]) <= 1e-6 * abs(r[0]["loss"])
    for k in ("wgrad", "bgrad"):
        assert np.isfinite(r[0][k]).all() and r[0][k].any() and r[0][k].tobytes() == r[1][k].tobytes(), k
