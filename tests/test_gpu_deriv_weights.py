"""Kaldi's per-frame derivative weights (``chain_loss(..., deriv_weights=w)``, ``tc_chain_step_weighted``): every gradient
element becomes ``w[row] * g``, one float32 multiply of the unweighted value (rounded once for 16-bit inputs), and the
results, the loss and ``xent_objf`` do not change.  Held bit for bit to the unweighted float32 call's gradients times ``w``
-- (B, C, T), 2-D and 2-D with a row stride, float32 / bfloat16 / float16, without and with the cross-entropy branch both
ways of ``kaldi_way``; on a small graph, C2, every denominator kernel family and both numerator modes, an end-to-end
supervision and C3.  Also: all-ones weights, the oracle, soft failure, evaluation, the registered operator, stream capture,
the data-parallel wrapper and a recipe trained on egs with ``<DW2>`` weights."""
import os

import numpy as np
import pytest
import torch

from torchain_amd import io, parallel, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss

import e2e_reference as ref
from helpers import REL, free_port, from3d, rel_err, to3d

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
LAYOUTS = ["3d", "2d", "2d_strided"]
XENT = [None, True, False]  # no cross-entropy branch, kaldi_way=True, kaldi_way=False
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
# what <DW> bytes decode to (k / 255), 0, 1 and weights above 1
_POOL = np.array([0.0, 1.0 / 255, 37.0 / 255, 128.0 / 255, 254.0 / 255, 1.0, 1.0, 1.0, 1.5, 2.0, 3.25], np.float32)


def _bits(t):
    return t.detach().contiguous().view(_BITS[t.dtype]).cpu()


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    diff = (_bits(a) != _bits(b))
    assert not bool(diff.any()), "%s: %d of %d elements differ" % (what, int(diff.sum()), diff.numel())


def _weights(S, T, seed):
    w = np.random.default_rng(seed).choice(_POOL, size=S * T)
    w[:len(_POOL)] = _POOL  # (every kind of weight at least once)
    return torch.from_numpy(w.astype(np.float32))


def _in_layout(w, S, T, three_d):
    """(T*S,) frame-major weights as a factor broadcast over the gradient of that layout."""
    w = w.to(DEV)
    return w.view(T, S).t().unsqueeze(1) if three_d else w.unsqueeze(1)


def _layout(y2d, S, T, layout, dtype, pad=5):
    """(S*T, P) float32 values -> a leaf tensor of ``dtype`` in the given layout."""
    P = y2d.shape[1]
    y = y2d.to(DEV).to(dtype)
    if layout == "3d":
        return y.view(T, S, P).permute(1, 2, 0).contiguous().requires_grad_(True)
    if layout == "2d":
        return y.clone().requires_grad_(True)
    wide = torch.zeros(S * T, P + pad, dtype=dtype, device=DEV)
    wide[:, :P] = y
    return wide[:, :P].detach().requires_grad_(True)  # (row stride P + pad)


def _run(x, xe, graph, sup, xent, l2, leaky, w=None):
    kw = dict(l2_regularize=l2, leaky_hmm_coefficient=leaky)
    if xent is not None:
        kw.update(xent_regularize=0.1, xent_input=xe, kaldi_way=xent)
    if w is not None:
        kw.update(deriv_weights=w)
    loss, res = chain_loss(x, graph, sup, **kw)
    loss.backward()
    return loss.detach(), res.data.clone(), res.xent_objf, x.grad, (xe.grad if xent is not None else None)


def _check_weighted(graph, sup, S, T, y2d, xe2d, dtype, layout, xent, w, l2=5e-5, leaky=0.1, one_step=True):
    """The weighted call against the unweighted float32 call on the (up-cast) same values: scalars equal, gradients equal
    that call's gradients times w, .to(dtype).  Returns the weighted call's outputs."""
    x = _layout(y2d, S, T, layout, dtype)
    xe = _layout(xe2d, S, T, layout, dtype) if xent is not None else None
    steps = lib.tc_debug_counter(b"den_launches")
    got = _run(x, xe, graph, sup, xent, l2, leaky, w=w)
    if one_step:
        assert lib.tc_debug_counter(b"den_launches") - steps == 1  # (one step: the weights add no second objective call)
    if dtype == torch.float32:
        xf = _layout(y2d, S, T, layout, dtype)
        xef = _layout(xe2d, S, T, layout, dtype) if xent is not None else None
    else:
        xf = x.detach().float().requires_grad_(True)
        xef = xe.detach().float().requires_grad_(True) if xe is not None else None
    want = _run(xf, xef, graph, sup, xent, l2, leaky)
    wl = _in_layout(w, S, T, layout == "3d")
    _same_bits(got[0], want[0].to(dtype), "loss")
    _same_bits(got[1], want[1], "results.data")
    assert got[2] == want[2]
    assert got[3].dtype == dtype and tuple(got[3].shape) == tuple(x.shape)
    _same_bits(got[3], (want[3] * wl).to(dtype), "grad")
    if xent is not None:
        _same_bits(got[4], (want[4] * wl).to(dtype), "xent grad")
    return got


_workloads = {}


def _workload(cfgname, S, T, seed=3, cached=True):
    """(cached=False: a graph built anew, for the diagnostic switches a test has set, which are read when a graph is built)"""
    key = (cfgname, S, T, seed)
    if cached and key in _workloads:
        return _workloads[key]
    cfg = synth.CONFIGS[cfgname]
    fst = synth.config_den_fst(cfgname)
    graph = io.DenominatorGraph(fst, cfg["P"]).prepare(DEV)
    sup = synth.random_supervision(fst, S, T, 3, seed=seed, initial_probs=graph.initial_probs())
    y = torch.from_numpy(synth.random_nnet_output(S, T, cfg["P"], seed=seed + 1))
    xe = torch.log_softmax(torch.from_numpy(synth.random_nnet_output(S, T, cfg["P"], seed=seed + 2)), dim=1)
    out = cfg, graph, io.Supervision.from_synth(sup), y, xe
    if cached and cfgname != "C3":
        _workloads[key] = out
    return out


_small = {}


def _small_workload(S=6, T=24, P=96):
    if not _small:
        fst = synth.random_den_fst(300, 4, P, seed=4)
        graph = io.DenominatorGraph(fst, P).prepare(DEV)
        sup = synth.random_supervision(fst, S, T, 3, seed=2, initial_probs=graph.initial_probs())
        _small.update(graph=graph, sup=io.Supervision.from_synth(sup), S=S, T=T, fst=fst,
                      y=torch.from_numpy(synth.random_nnet_output(S, T, P, seed=6)) * 3.0,
                      xe=torch.from_numpy(synth.random_nnet_output(S, T, P, seed=7)))
    return _small


# ---- layouts x dtypes x cross-entropy branch ----------------------------------------------------------------------------
@pytest.mark.parametrize("xent", XENT)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_graph_gradients_are_weighted(dtype, layout, xent):
    s = _small_workload()
    _check_weighted(s["graph"], s["sup"], s["S"], s["T"], s["y"], s["xe"], dtype, layout, xent, _weights(s["S"], s["T"], 1),
                    l2=1e-3)


@pytest.mark.parametrize("xent", XENT)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_c2_gradients_are_weighted(dtype, layout, xent):
    S, T = 64, 150
    cfg, graph, sup, y, xe = _workload("C2", S, T)
    _check_weighted(graph, sup, S, T, y, xe, dtype, layout, xent, _weights(S, T, 2), l2=cfg["l2"], leaky=cfg["leaky"])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_ones_weights_are_the_unweighted_call(dtype, layout):
    s = _small_workload()
    S, T = s["S"], s["T"]
    outs = []
    for w in (None, torch.ones(S * T, device=DEV)):
        x, xe = _layout(s["y"], S, T, layout, dtype), _layout(s["xe"], S, T, layout, dtype)
        outs.append(_run(x, xe, s["graph"], s["sup"], True, 1e-3, 0.1, w=w))
    for i, what in ((0, "loss"), (1, "results"), (3, "grad"), (4, "xent grad")):
        _same_bits(outs[0][i], outs[1][i], what)
    assert outs[0][2] == outs[1][2]


# ---- the 2-D float32 gradient's row-scale pass on every kernel family, both numerator modes -------------------------
@pytest.mark.parametrize("mode", ["staged", "no_num_overlap"])
@pytest.mark.parametrize("family", [None, "force_general", "force_streamed", "force_pair", "force_mitm"])
def test_kernel_families_and_numerator_modes(kernel_family, family, mode):
    if family is not None:
        kernel_family(family)
    if mode == "no_num_overlap":
        kernel_family("no_num_overlap")
    S, T = 16, 60  # (a small batch: by default the numerator runs beside the denominator and is scattered behind it)
    cfg, graph, sup, y, xe = _workload("C2", S, T, seed=11, cached=False)
    for layout in ("2d", "2d_strided", "3d"):
        for xent in XENT:
            _check_weighted(graph, sup, S, T, y, xe, torch.float32, layout, xent, _weights(S, T, 3), l2=cfg["l2"],
                            leaky=cfg["leaky"], one_step=False)


@pytest.mark.parametrize("mode", ["staged", "no_num_overlap"])
def test_plane_wise_graph(kernel_family, mode):
    """A tied graph of the plane-wise class (as large as tests/test_gpu_planes.py builds for chain_loss)."""
    if mode == "no_num_overlap":
        kernel_family("no_num_overlap")
    fst = synth.random_den_fst(18000, 3, 400, seed=71)
    S, T, P = 3, 11, fst.num_pdfs
    graph = io.DenominatorGraph(fst, P).prepare(DEV)
    assert graph.stats()["tied"] == 1 and graph.stats()["lds_bytes"] > 100 * 1024
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 2, seed=72, initial_probs=graph.initial_probs()))
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=73))
    xe = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=74))
    for layout in ("2d", "3d"):
        for xent in XENT:
            _check_weighted(graph, sup, S, T, y, xe, torch.float32, layout, xent, _weights(S, T, 4), l2=5e-5, one_step=False)


@pytest.mark.parametrize("mode", ["staged", "no_num_overlap"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_e2e_supervision(kernel_family, dtype, layout, mode):
    if mode == "no_num_overlap":
        kernel_family("no_num_overlap")
    S, T, P = 16, 40, 60
    graph = io.DenominatorGraph(synth.random_den_fst(80, 4, P, seed=31), P).prepare(DEV)
    sup = io.Supervision.from_e2e_fsts(0.9, T, P, ref.batch("chain", S, P, seed=11))
    rng = np.random.default_rng(12)
    y = torch.from_numpy((rng.normal(size=(S * T, P)) * 2.0).astype(np.float32))
    xe = torch.from_numpy(rng.normal(size=(S * T, P)).astype(np.float32))
    for xent in XENT:
        _check_weighted(graph, sup, S, T, y, xe, dtype, layout, xent, _weights(S, T, 5), l2=1e-4)


def test_c3_weighted_step():
    S, T = 256, 150
    cfg, graph, sup, y, xe = _workload("C3", S, T, seed=5)
    w = _weights(S, T, 6).to(DEV)
    _check_weighted(graph, sup, S, T, y, xe, torch.float32, "3d", True, w, l2=cfg["l2"], leaky=cfg["leaky"])
    _check_weighted(graph, sup, S, T, y, xe, torch.float32, "2d", None, w, l2=cfg["l2"], leaky=cfg["leaky"])
    _check_weighted(graph, sup, S, T, y, xe, torch.bfloat16, "3d", None, w, l2=cfg["l2"], leaky=cfg["leaky"])


# ---- against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["2d", "3d"])
def test_oracle_at_c2(oracle, layout):
    c = synth.CONFIGS["C2"]
    fst = synth.config_den_fst("C2")
    S, T, P = 6, 40, c["P"]
    g = oracle.DenGraph(fst)
    sup = synth.random_supervision(fst, S, T, 3, seed=7, initial_probs=g.initial_probs())
    y = synth.random_nnet_output(S, T, P, seed=5)
    want = oracle.compute_chain_objf_and_deriv(g, sup, y, c["l2"], c["leaky"], want_xent=True)
    w = _weights(S, T, 7)
    wn = w.numpy().astype(np.float64)[:, None]
    graph = io.DenominatorGraph(fst, P)
    if layout == "3d":
        x, xe = to3d(y, S, T, P).requires_grad_(True), to3d(y, S, T, P).requires_grad_(True)
    else:
        x, xe = torch.from_numpy(y).to(DEV).requires_grad_(True), torch.from_numpy(y).to(DEV).requires_grad_(True)
    loss, res = chain_loss(x, graph, io.Supervision.from_synth(sup), c["l2"], c["leaky"], 0.1, xe, True, deriv_weights=w)
    loss.backward()
    got = res.data.numpy()
    assert abs(got[0] - want["objf"]) <= REL * abs(want["objf"]) and got[2] == want["weight"]
    grad = from3d(x.grad, S, T, P) if layout == "3d" else x.grad.cpu().numpy()
    xgrad = from3d(xe.grad, S, T, P) if layout == "3d" else xe.grad.cpu().numpy()
    assert rel_err(-grad, want["deriv"] * wn, floor=1.0) <= REL
    assert rel_err(-xgrad, 0.1 * want["xent_deriv"] * wn, floor=0.1) <= REL
    assert np.all(grad[w.numpy() == 0] == 0) and np.all(xgrad[w.numpy() == 0] == 0)


# ---- soft failure, evaluation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", ["3d", "2d"])
@pytest.mark.parametrize("kaldi_way", [True, False])
def test_soft_failure_gradient_is_weighted(dtype, layout, kaldi_way):
    """A numerical failure with l2 != 0: the gradient is w times -l2 * weight * y, the xent gradient 0."""
    s = _small_workload()
    S, T = s["S"], s["T"]
    y, xe = s["y"].clone(), s["xe"].clone()
    (y if kaldi_way else xe)[17, 5] = float("inf")  # (kaldi_way=False evaluates the objective on xent_input)
    w = _weights(S, T, 8)
    w[17] = 0.5  # (no 0 * inf)
    got = _check_weighted(s["graph"], s["sup"], S, T, y, xe, dtype, layout, kaldi_way, w, l2=1e-3)
    assert float(got[1][0]) == -10.0 * S * T and float(got[1][2]) == S * T
    assert torch.count_nonzero(got[4]) == 0
    assert got[2] == 0.0
    zero = _in_layout(w, S, T, layout == "3d").expand_as(got[3]) == 0
    assert torch.count_nonzero(got[3][zero]) == 0 and torch.count_nonzero(got[3][~zero]) > 0


@pytest.mark.parametrize("layout", ["3d", "2d"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_evaluation_ignores_checked_weights(dtype, layout):
    s = _small_workload()
    S, T = s["S"], s["T"]
    kw = dict(l2_regularize=1e-3, leaky_hmm_coefficient=0.1, xent_regularize=0.1, kaldi_way=True)
    x, xe = _layout(s["y"], S, T, layout, dtype), _layout(s["xe"], S, T, layout, dtype)
    with torch.no_grad():
        loss0, res0 = chain_loss(x, s["graph"], s["sup"], xent_input=xe, **kw)
        want = loss0.clone(), res0.data.clone(), res0.xent_objf
        for w in (_weights(S, T, 9), _weights(S, T, 9).to(DEV)):
            loss, res = chain_loss(x, s["graph"], s["sup"], xent_input=xe, deriv_weights=w, **kw)
            _same_bits(loss, want[0], "loss")
            _same_bits(res.data, want[1], "results")
            assert res.xent_objf == want[2]
        for bad in (torch.ones(S * T + 1), torch.ones(S, T), torch.ones(S * T - 1, device=DEV)):
            with pytest.raises(ValueError):
                chain_loss(x, s["graph"], s["sup"], xent_input=xe, deriv_weights=bad, **kw)
    with pytest.raises(ValueError):  # (and when training)
        chain_loss(x, s["graph"], s["sup"], xent_input=xe, deriv_weights=torch.ones(S * T + 1), **kw)


# ---- operator, capture, data parallel -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["3d", "2d"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_registered_operator_takes_weights(dtype, layout):
    from torchain_amd.ops import chain_loss_op
    S, T = 8, 20
    cfg, graph, sup, y, xe = _workload("C2", S, T, seed=21)
    kw = dict(l2_regularize=5e-5, leaky_hmm_coefficient=0.1, xent_regularize=0.1, kaldi_way=True)
    w = _weights(S, T, 10)
    outs = []
    for fn in (chain_loss, chain_loss_op):
        a, b = _layout(y, S, T, layout, dtype), _layout(xe, S, T, layout, dtype)
        loss, res = fn(a, graph, sup, xent_input=b, deriv_weights=w, **kw)
        loss.sum().backward()
        outs.append((loss.detach(), res.data.clone(), a.grad, b.grad, res.xent_objf))
    for i, what in enumerate(("loss", "results", "grad", "xent grad")):
        _same_bits(outs[0][i], outs[1][i], what)
    assert outs[0][4] == outs[1][4]
    with pytest.raises(ValueError):
        chain_loss_op(a, graph, sup, xent_input=b, deriv_weights=torch.ones(3), **kw)


def test_registered_operator_with_weights_traces_as_one_node():
    from torchain_amd import ops  # noqa: F401
    S, T, P = 4, 20, 100
    fst = synth.random_den_fst(256, 6, P, seed=5)
    graph = io.DenominatorGraph(fst, P).prepare(DEV)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=9, initial_probs=graph.initial_probs()))
    x = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=10)).to(DEV)
    w = _weights(S, T, 11).to(DEV)
    gp, sp = int(graph.ptr.value), int(sup.ptr.value)

    def step(a, wt):
        out, _grad, _xgrad = torch.ops.torchain_amd.chain_step(a, a.new_empty((0,)), gp, sp, 5e-5, 0.1, 0.0, True, True, wt)
        return out[3]

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    a = x.clone().requires_grad_(True)
    loss = torch.compile(step, backend=backend, fullgraph=True)(a, w)
    loss.backward()
    assert len(graphs) == 1
    calls = [n for n in graphs[0].graph.nodes if n.op == "call_function" and "chain_step" in str(n.target)]
    assert len(calls) == 1, graphs[0].graph
    b = x.clone().requires_grad_(True)
    ref_loss, _ = chain_loss(b, graph, sup, 5e-5, 0.1, deriv_weights=w)
    ref_loss.backward()
    _same_bits(loss.detach().reshape(1), ref_loss.detach(), "loss")
    _same_bits(a.grad, b.grad, "grad")


@pytest.mark.parametrize("layout", ["3d", "2d"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_step_reads_the_weights_current_values(dtype, layout):
    S, T = 8, 30
    cfg, graph, sup, y, _ = _workload("C2", S, T)
    kw = dict(l2_regularize=5e-5, leaky_hmm_coefficient=cfg["leaky"], xent_regularize=0.1, kaldi_way=True)
    x = _layout(y, S, T, layout, dtype)
    xe = (0.5 * x.detach()).requires_grad_(True)
    w_cuda = _weights(S, T, 12).to(DEV)

    def step(w):
        loss, results = chain_loss(x, graph, sup, xent_input=xe, deriv_weights=w, **kw)
        g, gx = torch.autograd.grad(loss, (x, xe))
        return loss.detach(), g, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(w_cuda)
    side.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=side):
        captured = step(w_cuda)
    for seed in (13, 14):
        with torch.no_grad():
            w_cuda.copy_(_weights(S, T, seed).to(DEV))
        cg.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        want = step(w_cuda.clone())
        for g, w_, what in zip(got, want, ("loss", "grad", "xent grad")):
            _same_bits(g, w_, what)
    unweighted = step(None)
    assert not torch.equal(got[1], unweighted[1])
    # a CPU vector cannot be copied inside a capture
    w_cpu = w_cuda.cpu()
    cg2 = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError):
        with torch.cuda.graph(cg2, stream=side):
            x.detach().sum()
            chain_loss(x, graph, sup, xent_input=xe, deriv_weights=w_cpu, **kw)
    torch.cuda.synchronize()


def _dp_worker(rank, world, port, S, T, P, out_dir):
    """One rank: its shard of the sequences and of the weights through parallel.chain_loss_data_parallel on cuda:0 (both ranks
    share the GPU of the test box; the collective travels over gloo), as tests/test_gpu_parallel.py."""
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
        xe_local = np.ascontiguousarray(parallel.shard_rows(torch.from_numpy(d["xe"]), S, lo, hi).numpy())
        w_local = parallel.shard_deriv_weights(torch.from_numpy(d["dw"]), S, lo, hi)
        den, hsup = io.DenominatorGraph(fst, P), io.Supervision.from_synth(parallel.shard_supervision_fst(sup, lo, hi))
        B = hi - lo
        x = to3d(y_local, B, T, P).requires_grad_(True)
        x2 = to3d(xe_local, B, T, P).requires_grad_(True)
        loss, res = parallel.chain_loss_data_parallel(x, den, hsup, 1e-3, 0.1, 0.1, x2, kaldi_way=True, deriv_weights=w_local)
        loss.backward()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), res=res.data.numpy(), xent=res.xent_objf, loss=float(loss),
                 grad=from3d(x.grad, B, T, P), xgrad=from3d(x2.grad, B, T, P))
    finally:
        dist.destroy_process_group()


def test_data_parallel_two_ranks_with_weights(tmp_path):
    import torch.multiprocessing as mp

    world, S, T, P = 2, 5, 12, 64  # uneven shards: 3 + 2 sequences
    fst = synth.random_den_fst(120, 5, P, seed=71)
    sup = synth.random_supervision(fst, S, T, 1, seed=72, weight=0.5)  # 1 path: single boundary states
    y = synth.random_nnet_output(S, T, P, seed=73)
    xe = torch.log_softmax(torch.from_numpy(synth.random_nnet_output(S, T, P, seed=74)), dim=1).numpy()
    w = _weights(S, T, 15)
    np.savez(str(tmp_path / "inputs.npz"), y=y, xe=xe, dw=w.numpy(), w=sup.weight, nst=sup.num_states, arc_begin=sup.arc_begin,
             ilabel=sup.ilabel, arc_weight=sup.arc_weight, nextstate=sup.nextstate, final=sup.final)
    mp.spawn(_dp_worker, args=(world, free_port(), S, T, P, str(tmp_path)), nprocs=world, join=True)
    # the single call on the whole batch, weighted and not
    den, hsup = io.DenominatorGraph(fst, P), io.Supervision.from_synth(sup)
    single = {}
    for key, dw in (("weighted", w), ("plain", None)):
        x, x2 = to3d(y, S, T, P).requires_grad_(True), to3d(xe, S, T, P).requires_grad_(True)
        loss, res = chain_loss(x, den, hsup, 1e-3, 0.1, 0.1, x2, kaldi_way=True, deriv_weights=dw)
        loss.backward()
        single[key] = (res.data.numpy().copy(), res.xent_objf, from3d(x.grad, S, T, P), from3d(x2.grad, S, T, P))
    _same_bits(torch.from_numpy(single["weighted"][0]), torch.from_numpy(single["plain"][0]), "single-call results")
    r = [np.load(str(tmp_path / ("rank%d.npz" % k))) for k in range(world)]
    np.testing.assert_array_equal(r[0]["res"], r[1]["res"])
    want = single["plain"][0]
    assert abs(r[0]["res"][0] - want[0]) <= REL * abs(want[0]) and r[0]["res"][2] == want[2]
    assert abs(r[0]["res"][1] - want[1]) <= REL * abs(want[1])
    assert abs(float(r[0]["xent"]) - single["plain"][1]) <= REL * abs(single["plain"][1])
    for k in range(world):
        lo, hi = parallel.shard_range(S, k, world)
        g = parallel.shard_rows(torch.from_numpy(single["weighted"][2]), S, lo, hi).numpy()
        xg = parallel.shard_rows(torch.from_numpy(single["weighted"][3]), S, lo, hi).numpy()
        assert rel_err(r[k]["grad"], g, floor=0.5) <= REL
        assert rel_err(r[k]["xgrad"], xg, floor=0.05) <= REL
        zero = parallel.shard_deriv_weights(w.numpy(), S, lo, hi) == 0
        assert np.all(r[k]["grad"][zero] == 0) and np.all(r[k]["xgrad"][zero] == 0)


# ---- a recipe on egs with <DW2> weights -----------------------------------------------------------------------------
def _weighted_egs(tmp_path, fst, lengths, seed):
    import kaldi_egs_writer as kw
    import recipe_fixture as rf
    emb = np.random.default_rng(1234).standard_normal((fst.num_pdfs, rf.FEAT)).astype(np.float32)
    rng = np.random.default_rng(seed)
    keyed = []
    for i, L in enumerate(lengths):
        eg = rf.learnable_example(fst, L, seed=seed + i, emb=emb)
        eg["outputs"][0]["deriv_weights"] = rng.choice(_POOL, size=L).astype(np.float32)
        keyed.append(("dw%03d-%d" % (i, L), eg))
    ark, scp = str(tmp_path / "dw.ark"), str(tmp_path / "dw.scp")
    kw.write_ark(ark, keyed, scp_path=scp, dw="DW2")
    with open(scp + ".len", "w") as f:
        f.write("".join("%s %d\n" % (k, L) for (k, _), L in zip(keyed, lengths)))
    return scp


def test_recipe_with_egs_weights(tmp_path):
    """io.RandExample -> the recipe's network -> chain_loss(..., deriv_weights=ex.deriv_weights): the parameter gradients are
    those of the unweighted loss with the weights applied by a hook on the network's outputs, and the loss falls."""
    import copy

    import recipe_fixture as rf
    P = 32
    fst = synth.random_den_fst(120, 4, P, seed=3)
    scp = _weighted_egs(tmp_path, fst, [20] * 32, seed=100)
    graph = io.DenominatorGraph(fst, P).prepare(DEV)
    egs = io.RandExample(scp, seed=1, batchsize=8)
    torch.manual_seed(0)
    model = rf.TwoLayerTdnn(P).to(DEV)
    hooked = copy.deepcopy(model)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
    kw = dict(l2_regularize=5e-5, leaky_hmm_coefficient=0.1, xent_regularize=0.1, kaldi_way=True)
    losses, compared, nontrivial = [], 0, False
    for epoch in range(10):
        egs.reset()
        for (feats, ivec), sup in egs:
            w = egs.deriv_weights
            B, T = sup.n_batch, sup.n_frame
            assert w.shape == (T * B,)
            nontrivial |= bool((w != 1).any())
            feats, ivec = feats.to(DEV), ivec.to(DEV)
            mmi, xe = model(feats, ivec)
            loss, res = chain_loss(mmi, graph, sup, xent_input=xe, deriv_weights=w, **kw)
            loss.backward()
            if epoch == 0:
                hooked.load_state_dict(model.state_dict())
                hooked.zero_grad(set_to_none=True)
                hm, hx = hooked(feats, ivec)
                w_bct = w.to(DEV).view(T, B).t().unsqueeze(1)
                hm.register_hook(lambda g: g * w_bct)
                hx.register_hook(lambda g: g * w_bct)
                hloss, _ = chain_loss(hm, graph, sup, xent_input=hx, **kw)
                hloss.backward()
                for (name, p), q in zip(model.named_parameters(), hooked.parameters()):
                    np.testing.assert_allclose(p.grad.cpu().numpy(), q.grad.cpu().numpy(), rtol=1e-5, atol=1e-6,
                                               err_msg=name)
                compared += 1
            opt.step()
            opt.zero_grad(set_to_none=False)
            losses.append(float(res.loss))
    assert compared >= 2 and nontrivial
    assert np.isfinite(losses).all()
    first, last = np.mean(losses[:4]), np.mean(losses[-4:])
    assert last < 0.9 * first, (first, last, losses)
