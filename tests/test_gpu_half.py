"""bfloat16 / float16 network outputs (a model trained under ``torch.autocast``) through ``chain_loss``: ONE
``tc_chain_step_typed`` call, which widens the 16-bit tensors as it reads them and rounds each gradient element once as it
writes it.  Held bit for bit to the float32 path on the up-cast inputs: ``results.data``, ``xent_objf`` and the loss
(``.to(dtype)``) equal, the gradients equal the float32 ones ``.to(dtype)`` -- (B, C, T), 2-D and 2-D with a row stride,
without and with the cross-entropy branch both ways of ``kaldi_way``; on a small graph, the C2 workload, the other kernel
families, an end-to-end supervision and C3.  Also: the evaluation step allocates no float32 copy, soft failure, the
registered operator, stream capture, the data-parallel wrapper and a recipe trained under autocast."""
import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss

import e2e_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
LAYOUTS = ["3d", "2d", "2d_strided"]
XENT = [None, True, False]  # no cross-entropy branch, kaldi_way=True, kaldi_way=False
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def _bits(t):
    return t.detach().contiguous().view(_BITS[t.dtype]).cpu()


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    diff = (_bits(a) != _bits(b))
    assert not bool(diff.any()), "%s: %d of %d elements differ" % (what, int(diff.sum()), diff.numel())


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


def _run(x, xe, graph, sup, xent, l2, leaky):
    kw = dict(l2_regularize=l2, leaky_hmm_coefficient=leaky)
    if xent is not None:
        kw.update(xent_regularize=0.1, xent_input=xe, kaldi_way=xent)
    loss, res = chain_loss(x, graph, sup, **kw)
    loss.backward()
    return loss.detach(), res.data.clone(), res.xent_objf, x.grad, (xe.grad if xent is not None else None)


def _check_against_float32(graph, sup, S, T, y2d, xe2d, dtype, layout, xent, l2=5e-5, leaky=0.1):
    x = _layout(y2d, S, T, layout, dtype)
    xe = _layout(xe2d, S, T, layout, dtype) if xent is not None else None
    steps = lib.tc_debug_counter(b"den_launches")
    got = _run(x, xe, graph, sup, xent, l2, leaky)
    assert lib.tc_debug_counter(b"den_launches") - steps == 1  # (one step: no second objective call, no float32 detour)
    xf = x.detach().float().requires_grad_(True)  # (contiguous: what out.float() gives)
    xef = xe.detach().float().requires_grad_(True) if xe is not None else None
    want = _run(xf, xef, graph, sup, xent, l2, leaky)
    assert got[0].dtype == dtype
    _same_bits(got[0], want[0].to(dtype), "loss")
    _same_bits(got[1], want[1], "results.data")
    assert got[2] == want[2]
    assert got[3].dtype == dtype and tuple(got[3].shape) == tuple(x.shape)
    _same_bits(got[3], want[3].to(dtype), "grad")
    if xent is not None:
        _same_bits(got[4], want[4].to(dtype), "xent grad")
    return got


def _workload(cfgname, S, T, seed=3):
    cfg = synth.CONFIGS[cfgname]
    fst = synth.config_den_fst(cfgname)
    graph = io.DenominatorGraph(fst, cfg["P"]).prepare(DEV)
    sup = synth.random_supervision(fst, S, T, 3, seed=seed, initial_probs=graph.initial_probs())
    y = torch.from_numpy(synth.random_nnet_output(S, T, cfg["P"], seed=seed + 1))
    xe = torch.log_softmax(torch.from_numpy(synth.random_nnet_output(S, T, cfg["P"], seed=seed + 2)), dim=1)
    return cfg, graph, io.Supervision.from_synth(sup), y, xe


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


@pytest.mark.parametrize("xent", XENT)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_graph_equals_float32_path(dtype, layout, xent):
    w = _small_workload()
    _check_against_float32(w["graph"], w["sup"], w["S"], w["T"], w["y"], w["xe"], dtype, layout, xent, l2=1e-3)


@pytest.mark.parametrize("xent", XENT)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_c2_equals_float32_path(dtype, layout, xent):
    S, T = 64, 150
    cfg, graph, sup, y, xe = _workload("C2", S, T)
    _check_against_float32(graph, sup, S, T, y, xe, dtype, layout, xent, l2=cfg["l2"], leaky=cfg["leaky"])


@pytest.mark.parametrize("family", ["force_general", "force_streamed"])
@pytest.mark.parametrize("layout", ["3d", "2d_strided"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_other_kernel_families_equal_float32_path(kernel_family, family, dtype, layout):
    kernel_family(family)
    S, T = 16, 60
    cfg, graph, sup, y, xe = _workload("C2", S, T, seed=11)
    for xent in XENT:
        _check_against_float32(graph, sup, S, T, y, xe, dtype, layout, xent, l2=cfg["l2"], leaky=cfg["leaky"])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_e2e_supervision_equals_float32_path(dtype, layout):
    S, T, P = 16, 40, 60
    graph = io.DenominatorGraph(synth.random_den_fst(80, 4, P, seed=31), P).prepare(DEV)
    sup = io.Supervision.from_e2e_fsts(0.9, T, P, ref.batch("chain", S, P, seed=11))
    rng = np.random.default_rng(12)
    y = torch.from_numpy((rng.normal(size=(S * T, P)) * 2.0).astype(np.float32))
    xe = torch.from_numpy(rng.normal(size=(S * T, P)).astype(np.float32))
    for xent in XENT:
        _check_against_float32(graph, sup, S, T, y, xe, dtype, layout, xent, l2=1e-4)


def test_c3_bfloat16_equals_float32_path():
    S, T = 256, 150
    cfg, graph, sup, y, xe = _workload("C3", S, T, seed=5)
    _check_against_float32(graph, sup, S, T, y, xe, torch.bfloat16, "3d", True, l2=cfg["l2"], leaky=cfg["leaky"])


@pytest.mark.parametrize("layout", ["3d", "2d"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_evaluation_step_takes_half_input_as_it_is(dtype, layout):
    """Under ``no_grad`` the 16-bit input goes to the step as it is: the results equal the training step's and those of the
    float32 evaluation on the up-cast input, and once warm the call allocates far less than a float32 copy of the input."""
    S, T = 64, 150
    cfg, graph, sup, y, xe = _workload("C2", S, T, seed=13)
    kw = dict(l2_regularize=cfg["l2"], leaky_hmm_coefficient=cfg["leaky"], xent_regularize=0.1, kaldi_way=True)
    x, xe = _layout(y, S, T, layout, dtype), _layout(xe, S, T, layout, dtype)
    train = _run(x, xe, graph, sup, True, cfg["l2"], cfg["leaky"])
    with torch.no_grad():
        loss_f, res_f = chain_loss(x.detach().float(), graph, sup, xent_input=xe.detach().float(), **kw)
        want = res_f.data.clone(), res_f.xent_objf
        for _ in range(2):  # (the second call is warm: workspace and pools)
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            loss, res = chain_loss(x, graph, sup, xent_input=xe, **kw)
            torch.cuda.synchronize()
            grown = torch.cuda.memory_allocated() - before
    assert grown < S * T * cfg["P"] * 4, grown
    assert loss.dtype == dtype and not loss.requires_grad
    _same_bits(res.data, want[0], "evaluation results")
    assert res.xent_objf == want[1]
    _same_bits(loss, loss_f.to(dtype), "evaluation loss")
    assert float(res.data[2]) == float(train[1][2])
    np.testing.assert_allclose(res.data.numpy()[:2], train[1].numpy()[:2], rtol=1e-6)


@pytest.mark.parametrize("layout", ["3d", "2d"])
@pytest.mark.parametrize("kaldi_way", [True, False])
def test_soft_failure_zeroes_the_half_gradient(layout, kaldi_way):
    w = _small_workload()
    S, T = w["S"], w["T"]
    y, xe = w["y"].clone(), w["xe"].clone()
    (y if kaldi_way else xe)[17, 5] = float("inf")  # (kaldi_way=False evaluates the objective on xent_input)
    got = _check_against_float32(w["graph"], w["sup"], S, T, y, xe, torch.bfloat16, layout, kaldi_way, l2=0.0)
    assert float(got[1][0]) == -10.0 * S * T and float(got[1][2]) == S * T
    src = _layout(y if kaldi_way else xe, S, T, layout, torch.bfloat16).detach()
    assert torch.count_nonzero(got[3][torch.isfinite(src)]) == 0
    assert torch.count_nonzero(got[4]) == 0
    assert got[2] == 0.0


@pytest.mark.parametrize("layout", ["3d", "2d"])
def test_registered_operator_on_bfloat16(layout):
    from torchain_amd.ops import chain_loss_op
    S, T = 8, 20
    cfg, graph, sup, y, xe = _workload("C2", S, T, seed=21)
    kw = dict(l2_regularize=5e-5, leaky_hmm_coefficient=0.1, xent_regularize=0.1, kaldi_way=True)
    outs = []
    for fn in (chain_loss, chain_loss_op):
        a, b = _layout(y, S, T, layout, torch.bfloat16), _layout(xe, S, T, layout, torch.bfloat16)
        loss, res = fn(a, graph, sup, xent_input=b, **kw)
        loss.sum().backward()
        outs.append((loss.detach(), res.data.clone(), a.grad, b.grad, res.xent_objf))
    for i, what in enumerate(("loss", "results", "grad", "xent grad")):
        _same_bits(outs[0][i], outs[1][i], what)
    assert outs[0][4] == outs[1][4]
    with pytest.raises(ValueError):
        chain_loss_op(a, graph, sup, xent_input=b.detach().float(), **kw)


def test_registered_operator_on_bfloat16_traces_as_one_node():
    from torchain_amd import ops  # noqa: F401
    S, T, P = 4, 20, 100
    fst = synth.random_den_fst(256, 6, P, seed=5)
    graph = io.DenominatorGraph(fst, P).prepare(DEV)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=9, initial_probs=graph.initial_probs()))
    x = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=10)).to(DEV).to(torch.bfloat16)
    gp, sp = int(graph.ptr.value), int(sup.ptr.value)

    def step(a):
        out, _grad, _xgrad = torch.ops.torchain_amd.chain_step(a, a.new_empty((0,)), gp, sp, 5e-5, 0.1, 0.0, True, True)
        return out[3]

    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    a = x.clone().requires_grad_(True)
    loss = torch.compile(step, backend=backend, fullgraph=True)(a)
    loss.backward()
    assert len(graphs) == 1
    calls = [n for n in graphs[0].graph.nodes if n.op == "call_function" and "chain_step" in str(n.target)]
    assert len(calls) == 1, graphs[0].graph
    b = x.clone().requires_grad_(True)
    ref_loss, _ = chain_loss(b, graph, sup, 5e-5, 0.1)
    ref_loss.backward()
    _same_bits(loss.detach().reshape(1).to(torch.bfloat16), ref_loss.detach(), "loss")
    _same_bits(a.grad, b.grad, "grad")


@pytest.mark.parametrize("layout", ["3d", "2d"])
def test_bfloat16_step_replays_from_a_captured_graph(layout):
    S, T = 8, 30
    cfg, graph, sup, y, _ = _workload("C2", S, T)
    kw = dict(l2_regularize=5e-5, leaky_hmm_coefficient=cfg["leaky"], xent_regularize=0.1, kaldi_way=True)
    x = _layout(y, S, T, layout, torch.bfloat16)
    xe = (0.5 * x.detach()).requires_grad_(True)

    def step():
        loss, results = chain_loss(x, graph, sup, xent_input=xe, **kw)
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
    for seed in (21, 22):
        fresh = torch.randn(x.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
        with torch.no_grad():
            x.copy_(fresh)
            xe.copy_(0.25 * fresh)
        cg.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        want = step()
        for g, w_, what in zip(got, want, ("loss", "grad", "xent grad")):
            _same_bits(g, w_, what)


def test_data_parallel_wrapper_passes_half_through():
    """``parallel.chain_loss_data_parallel`` alone (no process group: the all-reduce of one rank) on bfloat16 input: the
    single-GPU call's results and gradients."""
    from torchain_amd import parallel
    w = _small_workload()
    S, T = w["S"], w["T"]
    kw = dict(l2_regularize=1e-3, leaky_hmm_coefficient=0.1, xent_regularize=0.1, kaldi_way=True)
    outs = []
    for fn in (chain_loss, parallel.chain_loss_data_parallel):
        a, b = _layout(w["y"], S, T, "3d", torch.bfloat16), _layout(w["xe"], S, T, "3d", torch.bfloat16)
        loss, res = fn(a, w["graph"], w["sup"], xent_input=b, **kw)
        loss.backward()
        outs.append((loss.detach(), res.data.clone(), a.grad, b.grad))
    # (the wrapper's loss is formed on the host from the reduced results, then stored in the input's dtype)
    assert outs[1][0].dtype == torch.bfloat16 and torch.allclose(outs[0][0].float(), outs[1][0].float(), rtol=1e-2)
    for i, what in ((1, "results"), (2, "grad"), (3, "xent grad")):
        _same_bits(outs[0][i], outs[1][i], what)


def test_mixed_dtypes_take_the_float32_path():
    w = _small_workload()
    S, T = w["S"], w["T"]
    kw = dict(l2_regularize=1e-3, leaky_hmm_coefficient=0.1, xent_regularize=0.1, kaldi_way=False)
    a, b = _layout(w["y"], S, T, "3d", torch.bfloat16), _layout(w["xe"], S, T, "3d", torch.float32)
    loss, res = chain_loss(a, w["graph"], w["sup"], xent_input=b, **kw)
    loss.backward()
    af, bf = a.detach().float().requires_grad_(True), b.detach().clone().requires_grad_(True)
    loss_f, res_f = chain_loss(af, w["graph"], w["sup"], xent_input=bf, **kw)
    loss_f.backward()
    assert loss.dtype == torch.float32 and a.grad.dtype == torch.bfloat16
    _same_bits(res.data, res_f.data, "results")
    _same_bits(a.grad, af.grad.to(torch.bfloat16), "grad")
    _same_bits(b.grad, bf.grad, "xent grad")


def test_non_contiguous_half_input_is_made_contiguous():
    w = _small_workload()
    S, T = w["S"], w["T"]
    base = _layout(w["y"], S, T, "3d", torch.bfloat16).detach()
    strided = base.transpose(0, 2).contiguous().transpose(0, 2).requires_grad_(True)  # (B, C, T) values, (T, C, B) memory
    assert not strided.is_contiguous()
    steps = lib.tc_debug_counter(b"den_launches")
    loss, res = chain_loss(strided, w["graph"], w["sup"], 1e-3, 0.1)
    loss.backward()
    assert lib.tc_debug_counter(b"den_launches") - steps == 1
    c = base.clone().requires_grad_(True)
    loss_c, res_c = chain_loss(c, w["graph"], w["sup"], 1e-3, 0.1)
    loss_c.backward()
    _same_bits(res.data, res_c.data, "results")
    _same_bits(strided.grad, c.grad, "grad")


def test_recipe_model_trains_under_autocast(tmp_path):
    """The recipe's pattern (tests/test_gpu_recipe.py) under ``torch.autocast("cuda", dtype=torch.bfloat16)``: the
    ``Conv1d`` heads emit bfloat16, ``chain_loss(..., xent_input, kaldi_way=True)`` takes them as they are, the loss falls,
    and once warm a step grows neither torch's allocator nor the library's pools."""
    import recipe_fixture as rf
    P = 32
    fst = synth.random_den_fst(120, 4, P, seed=3)
    scp = rf.write_learnable_set(tmp_path, fst, [20] * 32, seed=100, name="train")
    graph = io.DenominatorGraph(fst, P).prepare(DEV)
    egs = io.RandExample(scp, seed=1, batchsize=8)
    torch.manual_seed(0)
    model = rf.TwoLayerTdnn(P).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
    losses, allocated, pools = [], [], []
    for epoch in range(10):
        egs.reset()
        for (feats, ivec), sup in egs:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                mmi, xe = model(feats.to(DEV), ivec.to(DEV))
                assert mmi.dtype == torch.bfloat16 and xe.dtype == torch.bfloat16
                loss, res = chain_loss(mmi, graph, sup, l2_regularize=5e-5, leaky_hmm_coefficient=0.1,
                                       xent_regularize=0.1, xent_input=xe, kaldi_way=True)
            assert loss.dtype == torch.bfloat16
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=False)
            losses.append(float(res.loss))
        torch.cuda.synchronize()
        allocated.append(torch.cuda.memory_allocated())
        pools.append(int(lib.tc_debug_counter(b"pool_device_allocs")))
    assert np.isfinite(losses).all()
    first, last = np.mean(losses[:4]), np.mean(losses[-4:])
    assert last < 0.8 * first, (first, last, losses)
    assert allocated[-1] == allocated[3], allocated
    assert pools[-1] - pools[3] <= 2, pools  # (look-ahead timing may keep one more supervision alive: test_gpu_recipe.py)
