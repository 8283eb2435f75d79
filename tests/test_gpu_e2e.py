"""End-to-end supervisions on the GPU (num_e2e_kernels.hip through the C ABI and the Python layer), against the float64
reference of tests/e2e_reference.py with the repository's tolerances: scalars 1e-4 relative, derivatives matrix-wise
max |diff| <= 1e-4 * max(max |ref|, w)."""
import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import ChainResults, chain_loss, compute_chain_objf_and_deriv

import e2e_reference as ref
from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 60
REL = 1e-4


def _counter(name):
    return int(lib.tc_debug_counter(name.encode()))


_graphs = {}


def _den(P=P):
    """(HIP graph, oracle graph) of a small general den graph with P pdfs (cached per P)."""
    if P not in _graphs:
        from oracle import pyoracle
        pyoracle.build()
        fst = synth.random_den_fst(80, 4, P, seed=31)
        _graphs[P] = (io.DenominatorGraph(fst, P).prepare(0), pyoracle.DenGraph(fst))
    return _graphs[P]


def _y(S, T, P=P, seed=1, scale=2.0):
    return (np.random.default_rng(seed).normal(size=(S * T, P)) * scale).astype(np.float32)


def _hip(sup, y, l2=0.0, leaky=1e-5, xent=False, graph=None):
    graph = graph or _den(y.shape[1])[0]
    yt = torch.from_numpy(y).to(DEV)
    deriv = torch.full(yt.shape, 7.0, device=DEV)
    xd = torch.full(yt.shape, 7.0, device=DEV) if xent else None
    res = ChainResults()
    compute_chain_objf_and_deriv(graph, sup, yt, res.data, deriv, xd, l2, leaky, 0.1 if xent else 0.0)
    torch.cuda.synchronize()
    return res.data.numpy().copy(), deriv.cpu().numpy(), None if xd is None else xd.cpu().numpy()


def _check(got_res, got_d, want, w):
    assert abs(got_res[0] - want["objf"]) <= REL * abs(want["objf"]), (got_res, want["objf"])
    assert abs(got_res[1] - want["l2_term"]) <= REL * abs(want["l2_term"]) + 1e-30, (got_res, want["l2_term"])
    assert got_res[2] == np.float32(want["weight"])
    assert rel_err(got_d, want["deriv"], floor=w) <= REL


SHAPES = [(S, T) for S in (1, 7, 64, 256) for T in (1, 37, 150)]


@pytest.mark.parametrize("kind", ["chain", "random"])
@pytest.mark.parametrize("S,T,overlap", [s + (True,) for s in SHAPES] + [(7, 37, False), (64, 150, False), (256, 150, False)])
def test_objective_and_derivative_match_reference(kind, S, T, overlap, kernel_family):
    """Side stream (the default for batches that leave CUs idle: staged posteriors + scatter) and in-line order."""
    if not overlap:
        kernel_family("no_num_overlap")
    fsts = ref.batch(kind, S, P, seed=S * 1000 + T)
    if kind == "chain" and T < 12:  # (the chain family's shortest path is up to 9 arcs: short T exercise the random family)
        fsts = ref.batch("random", S, P, seed=S + T)
    w, l2, leaky = 0.7, 5e-4, 0.1
    y = _y(S, T, seed=S + T)
    sup = io.Supervision.from_e2e_fsts(w, T, P, fsts)
    staged = _counter("num_e2e_staged_launches")
    res, d, _ = _hip(sup, y, l2=l2, leaky=leaky)
    staged = _counter("num_e2e_staged_launches") - staged
    if not overlap:
        assert staged == 0
    elif S <= 64:  # (the small general den graph takes one CU per sequence: >= 16 CUs idle, so the side stream runs)
        assert staged == 1
    want = ref.e2e_objective(_den()[1], fsts, T, y, weight=w, l2=l2, leaky=leaky)
    assert want["ok"]
    _check(res, d, want, w)


def test_long_utterance_and_size_limit_sequence():
    """One utterance of 1200 frames, and a sequence at the size limit (2048 states, 8192 arcs, 1024 pdfs)."""
    T = 1200
    fsts = ref.batch("chain", 2, P, seed=5, words=12, max_phones=4)
    y = _y(2, T, seed=6)
    sup = io.Supervision.from_e2e_fsts(1.0, T, P, fsts)
    res, d, _ = _hip(sup, y, l2=1e-4, leaky=0.1)
    want = ref.e2e_objective(_den()[1], fsts, T, y, weight=1.0, l2=1e-4, leaky=0.1)
    _check(res, d, want, 1.0)

    PL, T = 1030, 20
    rng = np.random.default_rng(7)
    big = ref.random_fst(2048, 8192, PL, rng, pdf_pool=np.arange(1024))
    big[2][:1024] = rng.permutation(1024) + 1  # (every one of the 1024 pdfs present)
    assert len(big[5]) == 2048 and big[1][-1] == 8192 and len(set(big[2])) == 1024
    fsts = [big, ref.random_fst(5, 12, PL, rng)]
    y = _y(2, T, P=PL, seed=8)
    sup = io.Supervision.from_e2e_fsts(0.5, T, PL, fsts)
    res, d, _ = _hip(sup, y, graph=_den(PL)[0])
    want = ref.e2e_objective(_den(PL)[1], fsts, T, y, weight=0.5)
    _check(res, d, want, 0.5)


def test_xent_deriv_and_bit_identical_reruns():
    S, T, w = 16, 40, 0.9
    fsts = ref.batch("chain", S, P, seed=11)
    y = _y(S, T, seed=12)
    sup = io.Supervision.from_e2e_fsts(w, T, P, fsts)
    a = _hip(sup, y, l2=1e-4, leaky=0.1, xent=True)
    b = _hip(sup, y, l2=1e-4, leaky=0.1, xent=True)
    for x, z in zip(a, b):
        assert np.array_equal(x, z)
    want = ref.e2e_objective(_den()[1], fsts, T, y, weight=w, l2=1e-4, leaky=0.1)
    _check(a[0], a[1], want, w)
    assert rel_err(a[2], want["xent_deriv"], floor=w) <= REL


def test_soft_failure_on_an_infeasible_sequence():
    """A chain FST whose shortest path is longer than T in a batch of good ones: the whole minibatch takes Kaldi's
    failure route, objf = -10 * weight, deriv = -w * l2 * y, xent_deriv = 0, and nothing is NaN."""
    rng = np.random.default_rng(13)
    bad = ref.chain_fst(P, rng, words=4, max_phones=3, silence=False)
    T = ref.shortest_path_arcs(bad) - 1
    fsts = ref.batch("random", 5, P, seed=14)
    fsts = fsts[:2] + [bad] + fsts[2:]
    w, l2 = 0.8, 1e-3
    y = _y(len(fsts), T, seed=15)
    sup = io.Supervision.from_e2e_fsts(w, T, P, fsts)
    res, d, xd = _hip(sup, y, l2=l2, leaky=0.1, xent=True)
    want = ref.e2e_objective(_den()[1], fsts, T, y, weight=w, l2=l2, leaky=0.1)
    assert not want["ok"]
    assert res[0] == np.float32(-10.0 * w * len(fsts) * T)
    np.testing.assert_allclose(d, -w * l2 * y, rtol=1e-6, atol=0)
    assert not xd.any()


@pytest.mark.parametrize("kaldi_way", [True, False])
def test_chain_loss_three_d_xent_and_evaluation_step(kaldi_way):
    """chain_loss (tc_chain_step) with e2e supervisions: (B, C, T) input equals the 2-D input, the cross-entropy objective is
    sum(xent_input * w * gamma_num(input)), and the evaluation step (no_grad) reports the training step's values with no
    backward recursion of the denominator."""
    S, T, w = 8, 30, 1.0
    fsts = ref.batch("chain", S, P, seed=17)
    y = _y(S, T, seed=18)
    xe = _y(S, T, seed=19, scale=1.0)
    graph = _den()[0]
    sup = io.Supervision.from_e2e_fsts(w, T, P, fsts)
    kw = dict(l2_regularize=5e-5, leaky_hmm_coefficient=0.1, xent_regularize=0.1, kaldi_way=kaldi_way)
    y2, xe2 = torch.from_numpy(y).to(DEV), torch.from_numpy(xe).to(DEV)

    def bct(m):
        return m.view(T, S, P).permute(1, 2, 0).contiguous()

    out = {}
    for name, (a, b) in dict(two_d=(y2, xe2), three_d=(bct(y2), bct(xe2))).items():
        x, xx = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        loss, res = chain_loss(x, graph, sup, xent_input=xx, **kw)
        g = torch.autograd.grad(loss, x)[0]
        out[name] = (float(loss), res.data.numpy().copy(), res.xent_objf, g)
        before = _counter("den_backward_launches")
        with torch.no_grad():
            loss_e, res_e = chain_loss(a, graph, sup, xent_input=b, **kw)
        assert _counter("den_backward_launches") == before
        np.testing.assert_allclose(res_e.data.numpy(), out[name][1], rtol=1e-6)
        assert abs(res_e.xent_objf - out[name][2]) <= 1e-6 * abs(out[name][2])
        assert abs(float(loss_e) - out[name][0]) <= 1e-6 * abs(out[name][0])
    l2d, r2d, x2d, g2d = out["two_d"]
    l3d, r3d, x3d, g3d = out["three_d"]
    np.testing.assert_allclose(r3d, r2d, rtol=1e-6)
    assert abs(x3d - x2d) <= 1e-6 * abs(x2d)
    g3 = g3d.permute(2, 0, 1).reshape(S * T, P)
    assert rel_err(g3.cpu().numpy(), g2d.cpu().numpy()) <= 1e-6
    want = ref.e2e_objective(_den()[1], fsts, T, y if kaldi_way else xe, weight=w, l2=5e-5, leaky=0.1)
    assert abs(r2d[0] - want["objf"]) <= REL * abs(want["objf"])
    _, gamma = ref.num_logz(fsts, y.astype(np.float64), T)
    want_x = float((xe.astype(np.float64) * w * gamma).sum())
    assert abs(x2d - want_x) <= REL * abs(want_x)


def test_regular_path_unchanged_by_an_e2e_step_and_warm_steps_do_not_allocate():
    fst = synth.random_den_fst(80, 4, P, seed=31)
    graph = _den()[0]
    S, T = 8, 25
    rsup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=21, initial_probs=graph.initial_probs()))
    y = _y(S, T, seed=22)
    first = _hip(rsup, y, l2=1e-4, leaky=0.1, xent=True)
    fsts = ref.batch("chain", S, P, seed=23)
    for _ in range(2):
        _hip(io.Supervision.from_e2e_fsts(1.0, T, P, fsts), y, l2=1e-4, leaky=0.1, xent=True)
    again = _hip(rsup, y, l2=1e-4, leaky=0.1, xent=True)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    # warm: fresh e2e supervisions every step, no device allocation by the pool
    before = _counter("pool_device_allocs")
    for i in range(4):
        _hip(io.Supervision.from_e2e_fsts(1.0, T, P, fsts), y, l2=1e-4, leaky=0.1, xent=True)
    assert _counter("pool_device_allocs") == before


def test_captured_e2e_step_replays():
    S, T = 8, 30
    fsts = ref.batch("chain", S, P, seed=25)
    graph = _den()[0]
    sup = io.Supervision.from_e2e_fsts(1.0, T, P, fsts)
    kw = dict(l2_regularize=5e-5, leaky_hmm_coefficient=0.1, xent_regularize=0.1, kaldi_way=True)
    x = torch.from_numpy(_y(S, T, seed=26)).to(DEV).requires_grad_(True)
    xe = (0.5 * x.detach()).clone().requires_grad_(True)

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
    for seed in (27, 28):
        with torch.no_grad():
            x.copy_(torch.from_numpy(_y(S, T, seed=seed)).to(DEV))
            xe.copy_(0.5 * x)
        cg.replay()
        torch.cuda.synchronize()
        got = [c.clone() for c in captured]
        want = step()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def test_training_loop_from_e2e_egs(tmp_path):
    """e2e egs written to disk -> io.RandExample (native reader, look-ahead, merge, e2e handles) -> chain_loss -> SGD:
    the loss falls."""
    import e2e_egs_writer as ew
    torch.manual_seed(0)
    T, F, n = 30, 20, 24
    rng = np.random.default_rng(3)
    emb = rng.standard_normal((P, F))
    keyed = [("utt%02d" % i, ew.example(ref.chain_fst(P, rng, words=3, max_phones=3), T, P, F, seed=i, emb=emb))
             for i in range(n)]
    ark, scp = str(tmp_path / "e2e.ark"), str(tmp_path / "e2e.scp")
    ew.write_ark(ark, keyed, scp_path=scp, len_path=scp + ".len")
    graph = _den()[0]
    model = torch.nn.Conv1d(F, P, 1).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=0.02)
    losses = []
    for epoch in range(6):
        for (inp, _aux), sup in io.RandExample(scp, epoch, 8):
            assert sup.is_e2e
            loss, _ = chain_loss(model(inp.to(DEV)), graph, sup, l2_regularize=5e-5, leaky_hmm_coefficient=0.1)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss))
    assert np.isfinite(losses).all()
    assert np.mean(losses[-3:]) < 0.8 * np.mean(losses[:3]), losses
