"""Paths drawn from the denominator graph's posterior on the GPU (``csrc/den_sample_kernels.hip`` through
``io.DenominatorGraph.sample_paths`` / ``functions.den_sample_paths``) against ``tests/den_sample_reference.py``:

* the selection rule path for path: with the same uniforms every sample that the reference does not flag as a close call
  (a threshold within ``delta(T) = 16 (T + 2) 2^-24`` of an end of the chosen interval) equals the reference's exactly;
* every sample, flagged or not, is a latent path of the graph;
* the pdf occupancies of 4096 samples lie within 5 sigma of the float64 posteriors;
* batches, sample counts, generators, ragged lengths, layouts and dtypes, the form that reads the previous frame from the
  workspace, the workspace cap, non-finite inputs, an untouched graph handle and allocation-free warm calls are held bit
  for bit;
* ``functions.sampled_risk_surrogate`` on the GPU's samples reproduces ``den_expected_accuracy``'s gradient in projection."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss, den_expected_accuracy, den_sample_paths, sampled_risk_surrogate

import den_accuracy_reference as dar
import den_sample_reference as dsr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TC_ERR_INVALID_ARGUMENT = -1
TC_ERR_WORKSPACE = -4
# 4 * Hs + 1024 <= 163840 (include/torchain_hip.h): the largest graph whose alpha' stays in LDS
RESIDENT_MAX_STATES = (160 * 1024 - 1024) // 4


def _counter(key):
    return int(lib.tc_debug_counter(key))


def _counters():
    return _counter(b"den_sample_launches"), _counter(b"den_sample_streamed_launches"), _counter(b"den_launches")


@functools.lru_cache(maxsize=None)
def _graph(kind):
    fst = {
        "random": lambda: synth.random_den_fst(300, 5, 100, seed=32),
        "nearly_tied": lambda: synth.nearly_tied_den_fst(500, 5, 90, seed=7),
        "skewed_tied": lambda: synth.skewed_tied_den_fst(400, 7000, 150, seed=8),  # hub states: long incoming lists
        "skewed": lambda: synth.skewed_den_fst(300, 6000, 120, seed=4),
        "small": lambda: synth.random_den_fst(30, 4, 10),
    }[kind]()
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    return fst, graph, dsr.tables(fst, graph.initial_probs())


def _uniforms(seed, *shape):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. the rule, path for path; 2. every sample is a latent path ----
@functools.lru_cache(maxsize=None)
def _rule_case(kind, leaky):
    """The inputs of a case and the reference's samples (computed once, on the CPU)."""
    fst, graph, tab = _graph(kind)
    S, T, K = 3, 11, 64
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=41)
    u = _uniforms(61, S, K, T + 1, 3)
    return y, u, dsr.batch(tab, y, S, leaky, u)


@pytest.mark.parametrize("leaky", [1e-5, 0.1])
@pytest.mark.parametrize("kind", ["random", "nearly_tied", "skewed_tied", "skewed"])
def test_unflagged_samples_equal_the_reference(kind, leaky):
    fst, graph, tab = _graph(kind)
    S, T, K = 3, 11, 64
    y, u, (want_pdfs, want_states, close, leaks) = _rule_case(kind, leaky)
    # conditions on the reference, before the GPU is looked at
    print("%s, c = %g: %d of %d samples flagged, %d leaks" % (kind, leaky, close.sum(), close.size, leaks.sum()))
    assert (want_pdfs >= 0).all() and (want_states >= 0).all()
    assert close.sum() <= 0.10 * close.size
    assert (leaks.sum() > 0) if leaky == 0.1 else (leaks.sum() == 0)
    before = _counters()
    pdfs, states = graph.sample_paths(_dev(y), K, n_batch=S, leaky_hmm_coefficient=leaky, uniforms=_dev(u), return_states=True)
    assert _counters() == (before[0] + 1, before[1], before[2])
    assert pdfs.dtype == torch.int32 and pdfs.shape == (S, K, T)
    assert states.dtype == torch.int32 and states.shape == (S, K, T + 1, 2)
    pdfs, states = pdfs.cpu().numpy(), states.cpu().numpy()
    differ = (pdfs != want_pdfs).any(axis=2) | (states != want_states).any(axis=(2, 3))
    print("%d samples differ from the reference, all of them flagged: %s" % (differ.sum(), bool((~differ | close).all())))
    assert (~differ | close).all()
    for s in range(S):
        for k in range(K):
            assert dsr.valid_sample(tab, pdfs[s, k], states[s, k], leaky), (s, k)
    # the same samples at every call, and through the other entry (which returns no states unless asked)
    again = den_sample_paths(_dev(y), graph, K, n_batch=S, leaky_hmm_coefficient=leaky, uniforms=_dev(u))
    assert isinstance(again, torch.Tensor) and np.array_equal(again.cpu().numpy(), pdfs)


def test_no_leak_without_the_coefficient():
    fst, graph, tab = _graph("skewed_tied")
    S, T, K = 2, 9, 48
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=42)
    pdfs, states = graph.sample_paths(_dev(y), K, n_batch=S, leaky_hmm_coefficient=0.0, uniforms=_dev(_uniforms(62, S, K, T + 1, 3)),
                                      return_states=True)
    pdfs, states = pdfs.cpu().numpy(), states.cpu().numpy()
    assert (states[..., 0] == states[..., 1]).all()
    assert all(dsr.valid_sample(tab, pdfs[s, k], states[s, k], 0.0) for s in range(S) for k in range(K))


# ---- 3. statistics ----
def test_occupancies_follow_the_posteriors():
    fst, graph, tab = _graph("small")
    T, K, P, leaky = 4, 4096, fst.num_pdfs, 0.1
    y = synth.random_nnet_output(1, T, P, seed=43)
    gamma = dar.recursion(dar.arcs_of(fst, tab[3]), tab[4], y, np.zeros(T, np.int64), None, leaky)["gamma"]
    sigma = np.sqrt(np.maximum(gamma * (1.0 - gamma), 1e-300) / K)

    def worst(pdfs):
        occ = np.stack([np.bincount(pdfs[:, t], minlength=P) for t in range(T)]) / K
        z = np.abs(occ - gamma) / sigma
        z[(gamma == 0) & (occ == 0)] = 0.0
        return float(z.max())

    gen = torch.Generator(device=DEV)
    gen.manual_seed(2024)
    u = torch.rand((1, K, T + 1, 3), generator=gen, device=DEV)
    # the reference's outcome for that seed first
    ref_pdfs = dsr.batch(tab, y, 1, leaky, u.cpu().numpy())[0]
    print("reference: worst occupancy %.2f sigma" % worst(ref_pdfs[0]))
    assert worst(ref_pdfs[0]) <= 5.0
    gen.manual_seed(2024)
    pdfs = graph.sample_paths(_dev(y), K, n_batch=1, leaky_hmm_coefficient=leaky, generator=gen)
    assert torch.equal(pdfs, graph.sample_paths(_dev(y), K, n_batch=1, leaky_hmm_coefficient=leaky, uniforms=u))
    print("GPU: worst occupancy %.2f sigma" % worst(pdfs[0].cpu().numpy()))
    assert worst(pdfs[0].cpu().numpy()) <= 5.0
    # the same seed twice: the same output; another seed: another
    gen.manual_seed(2024)
    assert torch.equal(den_sample_paths(_dev(y), graph, K, n_batch=1, leaky_hmm_coefficient=leaky, generator=gen), pdfs)
    gen.manual_seed(2025)
    assert not torch.equal(den_sample_paths(_dev(y), graph, K, n_batch=1, leaky_hmm_coefficient=leaky, generator=gen), pdfs)


# ---- 4. bit-for-bit properties ----
def test_a_sequence_and_a_sample_do_not_depend_on_the_call():
    fst, graph, tab = _graph("nearly_tied")
    S, T, K, P, leaky = 3, 10, 24, fst.num_pdfs, 0.1
    y = synth.random_nnet_output(S, T, P, seed=44)
    u = _uniforms(63, S, K, T + 1, 3)
    whole = graph.sample_paths(_dev(y), K, n_batch=S, leaky_hmm_coefficient=leaky, uniforms=_dev(u), return_states=True)
    assert bool((whole[0] >= 0).all())
    for s in range(S):  # alone
        one = graph.sample_paths(_dev(y[s::S]), K, n_batch=1, leaky_hmm_coefficient=leaky, uniforms=_dev(u[s:s + 1]), return_states=True)
        assert _same(one, [o[s:s + 1] for o in whole])
    perm = [2, 0, 1]  # at another place
    yp = np.stack([y[s::S] for s in perm], axis=1).reshape(T * S, P)
    moved = graph.sample_paths(_dev(yp), K, n_batch=S, leaky_hmm_coefficient=leaky, uniforms=_dev(u[perm]), return_states=True)
    assert _same(moved, [o[perm] for o in whole])
    # the first k samples of a K-sample call are a k-sample call; so is any sample given its uniforms
    for k in (1, 5, 17):  # (17: a wave takes a second sample)
        fewer = graph.sample_paths(_dev(y), k, n_batch=S, leaky_hmm_coefficient=leaky, uniforms=_dev(u[:, :k]), return_states=True)
        assert _same(fewer, [o[:, :k] for o in whole])
    last = graph.sample_paths(_dev(y), 2, n_batch=S, leaky_hmm_coefficient=leaky, uniforms=_dev(u[:, K - 2:]), return_states=True)
    assert _same(last, [o[:, K - 2:] for o in whole])


@pytest.mark.parametrize("kind", ["random", "skewed"])
def test_ragged_batch_matches_single_sequences(kind):
    fst, graph, tab = _graph(kind)
    frames = np.array([11, 3, 7, 1], np.int32)
    S, T, K, P, leaky = len(frames), int(frames.max()), 20, fst.num_pdfs, 0.1
    y = synth.random_nnet_output(S, T, P, seed=45)
    for s in range(S):
        y[s::S][frames[s]:] = np.nan  # every padding frame
    u = _uniforms(64, S, K, T + 1, 3)
    pdfs, states = graph.sample_paths(_dev(y), K, frames=frames, leaky_hmm_coefficient=leaky, uniforms=_dev(u), return_states=True)
    want = dsr.batch(tab, y, S, leaky, u, frames)
    for s in range(S):
        Ts = int(frames[s])
        assert bool((pdfs[s, :, Ts:] == -1).all()) and bool((states[s, :, Ts + 1:] == -1).all())
        assert bool((pdfs[s, :, :Ts] >= 0).all()) and bool((states[s, :, :Ts + 1] >= 0).all())
        # alone, as a batch of its own length: row t of its uniforms is row t here
        one = graph.sample_paths(_dev(y[s::S][:Ts]), K, n_batch=1, leaky_hmm_coefficient=leaky, uniforms=_dev(u[s:s + 1, :, :Ts + 1]),
                                 return_states=True)
        assert torch.equal(one[0][0], pdfs[s, :, :Ts]) and torch.equal(one[1][0], states[s, :, :Ts + 1])
        ok = ~want[2][s]
        assert np.array_equal(pdfs[s].cpu().numpy()[ok], want[0][s][ok]) and np.array_equal(states[s].cpu().numpy()[ok], want[1][s][ok])
    # lengths as an int tensor on the device, (B, C, T) layout
    x = _dev(np.stack([y[s::S].T for s in range(S)]))
    assert _same(den_sample_paths(x, graph, K, frames=_dev(frames), leaky_hmm_coefficient=leaky, uniforms=_dev(u), return_states=True),
                 (pdfs, states))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_bct_layout_and_dtypes_match_the_2d_float32_call(dtype):
    fst, graph, tab = _graph("nearly_tied")
    S, T, K, P = 3, 10, 16, fst.num_pdfs
    x = _dev(synth.random_nnet_output(S, T, P, seed=46, scale=2.0).reshape(T, S, P)).permute(1, 2, 0).contiguous().to(dtype)
    y2d = x.float().permute(2, 0, 1).reshape(T * S, P).contiguous()  # the gathered float32 rows
    u = _dev(_uniforms(65, S, K, T + 1, 3))
    want = graph.sample_paths(y2d, K, n_batch=S, uniforms=u, return_states=True)
    assert bool((want[0] >= 0).all())
    assert _same(graph.sample_paths(x, K, uniforms=u, return_states=True), want)
    # a row stride beyond the columns: the gap is not read
    wide = torch.full((S * T, P + 5), float("nan"), device=DEV)
    wide[:, :P] = y2d
    assert _same(graph.sample_paths(wide[:, :P], K, n_batch=S, uniforms=u, return_states=True), want)


@pytest.mark.parametrize("kind", ["random", "skewed_tied"])
def test_both_forms_give_the_same_bits(kernel_family, kind):
    fst, graph, tab = _graph(kind)
    S, T, K = 3, 11, 20
    frames = [11, 4, 8]
    y = _dev(synth.random_nnet_output(S, T, fst.num_pdfs, seed=47))
    u = _dev(_uniforms(66, S, K, T + 1, 3))
    before = _counters()
    resident = graph.sample_paths(y, K, frames=frames, leaky_hmm_coefficient=0.1, uniforms=u, return_states=True)
    assert _counters() == (before[0] + 1, before[1], before[2])  # the streamed counter moves only when forced
    kernel_family("force_den_sample_streamed")
    streamed = graph.sample_paths(y, K, frames=frames, leaky_hmm_coefficient=0.1, uniforms=u, return_states=True)
    assert _counters() == (before[0] + 2, before[1] + 1, before[2])
    assert _same(streamed, resident) and bool((resident[0][0] >= 0).all())


@pytest.mark.parametrize("H, streamed", [(RESIDENT_MAX_STATES, False), (RESIDENT_MAX_STATES + 1, True)])
def test_graphs_either_side_of_the_lds_budget(kernel_family, H, streamed):
    """Each on the form it takes by itself; the samples are the reference's either way.  (No cap on the flagged samples here:
    with 40 000 states an interval of the last-state pick is about 2.5e-5 of the total and delta(5) = 6.7e-6 lies on either
    side of each end, so about half the samples are close calls by that pick alone.  A quarter at least must be left.)"""
    kernel_family("force_streamed")  # (the denominator's own tables: built in a fraction of a second; not what is tested)
    fst = synth.random_den_fst(H, 3, 700, seed=31)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    tab = dsr.tables(fst, graph.initial_probs())
    S, T, K, leaky = 2, 5, 24, 0.1
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=50)
    u = _uniforms(73, S, K, T + 1, 3)
    want_pdfs, want_states, close, leaks = dsr.batch(tab, y, S, leaky, u)
    print("%d states: %d of %d samples flagged, %d leaks" % (H, close.sum(), close.size, leaks.sum()))
    assert (~close).sum() >= close.size // 4 and leaks.sum() > 0
    before = _counters()
    pdfs, states = graph.sample_paths(_dev(y), K, n_batch=S, leaky_hmm_coefficient=leaky, uniforms=_dev(u), return_states=True)
    torch.cuda.synchronize()
    assert _counters() == (before[0] + 1, before[1] + int(streamed), before[2])
    pdfs, states = pdfs.cpu().numpy(), states.cpu().numpy()
    differ = (pdfs != want_pdfs).any(axis=2) | (states != want_states).any(axis=(2, 3))
    assert (~differ | close).all()
    assert all(dsr.valid_sample(tab, pdfs[s, k], states[s, k], leaky) for s in range(S) for k in range(K))


def test_workspace_cap_runs_groups_with_the_same_bits():
    fst, graph, tab = _graph("random")
    S, T, K, P = 5, 9, 12, fst.num_pdfs
    frames = [9, 2, 5, 9, 7]
    y = _dev(synth.random_nnet_output(S, T, P, seed=48))
    u = _dev(_uniforms(67, S, K, T + 1, 3))
    whole = graph.sample_paths(y, K, frames=frames, uniforms=u, return_states=True)
    cap = int(lib.tc_den_sample_paths_workspace_bytes(graph.ptr, 2, T))  # two sequences a group: 2 + 2 + 1
    assert int(lib.tc_den_sample_paths_workspace_bytes(graph.ptr, 3, T)) > cap
    before = _counters()
    assert _same(graph.sample_paths(y, K, frames=frames, uniforms=u, return_states=True, max_workspace_bytes=cap), whole)
    assert _counters() == (before[0] + 3, before[1], before[2])
    ws = torch.empty(cap + 100, dtype=torch.uint8, device=DEV)  # a workspace tensor of the caller's caps the same way
    x = y.reshape(T, S, P).permute(1, 2, 0).contiguous()
    assert _same(den_sample_paths(x, graph, K, frames=frames, uniforms=u, return_states=True, workspace=ws), whole)
    assert _counters() == (before[0] + 6, before[1], before[2])
    with pytest.raises(ValueError, match="one sequence needs"):
        graph.sample_paths(y, K, frames=frames, uniforms=u, max_workspace_bytes=1000)


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_input_fails_its_sequence_alone(value):
    fst, graph, tab = _graph("skewed_tied")
    S, T, K, P = 3, 8, 10, fst.num_pdfs
    frames = [8, 6, 8]
    y = _dev(synth.random_nnet_output(S, T, P, seed=49))
    u = _dev(_uniforms(68, S, K, T + 1, 3))
    clean = graph.sample_paths(y, K, frames=frames, uniforms=u, return_states=True)
    bad = y.clone()
    bad[4 * S + 1, P - 1] = value  # a valid frame of sequence 1
    bad[7 * S + 1, 0] = float("nan")  # ... and a padding frame of it, which nobody reads
    got = graph.sample_paths(bad, K, frames=frames, uniforms=u, return_states=True)
    assert bool((got[0][1] == -1).all()) and bool((got[1][1] == -1).all())
    for s in (0, 2):
        assert _same([o[s] for o in got], [o[s] for o in clean])
    assert bool((clean[0][1, :, :6] >= 0).all())
    # the surrogate gives the failed sequence 0 and no gradient
    x = bad.clone().requires_grad_(True)
    value_ = sampled_risk_surrogate(x, got[0], torch.rand(S, K, device=DEV), frames=frames)
    value_.sum().backward()
    assert float(value_.detach()[1]) == 0.0 and bool((x.grad.view(T, S, P)[:, 1] == 0).all())


def _step(den, sup, y):
    x = y.clone().requires_grad_(True)
    loss, res = chain_loss(x, den, sup, l2_regularize=5e-4, leaky_hmm_coefficient=0.1)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), res.data.clone(), x.grad.clone()


def test_training_step_is_the_same_after_the_call():
    fst = synth.random_den_fst(300, 5, 100, seed=32)
    den = io.DenominatorGraph(fst, fst.num_pdfs)  # a handle of this test's own: the first sample_paths call on it is made here
    S, T, K = 4, 12, 8
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=52))
    y = _dev(synth.random_nnet_output(S, T, fst.num_pdfs, seed=53))
    u = _dev(_uniforms(69, S, K, T + 1, 3))
    first = _step(den, sup, y)
    before = _counters()
    whole = den.sample_paths(y, K, n_batch=S, leaky_hmm_coefficient=0.1, uniforms=u, return_states=True)
    torch.cuda.synchronize()
    assert _counters() == (before[0] + 1, before[1], before[2]) and bool((whole[0] >= 0).all())
    second = _step(den, sup, y)
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert _same(den.sample_paths(y, K, n_batch=S, leaky_hmm_coefficient=0.1, uniforms=u, return_states=True), whole)


def test_warm_calls_allocate_nothing():
    fst, graph, tab = _graph("random")
    S, T, K, P = 4, 10, 8, fst.num_pdfs
    y = _dev(synth.random_nnet_output(S, T, P, seed=54))
    u = _dev(_uniforms(70, S, K, T + 1, 3))
    ws = torch.empty(int(lib.tc_den_sample_paths_workspace_bytes(graph.ptr, S, T)), dtype=torch.uint8, device=DEV)
    first = graph.sample_paths(y, K, n_batch=S, uniforms=u, return_states=True, workspace=ws)
    torch.cuda.synchronize()
    level = torch.cuda.memory_allocated(), _counter(b"pool_device_allocs")  # (the outputs of `first` are part of the level)
    for _ in range(3):
        got = graph.sample_paths(y, K, n_batch=S, uniforms=u, return_states=True, workspace=ws)
        torch.cuda.synchronize()
        assert _same(got, first)
        del got
        assert (torch.cuda.memory_allocated(), _counter(b"pool_device_allocs")) == level


# ---- 5. the ABI ----
def test_abi_refuses_bad_arguments_and_runs_good_ones():
    fst, graph, tab = _graph("random")
    S, T, K, P = 2, 5, 3, fst.num_pdfs
    need = int(lib.tc_den_sample_paths_workspace_bytes(graph.ptr, S, T))
    y = _dev(synth.random_nnet_output(S, T, P, seed=55))
    u = _dev(_uniforms(71, S, K, T + 1, 3))
    pdfs = torch.full((S, K, T), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def call(g=graph.ptr, s=S, yp=ptr(y), rows=S * T, cols=P, stride=P, fr=None, t=T, leaky=1e-5, k=K, up=ptr(u), pp=ptr(pdfs),
             st=None, wp=ptr(ws), nbytes=need):
        return lib.tc_den_sample_paths(g, s, yp, rows, cols, stride, fr, t, leaky, k, up, pp, st, wp, nbytes, 0, None)

    before = _counters()
    for kwargs in (dict(g=None), dict(yp=None), dict(up=None), dict(pp=None), dict(s=0), dict(t=0), dict(k=0),
                   dict(rows=S * T + 1), dict(cols=P + 1), dict(stride=P - 1), dict(leaky=-0.5), dict(leaky=float("inf")),
                   dict(leaky=float("nan")), dict(yp=ptr(y, 2)), dict(fr=ptr(y, 2)), dict(up=ptr(u, 1)), dict(pp=ptr(pdfs, 2)),
                   dict(st=ptr(pdfs, 2))):
        assert call(**kwargs) == TC_ERR_INVALID_ARGUMENT, kwargs
    for kwargs in (dict(wp=None), dict(wp=ptr(ws, 4)), dict(nbytes=need - 1)):
        assert call(**kwargs) == TC_ERR_WORKSPACE, kwargs
    torch.cuda.synchronize()
    assert _counters() == before and bool((pdfs == -7).all())  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert _counters() == (before[0] + 1, before[1], before[2])
    assert torch.equal(pdfs, graph.sample_paths(y, K, n_batch=S, uniforms=u))


# ---- 6. the surrogate ----
def test_surrogate_reproduces_the_exact_smbr_gradient_in_projection():
    fst, graph, tab = _graph("random")
    S, T, K, P, leaky = 2, 8, 2048, fst.num_pdfs, 0.1
    frames = [8, 6]
    y, refs, exact = np.zeros((T * S, P), np.float32), np.full((S, T), -1, np.int32), []
    for s in range(S):
        ys, ref, ex = dsr.boosted_reference(fst, tab, frames[s], leaky, path_seed=9 + s, y_seed=21 + s)
        assert 0.3 <= ex["acc"] / frames[s] <= 0.7
        y[s::S][:frames[s]], refs[s, :frames[s]] = ys, ref
        exact.append(ex)
    y[1::S][frames[1]:] = 3.0  # (the padding frames of sequence 1: finite, so that a gradient there would show)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    x = _dev(y).requires_grad_(True)
    pdfs = den_sample_paths(x, graph, K, frames=frames, leaky_hmm_coefficient=leaky, generator=gen)
    risks = (pdfs == _dev(refs).unsqueeze(1)).sum(dim=2)  # the frame accuracy of each path (padding: -1 == -1 is constant)
    value = sampled_risk_surrogate(x, pdfs, risks, frames=frames)
    assert value.dtype == torch.float64 and value.shape == (S,)
    value.sum().backward()
    got = x.grad.cpu().numpy()
    xe = _dev(y).requires_grad_(True)
    den_expected_accuracy(xe, graph, _dev(refs), frames=frames, leaky_hmm_coefficient=leaky).sum().backward()
    want = xe.grad.cpu().numpy()
    for s in range(S):
        Ts = frames[s]
        assert np.abs(want[s::S][:Ts] - exact[s]["grad"]).max() <= 1e-5 * np.abs(exact[s]["grad"]).max()  # (the exact side is)
        sampled = pdfs[s, :, :Ts].cpu().numpy()
        r = (sampled == refs[s, :Ts][None]).sum(axis=1).astype(np.float64)
        terms = dsr.estimator_terms(sampled, r, Ts, P)
        tol = (K + 2) * 2.0 ** -24 * np.abs(terms).mean(axis=0)
        assert (np.abs(got[s::S][:Ts] - terms.mean(axis=0)) <= tol).all()  # the surrogate's gradient is the stated estimator
        for i, (est, ex, se) in enumerate(dsr.projections(terms, want[s::S][:Ts].astype(np.float64))):
            print("sequence %d, direction %d: estimate %+.5f, exact %+.5f, z = %+.2f" % (s, i, est, ex, (est - ex) / se))
            assert abs(est - ex) <= 5.0 * se
    pad = got[1::S][frames[1]:]
    assert (pad == 0).all() and not np.signbit(pad).any()  # exactly +0 in padding rows


def test_surrogate_gradient_is_zero_outside_the_clamp():
    fst, graph, tab = _graph("random")
    S, T, K, P = 2, 6, 64, fst.num_pdfs
    y = synth.random_nnet_output(S, T, P, seed=56)
    u = _dev(_uniforms(72, S, K, T + 1, 3))
    j = int(graph.sample_paths(_dev(y), K, n_batch=S, uniforms=u)[0, 0, 2])  # a pdf that paths of sequence 0 emit in frame 2
    y[2 * S + 0, j] = 35.0
    x = _dev(y).requires_grad_(True)
    pdfs = den_sample_paths(x, graph, K, n_batch=S, uniforms=u)
    assert int((pdfs[0, :, 2] == j).sum()) >= 2  # (sampled: the clamp is what keeps the gradient away)
    risks = torch.arange(K, device=DEV, dtype=torch.float64).repeat(S, 1)
    sampled_risk_surrogate(x, pdfs, risks).sum().backward()
    g = x.grad.cpu().numpy()
    assert g[2 * S + 0, j] == 0 and not np.signbit(g[2 * S + 0, j]) and np.abs(g).max() > 0
