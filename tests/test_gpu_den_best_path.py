"""The best path through the denominator graph on the GPU (``csrc/den_best_path_kernels.hip`` through
``io.DenominatorGraph.best_path`` / ``functions.den_best_path``) against the float64 Viterbi of
``tests/den_best_path_reference.py``.  For every sequence:

* the returned states and pdfs are a path of the FST (every consecutive pair is an arc carrying that pdf, ``pi(h_0) > 0``);
* ``|score - rescore(path)| <= T_s * 2^-23 * M``, the bound of ``include/torchain_hip.h``: the kernel's running score is
  float32, one add and one max per arc, on float32 table entries the reference shares; ``M`` is the largest running
  ``|score|`` along the returned path, taken from the float64 rescoring;
* ``score >= reference optimum - bound``.

Ties, ragged batches, layouts and dtypes, the form that reads the previous frame from the workspace, the workspace cap,
non-finite inputs, an untouched graph handle and allocation-free warm calls are held bit for bit."""
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import chain_loss, den_best_path

import den_best_path_reference as dbp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# 8 * Hs + 1024 <= 163840 (include/torchain_hip.h): the largest graph whose previous frame stays in LDS
RESIDENT_MAX_STATES = (160 * 1024 - 1024) // 8


def _counter(key):
    return int(lib.tc_debug_counter(key))


@functools.lru_cache(maxsize=None)
def _graph(kind):
    fst = {
        "random": lambda: synth.random_den_fst(300, 5, 100, seed=32),
        "nearly_tied": lambda: synth.nearly_tied_den_fst(500, 5, 90, seed=7),
        "skewed_tied": lambda: synth.skewed_tied_den_fst(400, 7000, 150, seed=8),  # hub states: long incoming lists
        "skewed": lambda: synth.skewed_den_fst(300, 6000, 120, seed=4),
    }[kind]()
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    return fst, graph, graph.initial_probs()


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _seq(y2d, S, s, frames=None):
    """Sequence ``s`` of the frame-major matrix ``y2d`` (numpy, row t*S + s): its own ``(T_s, P)`` rows."""
    rows = y2d[s::S]
    return rows if frames is None else rows[:frames]


def _check(fst, pi, y2d, S, out, frames=None):
    """The three assertions of the module's docstring for every sequence; returns the reference's paths."""
    pdfs, scores, states = (o.cpu().numpy() for o in out)
    T = pdfs.shape[1]
    refs = []
    for s in range(S):
        Ts = T if frames is None else int(frames[s])
        y = _seq(y2d, S, s, Ts)
        assert (pdfs[s, Ts:] == -1).all() and (states[s, Ts + 1:] == -1).all()
        assert (pdfs[s, :Ts] >= 0).all() and (states[s, :Ts + 1] >= 0).all()
        exact, peak = dbp.rescore(fst, pi, states[s, :Ts + 1], pdfs[s, :Ts], y, running=True)
        assert exact > -np.inf, "sequence %d: not a path of the graph" % s
        bound = dbp.bound(Ts, peak)
        ref = dbp.viterbi(fst, pi, y)
        print("sequence %d: score %.9g, rescored %.9g, optimum %.9g, bound %.3g" % (s, scores[s], exact, ref[2], bound))
        assert abs(scores[s] - exact) <= bound
        assert scores[s] >= ref[2] - bound
        refs.append(ref)
    return refs


# ---- 1. graph families ----
@pytest.mark.parametrize("kind", ["random", "nearly_tied", "skewed_tied", "skewed"])
def test_path_is_valid_and_optimal_to_the_bound(kind):
    fst, graph, pi = _graph(kind)
    S, T = 3, 11
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=41)
    before = _counter(b"den_best_path_launches"), _counter(b"den_best_path_streamed_launches")
    out = graph.best_path(torch.from_numpy(y).to(DEV), n_batch=S, return_states=True)
    assert (_counter(b"den_best_path_launches"), _counter(b"den_best_path_streamed_launches")) == (before[0] + 1, before[1])
    assert out[0].dtype == torch.int32 and out[0].shape == (S, T) and out[2].dtype == torch.int32 and out[2].shape == (S, T + 1)
    assert out[1].dtype == torch.float64 and out[1].shape == (S,)
    _check(fst, pi, y, S, out)
    # the same path at every call, and through the other entry (which returns no states unless asked)
    again = den_best_path(torch.from_numpy(y).to(DEV), graph, n_batch=S)
    assert len(again) == 2 and _same(again, out[:2])


# ---- 2. planted path ----
def test_planted_path_is_returned_exactly():
    fst, graph, pi = _graph("random")
    S, T = 3, 11
    rng = np.random.default_rng(5)
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=42)
    planted = []
    for s in range(S):
        # On the CPU, with the reference alone: the planted path beats every other by more than the bound.  A boost on y
        # cannot separate two paths that emit the same pdfs (another first state entering h_1 on the same forward pdf): such a
        # draw is made again.
        done = False
        for _ in range(200):
            states, pdfs = dbp.random_path(fst, pi, T, rng)
            for boost in (20.0, 40.0, 80.0):
                ys = _seq(y, S, s).copy()
                ys[np.arange(T), pdfs] += np.float32(boost)
                exact, peak = dbp.rescore(fst, pi, states, pdfs, ys, running=True)
                done = exact - dbp.runner_up(fst, pi, ys, states, pdfs) > 2 * dbp.bound(T, peak)
                if done:
                    break
            if done:
                break
        assert done, "no separable path drawn"
        y[s::S] = ys
        ref = dbp.viterbi(fst, pi, ys)
        assert (ref[0] == states).all() and (ref[1] == pdfs).all()
        planted.append((states, pdfs))
    out = graph.best_path(torch.from_numpy(y).to(DEV), n_batch=S, return_states=True)
    _check(fst, pi, y, S, out)
    for s, (states, pdfs) in enumerate(planted):
        assert (out[0][s].cpu().numpy() == pdfs).all() and (out[2][s].cpu().numpy() == states).all()


# ---- 3. ragged ----
@pytest.mark.parametrize("kind", ["random", "skewed"])
def test_ragged_batch_matches_single_sequences_bit_for_bit(kind):
    fst, graph, pi = _graph(kind)
    frames = np.array([11, 3, 7, 1], np.int32)
    S, T, P = len(frames), int(frames.max()), fst.num_pdfs
    y = synth.random_nnet_output(S, T, P, seed=43)
    for s in range(S):
        y[s::S][frames[s]:] = np.nan  # every padding frame
    out = graph.best_path(torch.from_numpy(y).to(DEV), frames=frames, return_states=True)
    _check(fst, pi, y, S, out, frames)
    single = []
    for s in range(S):
        Ts = int(frames[s])
        one = graph.best_path(torch.from_numpy(np.ascontiguousarray(_seq(y, S, s, Ts))).to(DEV), n_batch=1, return_states=True)
        single.append(one)
        assert torch.equal(out[0][s, :Ts], one[0][0]) and torch.equal(out[2][s, :Ts + 1], one[2][0])
        assert torch.equal(_bits(out[1][s:s + 1]), _bits(one[1]))
        assert bool((out[0][s, Ts:] == -1).all()) and bool((out[2][s, Ts + 1:] == -1).all())
    # the sequences permuted, lengths as an int tensor on the device, (B, C, T) layout: the same bits per sequence
    perm = [2, 0, 3, 1]
    x = torch.from_numpy(np.stack([_seq(y, S, s).T for s in perm])).to(DEV)  # (S, P, T)
    out2 = den_best_path(x, graph, frames=torch.from_numpy(frames[perm]).to(DEV), return_states=True)
    for i, s in enumerate(perm):
        assert _same([o[i] for o in out2], [o[s] for o in out])


# ---- 4. layouts and dtypes ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_bct_layout_and_dtypes_match_the_2d_float32_call(dtype):
    fst, graph, pi = _graph("nearly_tied")
    S, T, P = 3, 10, fst.num_pdfs
    x = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=44, scale=2.0).reshape(T, S, P)).to(DEV)
    x = x.permute(1, 2, 0).contiguous().to(dtype)  # (S, P, T)
    y2d = x.float().permute(2, 0, 1).reshape(T * S, P).contiguous()
    want = graph.best_path(y2d, n_batch=S, return_states=True)
    _check(fst, pi, y2d.cpu().numpy(), S, want)
    assert _same(graph.best_path(x, return_states=True), want)
    # a view of another layout goes through a copy and gives the same
    assert _same(graph.best_path(x.transpose(1, 2).contiguous().transpose(1, 2), return_states=True), want)


def test_row_stride_beyond_the_columns_is_not_read():
    fst, graph, pi = _graph("random")
    S, T, P = 3, 9, fst.num_pdfs
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=45)).to(DEV)
    wide = torch.full((S * T, P + 5), float("nan"), device=DEV)  # sentinel NaNs in the gap
    wide[:, :P] = y
    view = wide[:, :P]
    assert view.stride(0) == P + 5 and not view.is_contiguous()
    ptr = view.data_ptr()
    got = graph.best_path(view, n_batch=S, return_states=True)
    assert view.data_ptr() == ptr
    assert bool(torch.isfinite(got[1]).all())
    assert _same(got, graph.best_path(y, n_batch=S, return_states=True))


# ---- 5. the form that reads the previous frame's scores from the workspace ----
def _large(H, kernel_family):
    kernel_family("force_streamed")  # (the denominator's own tables: built in a fraction of a second; not what is tested)
    fst = synth.random_den_fst(H, 3, 700, seed=31)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    return fst, graph, graph.initial_probs()


@pytest.mark.parametrize("H, forced, streamed", [(20000, True, True), (20000, False, False),
                                                 (RESIDENT_MAX_STATES, False, False), (RESIDENT_MAX_STATES + 1, False, True)])
def test_global_memory_form(kernel_family, H, forced, streamed):
    """``random_den_fst(20000, 3, 700, seed=31)`` sent through the global-memory form (its two vectors would fit LDS), and the
    graphs either side of the LDS budget, each on the form it takes by itself."""
    fst, graph, pi = _large(H, kernel_family)
    if forced:
        kernel_family("force_den_best_path_streamed")
    S, T = 2, 6
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=46)
    before = _counter(b"den_best_path_launches"), _counter(b"den_best_path_streamed_launches")
    out = graph.best_path(torch.from_numpy(y).to(DEV), n_batch=S, return_states=True)
    torch.cuda.synchronize()
    assert _counter(b"den_best_path_launches") == before[0] + 1
    assert _counter(b"den_best_path_streamed_launches") == before[1] + int(streamed)
    _check(fst, pi, y, S, out)


@pytest.mark.parametrize("kind", ["random", "skewed_tied"])
def test_both_forms_give_the_same_bits(kernel_family, kind):
    fst, graph, pi = _graph(kind)
    frames = [11, 4, 8]
    y = torch.from_numpy(synth.random_nnet_output(3, 11, fst.num_pdfs, seed=47)).to(DEV)
    resident = graph.best_path(y, frames=frames, return_states=True)
    kernel_family("force_den_best_path_streamed")
    before = _counter(b"den_best_path_streamed_launches")
    assert _same(graph.best_path(y, frames=frames, return_states=True), resident)
    assert _counter(b"den_best_path_streamed_launches") == before + 1


# ---- 6. workspace cap ----
@pytest.mark.parametrize("three_d", [False, True])
def test_workspace_cap_runs_groups_with_the_same_bits(three_d):
    fst, graph, pi = _graph("random")
    S, T, P = 5, 9, fst.num_pdfs
    frames = [9, 2, 5, 9, 7]
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=48)).to(DEV)
    x = y.reshape(T, S, P).permute(1, 2, 0).contiguous() if three_d else y
    whole = graph.best_path(x, frames=frames, return_states=True)
    cap = int(lib.tc_den_best_path_workspace_bytes(graph.ptr, 2, T))  # two sequences a group: 2 + 2 + 1
    assert int(lib.tc_den_best_path_workspace_bytes(graph.ptr, 3, T)) > cap
    before = _counter(b"den_best_path_launches")
    capped = graph.best_path(x, frames=frames, return_states=True, max_workspace_bytes=cap)
    assert _counter(b"den_best_path_launches") == before + 3
    assert _same(capped, whole)
    # a workspace tensor of the caller's caps the same way
    before = _counter(b"den_best_path_launches")
    ws = torch.empty(cap + 100, dtype=torch.uint8, device=DEV)
    assert _same(den_best_path(x, graph, frames=frames, return_states=True, workspace=ws), whole)
    assert _counter(b"den_best_path_launches") == before + 3
    with pytest.raises(ValueError, match="one sequence needs"):
        graph.best_path(x, frames=frames, max_workspace_bytes=1000)


# ---- 7. non-finite ----
@pytest.mark.parametrize("three_d", [False, True])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_input_fails_its_sequence_alone(value, three_d):
    fst, graph, pi = _graph("skewed_tied")
    S, T, P = 3, 8, fst.num_pdfs
    frames = [8, 6, 8]
    y = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=49)).to(DEV)
    to_x = (lambda m: m.reshape(T, S, P).permute(1, 2, 0).contiguous()) if three_d else (lambda m: m)
    clean = graph.best_path(to_x(y), frames=frames, return_states=True)
    bad = y.clone()
    bad[4 * S + 1, P - 1] = value  # a valid frame of sequence 1, a pdf that few arcs carry
    bad[7 * S + 1, 0] = float("nan")  # ... and a padding frame of it, which nobody reads
    got = graph.best_path(to_x(bad), frames=frames, return_states=True)
    assert bool(torch.isnan(got[1][1])) and bool((got[0][1] == -1).all()) and bool((got[2][1] == -1).all())
    for s in (0, 2):
        assert _same([o[s] for o in got], [o[s] for o in clean])
    assert bool(torch.isfinite(clean[1]).all())


# ---- 8. the graph handle is left alone ----
def _step(den, sup, y):
    x = y.clone().requires_grad_(True)
    loss, res = chain_loss(x, den, sup, l2_regularize=5e-4, leaky_hmm_coefficient=0.1)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), res.data.clone(), x.grad.clone()


@pytest.mark.parametrize("kind", ["random", "skewed"])
def test_training_step_is_the_same_after_the_call(kind):
    fst = {"random": lambda: synth.random_den_fst(300, 5, 100, seed=32),
           "skewed": lambda: synth.skewed_den_fst(300, 6000, 120, seed=4)}[kind]()
    den = io.DenominatorGraph(fst, fst.num_pdfs)  # a handle of this test's own: the first best_path call on it is made here
    S, T = 4, 12
    sup = io.Supervision.from_synth(synth.random_supervision(fst, S, T, 3, seed=52))
    y = torch.from_numpy(synth.random_nnet_output(S, T, fst.num_pdfs, seed=53)).to(DEV)
    first = _step(den, sup, y)
    before = _counter(b"den_launches"), _counter(b"den_best_path_launches")
    cap = int(lib.tc_den_best_path_workspace_bytes(den.ptr, 3, T))
    whole = den.best_path(y, n_batch=S, return_states=True)
    groups = den.best_path(y, n_batch=S, return_states=True, max_workspace_bytes=cap)  # 3 + 1
    torch.cuda.synchronize()
    assert _counter(b"den_launches") == before[0]
    assert _counter(b"den_best_path_launches") == before[1] + 3
    assert _same(groups, whole) and bool(torch.isfinite(whole[1]).all())
    second = _step(den, sup, y)
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert _same(den.best_path(y, n_batch=S, return_states=True), whole)  # ... and the step leaves the path alone


# ---- 9. warm calls allocate nothing ----
def test_warm_calls_allocate_nothing():
    fst, graph, pi = _graph("random")
    S, T, P = 4, 10, fst.num_pdfs
    x = torch.from_numpy(synth.random_nnet_output(S, T, P, seed=54).reshape(T, S, P)).to(DEV).permute(1, 2, 0).contiguous()
    ws = torch.empty(int(lib.tc_den_best_path_workspace_bytes(graph.ptr, S, T)), dtype=torch.uint8, device=DEV)
    out = (torch.empty((S, T), dtype=torch.int32, device=DEV), torch.empty((S,), dtype=torch.float64, device=DEV),
           torch.empty((S, T + 1), dtype=torch.int32, device=DEV))
    got = graph.best_path(x, return_states=True, workspace=ws, out=out)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(got, out))
    first = [o.clone() for o in out]
    level = torch.cuda.memory_allocated(), _counter(b"pool_device_allocs")
    for _ in range(3):
        for o in out:
            o.fill_(-7)
        graph.best_path(x, return_states=True, workspace=ws, out=out)
        torch.cuda.synchronize()
        assert (torch.cuda.memory_allocated(), _counter(b"pool_device_allocs")) == level
        assert _same(out, first)
