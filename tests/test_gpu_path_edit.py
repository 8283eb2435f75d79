"""Token sequences and edit distances of sampled paths on the GPU (``csrc/path_edit_kernels.hip`` through
``functions.path_edit_distance`` / ``functions.path_tokens``) and the fused gradient of ``functions.sampled_risk_surrogate``
against ``tests/path_edit_reference.py``.  Everything but the comparison with autograd's route is exact: the first is integer
arithmetic, the second fixes the order of its sums."""
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import den_best_path, den_sample_paths, path_edit_distance, path_tokens, sampled_risk_surrogate

import path_edit_reference as per

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# P = 12: 11 pdfs on 4 tokens and one silent pdf; a few pdfs start a token
TOKEN_OF_PDF = np.array([0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3, -1], np.int32)
STARTS = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1], np.uint8)  # (the flag on the silent pdf emits nothing)
P = 12


def _counter(key):
    return int(lib.tc_debug_counter(key))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _refs(rng, lengths, width=None):
    width = max(lengths) if width is None else width
    refs = np.full((len(lengths), max(width, 0)), -1, np.int32)
    for b, m in enumerate(lengths):
        refs[b, :m] = rng.integers(0, 4, m)
    return refs


def _check(pdfs, refs, ref_lengths, starts=None, frames=None, token_of_pdf=TOKEN_OF_PDF):
    """One call with the tokens and one without against the reference; returns the GPU's (dist, lengths, tokens)."""
    want = per.batch(pdfs, token_of_pdf, refs, ref_lengths, starts, frames)
    args = (_dev(pdfs), _dev(token_of_pdf), _dev(refs))
    kwargs = dict(ref_lengths=_dev(np.asarray(ref_lengths, np.int32)), starts=None if starts is None else _dev(starts),
                  frames=None if frames is None else _dev(np.asarray(frames, np.int32)))
    got = path_edit_distance(*args, return_tokens=True, **kwargs)
    for g, w, name in zip(got, want, ("dist", "lengths", "tokens")):
        assert g.dtype == torch.int32 and g.shape == w.shape, name
        assert torch.equal(g.cpu(), torch.from_numpy(w)), name
    lean = path_edit_distance(*args, **kwargs)
    assert len(lean) == 2 and torch.equal(lean[0], got[0]) and torch.equal(lean[1], got[1])
    return got


# ---- chunk edges in both dimensions, both modes ----
@pytest.mark.parametrize("mode", ["collapse", "start"])
@pytest.mark.parametrize("Tmax", [1, 2, 63, 64, 65, 128, 130, 200])
def test_chunk_edges(Tmax, mode):
    B, K = 3, 5
    rng = np.random.default_rng(100 + Tmax)
    pdfs = rng.integers(0, P, (B, K, Tmax)).astype(np.int32)
    starts = STARTS if mode == "start" else None
    for lengths in ([0, 1, 63], [64, 65, 129], [130, 0, 64]):
        refs = _refs(rng, lengths)
        dist, lens, _ = _check(pdfs, refs, lengths, starts)
        assert int(lens.min()) >= 0 and int(dist.min()) >= 0
    # hypotheses that match their references: the paths' own tokens as references, distance 0 on the diagonal
    _, lens, tokens = per.batch(pdfs, TOKEN_OF_PDF, None, None, starts)
    own = tokens[:, 0, :]
    dist, _, _ = _check(pdfs, own, lens[:, 0], starts)
    assert dist[:, 0].tolist() == [0] * B


def test_long_paths_and_references():
    B, K, Tmax, M = 1, 2, 1000, 700
    rng = np.random.default_rng(7)
    pdfs = rng.integers(0, P, (B, K, Tmax)).astype(np.int32)
    _, lens, tokens = per.batch(pdfs, TOKEN_OF_PDF, None, None)
    assert 10 * 64 < lens.min() <= lens.max() < M  # (many chunks of hypothesis against many of reference)
    refs = tokens[:, 1, :M].copy()  # the second path's own tokens and a few more, spoilt here and there
    refs[0, lens[0, 1]:] = rng.integers(0, 4, M - lens[0, 1])
    refs[0, ::7] = (refs[0, ::7] + 1) % 4
    dist, _, _ = _check(pdfs, refs, [M])
    assert 0 < int(dist[0, 1]) < int(dist[0, 0])


def test_ragged_frames_do_not_read_the_padding():
    B, K, Tmax = 4, 3, 130
    rng = np.random.default_rng(8)
    frames = [130, 64, 1, 77]
    lengths = [40, 64, 3, 65]
    refs = _refs(rng, lengths)
    pdfs = rng.integers(0, P, (B, K, Tmax)).astype(np.int32)
    clean = pdfs.copy()
    for b, n in enumerate(frames):
        clean[b, :, n:] = -1
        pdfs[b, :, n:] = rng.choice(np.array([-7, 12, 1 << 20, 3, -1, 11], np.int32), (K, Tmax - n))
    for starts in (None, STARTS):
        a = _check(pdfs, refs, lengths, starts, frames)
        b = _check(clean, refs, lengths, starts, frames)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert int(a[1].min()) >= 0  # no path failed: the garbage was not read


def test_failed_paths_get_minus_one_and_neighbours_keep_their_bits():
    B, K, Tmax = 3, 4, 70
    rng = np.random.default_rng(9)
    lengths = [10, 20, 30]
    refs = _refs(rng, lengths)
    good = rng.integers(0, P, (B, K, Tmax)).astype(np.int32)
    base = _check(good, refs, lengths)
    bad = good.copy()
    bad[1] = -1  # a failed sequence of den_sample_paths
    bad[2, 3, 69] = P  # one pdf out of range, in the second chunk
    bad[0, 0, 5] = -1
    for starts in (None, STARTS):
        base = _check(good, refs, lengths, starts)
        got = _check(bad, refs, lengths, starts)
        failed = torch.zeros((B, K), dtype=torch.bool)
        failed[1] = True
        failed[2, 3] = True
        failed[0, 0] = True
        for g, w in zip(got, base):
            g, w = g.cpu(), w.cpu()
            assert bool((g[failed] == -1).all())
            assert torch.equal(g[~failed], w[~failed])


def test_a_path_depends_on_its_own_row_alone():
    B, K, Tmax = 5, 6, 90
    rng = np.random.default_rng(10)
    lengths = [0, 17, 64, 65, 30]
    refs = _refs(rng, lengths, width=70)
    pdfs = rng.integers(0, P, (B, K, Tmax)).astype(np.int32)
    frames = [90, 64, 65, 1, 33]
    tok, r, rl, fr, st = _dev(TOKEN_OF_PDF), _dev(refs), _dev(np.asarray(lengths, np.int32)), _dev(np.asarray(frames, np.int32)), _dev(STARTS)
    d = _dev(pdfs)
    for starts in (None, st):
        whole = path_edit_distance(d, tok, r, rl, starts=starts, frames=fr, return_tokens=True)
        # batch slices and sample slices
        part = path_edit_distance(d[1:4], tok, r[1:4], rl[1:4], starts=starts, frames=fr[1:4], return_tokens=True)
        assert all(torch.equal(a, b[1:4]) for a, b in zip(part, whole))
        part = path_edit_distance(d[:, 2:5], tok, r, rl, starts=starts, frames=fr, return_tokens=True)
        assert all(torch.equal(a, b[:, 2:5]) for a, b in zip(part, whole))
        # (B, Tmax) against (B, 1, Tmax)
        flat = path_edit_distance(d[:, 3], tok, r, rl, starts=starts, frames=fr, return_tokens=True)
        assert flat[0].shape == (B,) and flat[1].shape == (B,) and flat[2].shape == (B, Tmax)
        assert all(torch.equal(a, b[:, 3]) for a, b in zip(flat, whole))
        # int64 against int32, for the paths and for the other integer arguments
        wide = path_edit_distance(d.long(), tok.long(), r.long(), rl.long(), starts=starts, frames=fr.long(), return_tokens=True)
        assert all(a.dtype == torch.int32 and torch.equal(a, b) for a, b in zip(wide, whole))
        # the tokens alone, the reference widths, and lengths counted from the padding
        tokens, lens = path_tokens(d, tok, starts=starts, frames=fr)
        assert torch.equal(tokens, whole[2]) and torch.equal(lens, whole[1])
        counted = path_edit_distance(d, tok, r, starts=starts, frames=fr)
        assert torch.equal(counted[0], whole[0]) and torch.equal(counted[1], whole[1])
        narrow = path_edit_distance(d, tok, r[:, :65].contiguous(), rl, starts=starts, frames=fr)
        assert torch.equal(narrow[0], whole[0])
        empty = path_edit_distance(d, tok, r[:, :0], starts=starts, frames=fr)
        assert torch.equal(empty[0], whole[1])  # against nothing the distance is the length
    # an int64 pdf beyond int32 is out of range, not wrapped into it
    big = d.long().clone()
    big[0, 0, 0] = (1 << 32) + 3
    got = path_edit_distance(big, tok, r, rl)
    assert int(got[0][0, 0]) == -1 and int(got[1][0, 0]) == -1 and int(got[0][0, 1]) >= 0


# ---- the sampler's and the decoder's outputs ----
@functools.lru_cache(maxsize=None)
def _graph(kind):
    fst = {
        "random": lambda: synth.random_den_fst(300, 5, 100, seed=32),
        "small": lambda: synth.random_den_fst(30, 4, 10),
    }[kind]()
    return fst, io.DenominatorGraph(fst, fst.num_pdfs)


@pytest.mark.parametrize("kind", ["small", "random"])
def test_sampled_and_decoded_paths(kind):
    fst, graph = _graph(kind)
    S, T, K, C = 3, 40, 6, fst.num_pdfs
    rng = np.random.default_rng(11)
    token_of_pdf = (np.arange(C) % 7 - 1).astype(np.int32)  # six tokens and a silent class
    starts = (rng.random(C) < 0.5).astype(np.uint8)
    frames = [40, 25, 1]
    lengths = [12, 0, 30]
    refs = np.full((S, 30), -1, np.int32)
    for b, m in enumerate(lengths):
        refs[b, :m] = rng.integers(0, 6, m)
    y = _dev(synth.random_nnet_output(S, T, C, seed=57, scale=3.0))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    pdfs = den_sample_paths(y, graph, K, frames=frames, generator=gen)
    best, _ = graph.best_path(y, frames=frames)
    assert pdfs.shape == (S, K, T) and best.shape == (S, T)
    for st in (None, starts):
        _check(pdfs.cpu().numpy(), refs, lengths, st, frames, token_of_pdf)
        _check(best.cpu().numpy()[:, None, :], refs, lengths, st, frames, token_of_pdf)
        # without `frames` the sampler's -1 padding fails the shorter sequences
        dist, lens = path_edit_distance(best, _dev(token_of_pdf), _dev(refs), starts=None if st is None else _dev(st))
        assert dist.shape == (S,) and int(lens[0]) >= 0 and lens[1:].tolist() == [-1, -1]
    # the one-call error count of a free decoding
    dist, _ = path_edit_distance(den_best_path(y, graph, frames=frames)[0], _dev(token_of_pdf), _dev(refs), frames=frames)
    want = per.batch(best.cpu().numpy()[:, None, :], token_of_pdf, refs, lengths, None, frames)[0]
    assert int(dist.sum()) == int(want.sum())


def test_warm_calls_allocate_nothing_and_do_not_synchronise():
    B, K, Tmax = 4, 8, 100
    rng = np.random.default_rng(12)
    lengths = [10, 64, 65, 0]
    d, tok, st = _dev(rng.integers(0, P, (B, K, Tmax)).astype(np.int32)), _dev(TOKEN_OF_PDF), _dev(STARTS)
    r, rl, fr = _dev(_refs(rng, lengths)), _dev(np.asarray(lengths, np.int32)), _dev(np.asarray([100, 3, 64, 99], np.int32))
    first = path_edit_distance(d, tok, r, rl, starts=st, frames=fr, return_tokens=True)
    torch.cuda.synchronize()
    level = torch.cuda.memory_allocated(), _counter(b"pool_device_allocs")  # (the outputs of `first` are part of the level)
    launches = _counter(b"path_edit_launches")
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(3):
            got = path_edit_distance(d, tok, r, rl, starts=st, frames=fr, return_tokens=True)
            lean = path_edit_distance(d, tok, r, rl, starts=st, frames=fr)
            tokens = path_tokens(d, tok, starts=st, frames=fr)
            assert _counter(b"path_edit_launches") == launches + 3 * (i + 1)
            torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(got, first)) and torch.equal(tokens[0], first[2])
            assert torch.equal(lean[0], first[0])
            del got, lean, tokens
            assert (torch.cuda.memory_allocated(), _counter(b"pool_device_allocs")) == level
            torch.cuda.set_sync_debug_mode("error")
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_call_can_be_captured_in_a_graph():
    B, K, Tmax = 2, 3, 70
    rng = np.random.default_rng(13)
    lengths = [20, 66]
    d, tok = _dev(rng.integers(0, P, (B, K, Tmax)).astype(np.int32)), _dev(TOKEN_OF_PDF)
    r, rl = _dev(_refs(rng, lengths)), _dev(np.asarray(lengths, np.int32))
    want = path_edit_distance(d, tok, r, rl, return_tokens=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        path_edit_distance(d, tok, r, rl, return_tokens=True)  # (warm on the capturing stream)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        got = path_edit_distance(d, tok, r, rl, return_tokens=True)
    fresh = _dev(rng.integers(0, P, (B, K, Tmax)).astype(np.int32))
    d.copy_(fresh)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    again = path_edit_distance(fresh, tok, r, rl, return_tokens=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    assert not torch.equal(got[2], want[2])


# ---- the fused gradient ----
_TORCH = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
_MANTISSA = {"float32": 24, "bfloat16": 8, "float16": 11}


@functools.lru_cache(maxsize=None)
def _grad_case(dtype, K):
    """Inputs that exercise every clause of the rule, as numpy arrays: y (B, C, T) holding values of `dtype` exactly."""
    B, C, T = 4, 9, 37
    rng = np.random.default_rng(20 + K)
    y = torch.from_numpy(rng.standard_normal((B, C, T)) * 12.0).to(_TORCH[dtype])
    edge = torch.tensor([30.0, -30.0, 30.0, -30.0]).to(_TORCH[dtype])
    y[0, :4, 0] = edge  # exactly on the clamp: inside
    above = {"float32": np.nextafter(np.float32(30), np.float32(40)), "bfloat16": 30.125, "float16": 30.015625}[dtype]
    y[0, 4:8, 0] = torch.tensor([above, -above, 31.0, -1e4]).to(_TORCH[dtype])  # just outside, and far
    y[0, 8, 0] = float("nan")
    pdfs = rng.integers(0, 4, (B, K, T)).astype(np.int32)  # few pdfs: samples repeat a pdf at a frame
    pdfs[0, :, 0] = np.arange(K) % C  # frame 0 of sequence 0 visits the edge values
    pdfs[:, 1::2, T // 2:] = rng.integers(0, C, pdfs[:, 1::2, T // 2:].shape)
    pdfs[2] = -1  # a failed sequence
    frames = [T, 20, T, 1]
    for b, n in enumerate(frames):
        pdfs[b, :, n:] = -1
    risks = rng.integers(0, 40, (B, K)).astype(np.float64)  # edit distances: integers
    grad_output = np.array([1.0, -0.37, 2.5, 1.0 / 3.0])
    return y, pdfs, risks, grad_output, frames


def _fused_grad(x, pdfs, risks, grad_output, frames, fused=True):
    x = x.detach().requires_grad_(True)
    value = sampled_risk_surrogate(x, pdfs, risks, frames=frames, fused=fused)
    (value * grad_output).sum().backward()
    return value.detach(), x.grad


def _same_values(a, b):
    """Equal, a NaN (the value of a sequence that sampled a NaN output) being equal to a NaN."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _bits(a):
    return a.view(torch.int32 if a.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("K", [2, 8, 64, 5])
@pytest.mark.parametrize("layout, dtype", [("bct", "float32"), ("bct", "bfloat16"), ("bct", "float16"), ("2d", "float32"),
                                           ("channel_last", "float32"), ("channel_last", "bfloat16")])
def test_fused_gradient_equals_the_reference_bit_for_bit(layout, dtype, K):
    y, pdfs, risks, grad_output, frames = _grad_case(dtype, K)
    B, C, T = y.shape
    if K & (K - 1) == 0:
        weight = per.risk_weights(risks)  # (exact: see risk_weights)
    else:  # the weights are an input of the kernel: torch's own, whose mean may round otherwise than numpy's
        r = _dev(risks)
        weight = ((r - r.mean(dim=1, keepdim=True)) / (K - 1)).cpu().numpy()
    want = per.risk_grad(y.double().numpy(), pdfs, weight, grad_output, dtype, frames)
    want = torch.from_numpy(np.asarray(want, np.float32) if dtype != "float32" else want).to(_TORCH[dtype])
    if layout == "bct":
        x = y.to(DEV)
    elif layout == "channel_last":  # a batch-first model's out.transpose(1, 2)
        x = y.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
        assert x.stride(1) == 1
    else:
        x = y.permute(2, 0, 1).reshape(T * B, C).contiguous().to(DEV)
        want = want.permute(2, 0, 1).reshape(T * B, C)
    before = _counter(b"sampled_risk_grad_launches")
    value, grad = _fused_grad(x, _dev(pdfs), _dev(risks), _dev(grad_output), frames)
    assert _counter(b"sampled_risk_grad_launches") == before + 1
    assert grad.dtype == x.dtype and grad.shape == x.shape
    assert torch.equal(_bits(grad.cpu().contiguous()), _bits(want.contiguous()))
    g3 = grad.cpu().float() if layout != "2d" else grad.cpu().view(T, B, C).permute(1, 2, 0)
    # +0 wherever the rule gives nothing: the failed sequence, padding frames, outside the clamp, the NaN
    assert not bool(torch.signbit(g3[2]).any()) and bool((g3[2] == 0).all())
    assert bool((g3[1, :, 20:] == 0).all()) and bool((g3[0, 4:, 0] == 0).all()) and bool((g3[0, :4, 0] != 0).any())
    # the same bits at every call, int64 paths and frames=None (the -1 padding says the same) included
    _, again = _fused_grad(x, _dev(pdfs).long(), _dev(risks), _dev(grad_output), None)
    assert torch.equal(_bits(again), _bits(grad))
    # equal forward values, exactly
    plain_value, _ = _fused_grad(x, _dev(pdfs), _dev(risks), _dev(grad_output), frames, fused=False)
    assert value.dtype == torch.float64 and _same_values(value, plain_value)


# The largest difference between the fused gradient and autograd's route (fused=False), in units of the input dtype's ulp
# at the size of the element's largest term |grad_output[s] * weight[s][k]| -- autograd rounds every term to the dtype and
# adds them there, in an order it does not fix, so its error is a few roundings at that size; the fused sum is rounded
# once.  Measured on these cases on an MI355X (the test prints the figure): 8 ulp in float32, 12 in bfloat16, 16 in float16
# (profiles/path_edit/README.md); the bound is twice that, because autograd's order may differ from run to run.
_MEASURED_ULPS = {"float32": 8.0, "bfloat16": 12.0, "float16": 16.0}


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_fused_gradient_against_autograds_route(dtype):
    worst = 0.0
    for K in (2, 8, 64, 5):
        y, pdfs, risks, grad_output, frames = _grad_case(dtype, K)
        B, C, T = y.shape
        x = y.to(DEV)
        value, fused = _fused_grad(x, _dev(pdfs), _dev(risks), _dev(grad_output), frames)
        plain_value, plain = _fused_grad(x, _dev(pdfs), _dev(risks), _dev(grad_output), frames, fused=False)
        assert _same_values(value, plain_value)
        r = torch.from_numpy(risks)
        weight = (r - r.mean(dim=1, keepdim=True)) / (K - 1)
        scale = (weight * torch.from_numpy(grad_output).view(B, 1)).abs().amax(dim=1)  # (B,)
        assert float(scale.min()) > 0.0
        ulp = torch.exp2(torch.floor(torch.log2(scale)) - (_MANTISSA[dtype] - 1)).view(B, 1, 1)
        diff = (fused.double().cpu() - plain.double().cpu()).abs() / ulp
        worst = max(worst, float(diff.max()))
    print("fused vs autograd, %s: largest difference %.3f ulp" % (dtype, worst))
    assert worst <= 2.0 * _MEASURED_ULPS[dtype]


# ---- end to end ----
def test_a_few_steps_lower_the_sampled_edit_distance():
    fst, graph = _graph("small")
    B, T, K, C = 8, 24, 16, fst.num_pdfs
    rng = np.random.default_rng(14)
    token_of_pdf = _dev((np.arange(C) % 5 - 1).astype(np.int32))  # four phones and silence
    lengths = rng.integers(3, 8, B)
    refs = np.full((B, 8), -1, np.int32)
    for b, m in enumerate(lengths):
        refs[b, :m] = rng.integers(0, 4, m)
    refs, ref_lengths = _dev(refs), _dev(lengths.astype(np.int32))
    out = _dev(synth.random_nnet_output(B, T, C, seed=58).reshape(T, B, C).transpose(1, 2, 0)).requires_grad_(True)  # (B, C, T)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(6)
    judge = torch.rand((B, 256, T + 1, 3), generator=gen, device=DEV)  # the same random numbers before and after

    def mean_distance():
        pdfs = den_sample_paths(out, graph, 256, uniforms=judge)
        dist, _ = path_edit_distance(pdfs, token_of_pdf, refs, ref_lengths)
        assert int(dist.min()) >= 0
        return float(dist.double().mean())

    before = mean_distance()
    copies = _counter(b"path_edit_launches")
    for _ in range(10):
        pdfs = den_sample_paths(out, graph, K, generator=gen)
        risks, _ = path_edit_distance(pdfs, token_of_pdf, refs, ref_lengths)
        sampled_risk_surrogate(out, pdfs, risks, fused=True).sum().backward()
        with torch.no_grad():
            out -= 1.0 * out.grad
            out.grad = None
    assert _counter(b"path_edit_launches") == copies + 10
    after = mean_distance()
    print("mean sampled edit distance: %.3f -> %.3f" % (before, after))
    assert after < before
