"""Rows wherever they lie (cases: tests/far_rows_cases.py; their geometry is proven in tests/test_far_rows_host.py).

Every kernel forms addresses ``base + ((t*S + s) * row_stride + pdf)`` from 32-bit t, S, s, pdf, and is right only because
each product is widened in the right place.  Here ONE matrix of a call lies in a buffer of 2^32 floats and more, its rows on
both sides of 2^29, 2^30, 2^31 and 2^32 floats from its base; everything else stays near.  The acceptance rule costs no
tolerance: results, log-probs, statuses and every element of every output have the bits of the same call on contiguous,
aligned matrices (which tests/test_gpu_row_contract.py and the other modules hold to float64), every element of the far
buffer outside the view keeps its filling -- a sentinel under an output, NaN under an input, scanned in chunks of 1 GiB --
and an input is unchanged.  A row offset that lost its upper bits reads NaN or writes the sentinel (or leaves the buffer):
it cannot meet a row of its own matrix.  Every call is a legal call on the test's own allocation.

The alpha history does not move with a stride, only with the problem: the last four tests run each kernel family that keeps
one at the smallest (S, T) where (T + 1) * S * Hs passes 2^31 floats, against the CPU oracle on all sequences, with the
bounds every denominator at size is held to (helpers.check_den_at_size) over the whole matrix, and with the first and the
last eighth of the frames held to the middle's accuracy: within far_rows_cases.ENDS_FACTOR of the median eighth's worst errors.

A test holds one far buffer at a time, allocated once for all its placements (17.2 GB whatever the matrix) and dropped when
it returns; torch's allocator hands the block on to the next test, and the device has it back behind the module."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

from torchain_amd import functions, io, synth
from torchain_amd._lib import TC_DTYPE_BF16, TC_DTYPE_F32, check, lib
from torchain_amd.functions import ChainResults, chain_loss, compute_chain_objf_and_deriv

import far_rows_cases as fr
import num_elementwise_cases as nc
import out_of_range_cases as oor
import row_contract_cases as rc
from helpers import check_den_at_size, hip_den_on, oracle_den

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L2 = 1e-3
NAN = float("nan")
MODES = ("write_l2", "accumulate")
CHUNK_BYTES = 1 << 30
fam_ids = dict(ids=lambda f: f.name)


# ---- buffers ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    """Behind the module, what torch's allocator still caches goes back to the device."""
    yield
    _at_size_reference.cache_clear()   # (about 1 GB of host arrays)
    gc.collect()
    functions._workspaces.clear()
    torch.cuda.empty_cache()


def room_for(nbytes):
    """Skips, naming the numbers, only when the device cannot give the test what it needs plus 2 GB.  ``mem_get_info`` alone
    would count the last test's pool, which torch's allocator holds for this one, as taken: what the allocator has reserved and
    not handed out is added to it."""
    free = torch.cuda.mem_get_info(0)[0] + torch.cuda.memory_reserved(0) - torch.cuda.memory_allocated(0)
    if free < nbytes + (2 << 30):
        pytest.skip("needs %.1f GB + 2 GB of device memory, %.1f GB are free" % (nbytes / 1e9, free / 1e9))


def _as_ints(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def pattern_of(value, dtype):
    return int(_as_ints(torch.tensor([value], dtype=dtype)).item())


def holds_only(buffer, value):
    """Whether every element of the flat buffer has the bit pattern of ``value``: chunks of 1 GiB, one host read."""
    flat, want = _as_ints(buffer), pattern_of(value, buffer.dtype)
    step = CHUNK_BYTES // buffer.element_size()
    bad = torch.zeros((), dtype=torch.int64, device=buffer.device)
    for i in range(0, flat.numel(), step):
        bad += (flat[i:i + step] != want).sum()
    return int(bad.item()) == 0


def take_out(buffer, view, fill):
    """The view's contents as a contiguous tensor; the view is filled with ``fill`` behind it, and the whole buffer must then
    be ``fill``: nothing was written outside the view."""
    got = view.clone()
    view.fill_(fill)
    return got, holds_only(buffer, fill)


def bits(t):
    return _as_ints(t.detach().contiguous())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def on_device(y):
    return torch.from_numpy(np.array(y, np.float32)).to(DEV)


def far_pool(rows, cols, dtype=torch.float32):
    """The test's one far allocation, for all its placements: 17.2 GB, the same for every test, so that the allocator can hand
    the block the last test returned out again (a fresh 17 GB from the device costs up to seconds); as ``dtype``.  The test
    drops it when it returns."""
    assert fr.pool_numel(rows, cols) * (2 if dtype == torch.bfloat16 else 4) <= 4 * fr.POOL_NUMEL
    room_for(4 * fr.POOL_NUMEL + (1 << 30))
    pool = torch.empty(fr.POOL_NUMEL, dtype=torch.float32, device=DEV)
    return pool if dtype == torch.float32 else pool.view(dtype)


def placed(which, far_one, rows, cols, path, fill, pool):
    """(buffer, view) of the matrix ``which``: far -- in the test's pool -- if it is ``far_one``, else near, on ``path``."""
    if which == far_one:
        buf, view = fr.far(rows, cols, fr.far_placement(rows, path), fill, DEV, pool=pool)
        assert view.stride(0) * (rows - 1) >= fr.B4 and buf.numel() > fr.B4
    else:
        buf, view = fr.near(rows, cols, path, fill, DEV)
    assert fr.on_path(view, path), (which, far_one, path, view.stride(), view.data_ptr())
    return buf, view


def untouched(buf, view, fill, far_one):
    """``take_out`` for either kind of buffer (a near one through the row contract's mask)."""
    if far_one:
        return take_out(buf, view, fill)
    got = view.clone()
    outside = rc.outside(buf, view)
    return got, bool((outside == pattern_of(fill, buf.dtype)).all())


# ---- 1. the denominator, every family -----------------------------------------------------------------------------------------
def _den_references(graph, family, yt):
    out = {}
    for mode in MODES:
        accumulate, l2_scale, init = rc.MODES[mode]
        d = torch.full_like(yt, init if accumulate else 3.0)
        r = hip_den_on(graph, family.S, yt, d, leaky=rc.LEAKY, l2_scale=l2_scale, accumulate=accumulate)
        assert r["status"] == 0 and np.isfinite(r["logprob"]), (family.name, mode, r)
        out[mode] = (r["logprob"], d)
    return out


@pytest.mark.parametrize("family", rc.FAMILIES, **fam_ids)
def test_denominator_on_far_rows(kernel_family, family):
    """y far and the derivative near, then the derivative far and y near, on the 16-byte and on the four-dword path, written
    (with the l2 term, which reads y at the row it writes) and accumulated: log-prob, status and derivative have the bits of
    the contiguous call, the far buffer is otherwise untouched, y is unchanged."""
    graph = rc.den_graph(family, kernel_family)
    assert graph.stats()["tied"] == family.tied
    S, T = family.S, family.T
    yt = on_device(rc.nnet_output(family.graph, S, T))
    rows, P = yt.shape
    pool = far_pool(rows, P)
    ref = _den_references(graph, family, yt)
    for path in fr.PATHS:
        for far_one in ("y", "deriv"):
            ybuf, yv = placed("y", far_one, rows, P, path, NAN, pool)
            dbuf, dv = placed("deriv", far_one, rows, P, path, rc.SENTINEL, pool)
            try:
                yv.copy_(yt)
                for mode in MODES:
                    accumulate, l2_scale, init = rc.MODES[mode]
                    dv.fill_(init)
                    r = hip_den_on(graph, S, yv, dv, leaky=rc.LEAKY, l2_scale=l2_scale, accumulate=accumulate)
                    what = (family.name, path, far_one, mode)
                    assert r["status"] == 0, what
                    assert r["logprob"] == ref[mode][0], what + (r["logprob"], ref[mode][0])
                    got, kept = untouched(dbuf, dv, rc.SENTINEL, far_one == "deriv")
                    assert same_bits(got, ref[mode][1]), what + (float((got - ref[mode][1]).abs().max()),)
                    assert kept, what + ("the derivative's buffer was written outside the view",)
                got, kept = untouched(ybuf, yv, NAN, far_one == "y")
                assert same_bits(got, yt) and kept, (family.name, path, far_one, "y changed, or its buffer did")
            finally:
                del yv, dv, ybuf, dbuf


# ---- 2. the whole objective -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", rc.OBJECTIVE_FAMILIES, **fam_ids)
def test_objective_on_far_rows(kernel_family, family):
    """y, deriv and xent_deriv far, each in turn: the numerator's reads and sparse ``+=`` writes, the zero rows of xent_deriv
    (x_vec, or the clearing in front) and, in a call that fails softly -- a NaN in the last, farthest row of y, then under a
    far derivative -- zero_on_fail_kernel's reset -(w * l2) * y."""
    graph = rc.den_graph(family, kernel_family)
    S, T = family.S, family.T
    sup = rc.supervision(family.graph, S, T)
    hsup = io.Supervision.from_synth(sup)
    not_carried = torch.from_numpy(~rc.carried(sup)).to(DEV)
    y = np.array(rc.nnet_output(family.graph, S, T), np.float32)
    yt = on_device(y)
    rows, P = yt.shape
    pool = far_pool(rows, P)

    def run(yy, deriv, xd):
        res = ChainResults()
        compute_chain_objf_and_deriv(graph, hsup, yy, res.data, deriv, xd, L2, rc.LEAKY, 0.1)
        torch.cuda.synchronize()
        return res.data.clone()

    d0, x0 = torch.full_like(yt, 3.0), torch.full_like(yt, 3.0)
    res0 = run(yt, d0, x0)
    assert bool(torch.isfinite(res0).all()) and res0[0] != -10.0 * res0[2] and res0[2] == sup.weight * S * T
    # the soft failure's reference: the same NaN in the contiguous call
    bad_row, bad_col = rows - 1, P // 2
    y_bad = yt.clone()
    y_bad[bad_row, bad_col] = NAN
    d1, x1 = torch.full_like(yt, 3.0), torch.full_like(yt, 3.0)
    res1 = run(y_bad, d1, x1)
    weight = np.float32(sup.weight) * np.float32(S) * np.float32(T)
    assert float(res1[0]) == np.float32(-10.0) * weight and not bool(x1.any())
    ok = torch.isfinite(y_bad)
    want = -(np.float32(np.float32(sup.weight) * np.float32(L2)) * y_bad.cpu().numpy()[ok.cpu().numpy()])
    assert np.array_equal(d1[ok].cpu().numpy().view(np.int32), want.view(np.int32))

    for path in fr.PATHS:
        for far_one in ("y", "deriv", "xent_deriv"):
            ybuf, yv = placed("y", far_one, rows, P, path, NAN, pool)
            dbuf, dv = placed("deriv", far_one, rows, P, path, rc.SENTINEL, pool)
            xbuf, xv = placed("xent_deriv", far_one, rows, P, path, rc.SENTINEL, pool)
            try:
                calls = [("clean", yt, res0, d0, x0)]
                if far_one in ("y", "deriv"):
                    calls.append(("soft failure", y_bad, res1, d1, x1))
                for name, values, res_want, d_want, x_want in calls:
                    yv.copy_(values)
                    dv.fill_(rc.SENTINEL)
                    xv.fill_(rc.SENTINEL)
                    res = run(yv, dv, xv)
                    what = (family.name, path, far_one, name)
                    assert same_bits(res, res_want), what + (res, res_want)
                    got, kept = untouched(dbuf, dv, rc.SENTINEL, far_one == "deriv")
                    assert same_bits(got, d_want) and kept, what + ("deriv", kept)
                    got, kept = untouched(xbuf, xv, rc.SENTINEL, far_one == "xent_deriv")
                    assert same_bits(got, x_want) and kept, what + ("xent_deriv", kept)
                    assert bool((got[not_carried] == 0).all()), what
                    got, kept = untouched(ybuf, yv, NAN, far_one == "y")
                    assert same_bits(got, values) and kept, what + ("y", kept)
            finally:
                del yv, dv, xv, ybuf, dbuf, xbuf


# ---- 3. the numerators alone ------------------------------------------------------------------------------------------------
def _num_on(hsup, yv, dv):
    rows, cols = yv.shape
    nbytes = 256 * ((hsup.n_batch * 8 + 255) // 256) + 256
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    lp = torch.zeros(1, dtype=torch.float64, device=DEV)
    rc_ = lib.tc_num_forward_backward(hsup.ptr, C.c_void_p(yv.data_ptr()), rows, cols, yv.stride(0), C.c_void_p(dv.data_ptr()),
                                      dv.stride(0), C.c_void_p(lp.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, 0,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    check(rc_, "tc_num_forward_backward")
    torch.cuda.synchronize()
    return float(lp.item())


def _numerator(kind):
    """(supervision handle, y, mask of the entries some arc carries or None): the smallest case of
    tests/num_elementwise_cases.py with the ten rows a far placement needs."""
    if kind == "end_to_end":
        fsts, T, P = nc.E2E[fr.NUM_E2E]()
        hsup = io.Supervision.from_e2e_fsts(nc.E2E_WEIGHT, T, P, fsts)
        y = (np.random.default_rng(7 + T).normal(size=(len(fsts) * T, P)) * 2.0).astype(np.float32)
        return hsup, y, None
    sup = nc.regular_supervision(fr.NUM_REGULAR)
    y = synth.random_nnet_output(sup.num_sequences, sup.frames_per_sequence, sup.label_dim, seed=5)
    return io.Supervision.from_synth(sup), y, rc.carried(sup)


@pytest.mark.parametrize("kind", ["resident", "windowed", "end_to_end"])
def test_numerators_on_far_rows(kernel_family, kind):
    """tc_num_forward_backward with row_stride far, then deriv_stride far: the contiguous call's log-prob and bits; the
    derivative is added to, and entries no arc carries keep what they held."""
    if kind == "windowed":
        kernel_family("force_num_windowed")
    hsup, y, carried = _numerator(kind)
    yt = on_device(y)
    rows, P = yt.shape
    pool = far_pool(rows, P)
    # which of the three kernels: the handle's kind; for a regular one the route the library announces on the host (read, like
    # the launch, under the switch as it stands) and the launch counters
    assert hsup.is_e2e == (kind == "end_to_end")
    if kind != "end_to_end":
        assert hsup.stats()["kernel"] == kind, hsup.stats()
    keys = (b"num_launches", b"num_backward_launches", b"num_windowed_launches", b"num_e2e_staged_launches")
    before = [lib.tc_debug_counter(k) for k in keys]
    d0 = torch.full_like(yt, rc.SENTINEL)
    lp0 = _num_on(hsup, yt, d0)
    # (one numerator with a backward pass; windowed only when asked for; never the staged form, which runs beside a denominator)
    assert [lib.tc_debug_counter(k) - b for k, b in zip(keys, before)] == [1, 1, 1 if kind == "windowed" else 0, 0], kind
    assert np.isfinite(lp0) and bool((d0 != rc.SENTINEL).any())
    if carried is not None:
        mask = torch.from_numpy(carried).to(DEV)
        assert bool((d0[~mask] == rc.SENTINEL).all()) and bool((d0[mask] > rc.SENTINEL).all())
    for path in fr.PATHS:
        for far_one in ("y", "deriv"):
            ybuf, yv = placed("y", far_one, rows, P, path, NAN, pool)
            dbuf, dv = placed("deriv", far_one, rows, P, path, rc.SENTINEL, pool)
            try:
                yv.copy_(yt)
                lp = _num_on(hsup, yv, dv)
                what = (kind, path, far_one)
                assert lp == lp0, what + (lp, lp0)
                got, kept = untouched(dbuf, dv, rc.SENTINEL, far_one == "deriv")
                assert same_bits(got, d0) and kept, what + ("deriv", kept)
                got, kept = untouched(ybuf, yv, NAN, far_one == "y")
                assert same_bits(got, yt) and kept, what + ("y", kept)
            finally:
                del yv, dv, ybuf, dbuf


# ---- 4. the step -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_workload():
    B, T, P = fr.STEP_B, fr.STEP_T, fr.STEP_P
    fst = synth.random_den_fst(40, 4, P, seed=6)
    graph = io.DenominatorGraph(fst, P).prepare(DEV)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, B, T, 2, seed=1))
    y, n = oor.overwrite(synth.random_nnet_output(B, T, P, seed=1), "dense")   # three whole rows beyond +-30
    assert n > 0
    return graph, sup, y, synth.random_nnet_output(B, T, P, seed=2)


def _weights(rows):
    w = np.random.default_rng(4).choice(np.array([0.0, 1.0 / 255, 0.5, 1.0, 1.0, 1.5, 3.25], np.float32), size=rows)
    return torch.from_numpy(w.astype(np.float32))


def _joint_head(kind, dtype, path, pool):
    """(buffer, input view, xent_input view): B * T far rows of 2 P elements, the chain output in a row's first half and the
    xent output in the second, NaN everywhere else.  ``rows``: 2-D, row t * B + b.  ``batch``: the (B, C, T) view of a
    batch-first (B, T, 2 P) tensor, row b * T + t."""
    graph, sup, y, xe = _step_workload()
    B, T, P = fr.STEP_B, fr.STEP_T, fr.STEP_P
    place = fr.far_placement(B * T, path)
    buf, joint = fr.far(B * T, 2 * P, place, NAN, DEV, dtype, pool=pool)
    assert fr.on_path(joint, path) and fr.on_path(joint[:, P:], path)
    if kind == "rows":
        x, xv = joint[:, :P], joint[:, P:]
        x.copy_(torch.from_numpy(y).to(DEV).to(dtype))
        xv.copy_(torch.from_numpy(xe).to(DEV).to(dtype))
    else:
        sb, st = fr.channel_last_strides("batch", B, T, place.stride)
        x = buf.as_strided((B, P, T), (sb, 1, st), place.offset)
        xv = buf.as_strided((B, P, T), (sb, 1, st), place.offset + P)
        x.copy_(torch.from_numpy(y).view(T, B, P).permute(1, 2, 0).to(DEV).to(dtype))
        xv.copy_(torch.from_numpy(xe).view(T, B, P).permute(1, 2, 0).to(DEV).to(dtype))
    return buf, joint, x, xv


def _loss(x, xe, opts):
    graph, sup, _, _ = _step_workload()
    x = x.detach().requires_grad_(True)
    xe = xe.detach().requires_grad_(True)
    loss, res = chain_loss(x, graph, sup, l2_regularize=5e-4, leaky_hmm_coefficient=0.05, xent_regularize=0.1, xent_input=xe,
                           kaldi_way=True, **opts)
    loss.sum().backward()
    torch.cuda.synchronize()
    return loss.detach(), res.data.clone(), res.xent_objf, x.grad, xe.grad


def _compare_step(kind, dtype, path, opts):
    B, T, P = fr.STEP_B, fr.STEP_T, fr.STEP_P
    pool = far_pool(B * T, 2 * P, dtype)
    buf, joint, x, xv = _joint_head(kind, dtype, path, pool)
    try:
        want_layout = ("rows", joint.stride(0), 0) if kind == "rows" else ("channel_last", T * joint.stride(0), joint.stride(0))
        assert functions.classify_layout(x.shape, x.stride()) == want_layout
        before = joint.clone()
        steps = lib.tc_debug_counter(b"channel_last_steps")
        got = _loss(x, xv, opts)
        assert lib.tc_debug_counter(b"channel_last_steps") - steps == (0 if kind == "rows" else 1)
        want = _loss(x.contiguous(), xv.contiguous(), opts)
        what = (kind, dtype, path, sorted(opts))
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2], what + (got[:3], want[:3])
        assert np.isfinite(got[2]) and not oor.took_soft_failure(float(got[1][0]), float(got[1][2]))
        assert got[3].dtype == dtype and same_bits(got[3], want[3]), what + ("grad",)
        assert same_bits(got[4], want[4]), what + ("xent grad",)
        after, kept = take_out(buf, joint, NAN)
        assert same_bits(after, before) and kept, what + ("the input buffer changed", kept)
    finally:
        del joint, x, xv, buf, pool


@pytest.mark.parametrize("path", fr.PATHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_step_on_far_two_d_rows(dtype, path):
    """input and xent_input as 2-D rows with a far row_stride: the numerator's reads, bfloat16 through widen_rows_kernel's
    in_stride, and -- with deriv_weights and the penalty -- the float32 in-place pass that reads ``input`` with row_stride."""
    _compare_step("rows", dtype, path, {})
    _compare_step("rows", dtype, path, dict(deriv_weights=_weights(fr.STEP_B * fr.STEP_T), out_of_range_regularize=0.25))


@pytest.mark.parametrize("path", fr.PATHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_step_on_a_far_batch_major_view(dtype, path):
    """A (B, T, C) view with far frame and batch strides through chain_loss, the penalty on: the gather reads the far rows, the
    scatter reads ``input`` at the row it writes.  Held to the (B, C, T) step on the contiguous copy, as every channel-last
    view is (tests/test_gpu_channel_last.py)."""
    _compare_step("batch", dtype, path, dict(deriv_weights=_weights(fr.STEP_B * fr.STEP_T), out_of_range_regularize=0.25))


def _abi_step(x, xe, sb, st, dtype, w):
    """tc_chain_step_strided in TC_LAYOUT_CHANNEL_LAST with the penalty on: (scalars, grad, xent grad), dense (B, T, C)."""
    graph, sup, _, _ = _step_workload()
    B, T, P = fr.STEP_B, fr.STEP_T, fr.STEP_P
    code = TC_DTYPE_F32 if dtype == torch.float32 else TC_DTYPE_BF16
    nbytes = lib.tc_chain_step_strided_workspace_bytes(graph.ptr, B, T, 2, 1, code)
    ws = torch.zeros(int(nbytes), dtype=torch.uint8, device=DEV)
    grad = torch.full((B, T, P), rc.SENTINEL, dtype=dtype, device=DEV)
    xgrad = torch.full((B, T, P), rc.SENTINEL, dtype=dtype, device=DEV)
    out = torch.zeros(6, dtype=torch.float32, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    code_ = lib.tc_chain_step_strided(graph.ptr, sup.ptr, ptr(x), ptr(xe), 2, 0, sb, st, 5e-4, 0.05, 0.1, 1, ptr(grad), ptr(xgrad),
                                      C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 12), C.c_void_p(out.data_ptr() + 16),
                                      ptr(w), 0.25, code, ptr(ws), ws.numel(), 0,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    check(code_, "tc_chain_step_strided")
    torch.cuda.synchronize()
    return out, grad, xgrad


@pytest.mark.parametrize("path", fr.PATHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_step_on_a_far_time_major_view_through_the_c_abi(dtype, path):
    """A (T, B, C) view with far batch and frame strides, handed to tc_chain_step_strided as a channel-last view (chain_loss
    takes such a view as the 2-D rows it is: the test above): scalars and dense gradients of the call on the dense copy."""
    graph, sup, y, xe = _step_workload()
    B, T, P = fr.STEP_B, fr.STEP_T, fr.STEP_P
    pool = far_pool(B * T, 2 * P, dtype)
    buf, joint, x, xv = _joint_head("rows", dtype, path, pool)  # row t * B + b: time-major
    try:
        w = _weights(B * T).to(DEV)
        sb, st = fr.channel_last_strides("time", B, T, joint.stride(0))
        before = joint.clone()
        steps = lib.tc_debug_counter(b"channel_last_steps")
        got = _abi_step(x, xv, sb, st, dtype, w)
        assert lib.tc_debug_counter(b"channel_last_steps") == steps + 1
        dense, xdense = (v.contiguous().view(T, B, P).permute(1, 0, 2).contiguous() for v in (x, xv))   # (B, T, C)
        want = _abi_step(dense, xdense, T * P, P, dtype, w)
        for a, b, name in zip(got, want, ("scalars", "grad", "xent grad")):
            assert same_bits(a, b), (dtype, path, name)
        assert bool((got[1] != rc.SENTINEL).all()) and float(got[0][0]) != -10.0 * float(got[0][2])
        after, kept = take_out(buf, joint, NAN)
        assert same_bits(after, before) and kept, (dtype, path, "the input buffer changed", kept)
    finally:
        del joint, x, xv, buf, pool


# ---- 5. tc_xent_objf --------------------------------------------------------------------------------------------------------
def test_xent_objf_on_far_rows():
    rows, P = fr.XENT_SHAPE
    rng = np.random.default_rng(3)
    out, deriv = (on_device(rng.normal(size=(rows, P))) for _ in range(2))
    pool = far_pool(rows, P)
    want = float(functions.xent_objective(out, deriv).item())
    assert want == float(functions.xent_objective(out, deriv).item()) and np.isfinite(want) and want != 0.0
    # (a float32 product or a float64 one, summed in double: within 2^-23 of the sum of the terms' magnitudes either way)
    assert abs(want - float((out.double() * deriv.double()).sum())) <= 2.0 ** -23 * float((out.double() * deriv.double()).abs().sum())
    for path in fr.PATHS:
        for far_one in ("output", "deriv"):
            obuf, ov = placed("output", far_one, rows, P, path, NAN, pool)
            dbuf, dv = placed("deriv", far_one, rows, P, path, NAN, pool)
            try:
                ov.copy_(out)
                dv.copy_(deriv)
                got = float(functions.xent_objective(ov, dv).item())
                assert got == want, (path, far_one, got, want)
                for buf, view, values, is_far in ((obuf, ov, out, far_one == "output"), (dbuf, dv, deriv, far_one == "deriv")):
                    after, kept = untouched(buf, view, NAN, is_far)
                    assert same_bits(after, values) and kept, (path, far_one)
            finally:
                del ov, dv, obuf, dbuf


# ---- 6. the history at size -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _at_size_reference(oracle, graph, S, T):
    """(y, the oracle's log-prob and derivative on all sequences): shared by the cases of one graph and batch, read-only;
    dropped behind the module."""
    fst = fr.at_size_fst(graph)
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=3)
    lp, deriv = oracle_den(oracle, fst, y, S, T, rc.LEAKY)
    y.setflags(write=False)
    deriv.setflags(write=False)
    return y, lp, deriv


@pytest.mark.parametrize("case", fr.AT_SIZE, ids=lambda c: c.name)
def test_history_beyond_2_31_floats(oracle, kernel_family, case):
    """One kernel family per case at the smallest batch whose alpha history passes 2^31 floats (8.6 GB), so that its last frames
    lie behind every 32-bit offset: the bounds of a denominator at size over all rows, and the first and the last eighth of the
    frames as good as the median eighth within ENDS_FACTOR -- an offset that wrapped inside the history would spoil one end,
    and the global bounds, fifty times above the kernels' rounding, would not have to notice."""
    kernel_family("no_tune")
    for key in case.build + case.launch:
        kernel_family(key)
    fst = fr.at_size_fst(case.graph)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    S, T, P = case.S, case.T, fst.num_pdfs
    nbytes = lib.tc_chain_workspace_bytes(graph.ptr, S, T)
    per_frame = (lib.tc_chain_workspace_bytes(graph.ptr, S, T + 1) - nbytes) // (4 * case.Sp)
    # which kernel: the class the graph reports, the states per frame its workspace keeps (4096: one-stream forms; 20480: the
    # plane-wise form; the graph's own states: streamed), more than 128 sequences (no two-CU form), no_tune (no two-sequence form)
    # (+ exp(y) of every frame on the streamed path)
    assert graph.stats()["tied"] == case.tied and S > 128
    assert case.Hs <= per_frame <= case.Hs + 128 + (P if case.tied == 2 else 0), per_frame
    assert (T + 1) * case.Sp * case.Hs > 2 ** 31 and nbytes > 4 * 2 ** 31
    torch.cuda.empty_cache()   # (the far tests' pool goes back first: this test's footprint is its own 9 to 10 GB)
    room_for(nbytes + 3 * 4 * S * T * P + (1 << 30))
    y, ref_lp, ref = _at_size_reference(oracle, case.graph, S, T)
    yt = on_device(y)
    deriv = torch.full_like(yt, 3.0)
    launches = [lib.tc_debug_counter(k) for k in (b"den_launches", b"den_backward_launches")]
    r = hip_den_on(graph, S, yt, deriv, leaky=rc.LEAKY)
    assert [lib.tc_debug_counter(k) for k in (b"den_launches", b"den_backward_launches")] == [launches[0] + 1, launches[1] + 1]
    d = deriv.cpu().numpy()
    del yt, deriv
    assert r["status"] == 0
    what = "%s %dx%d" % (case.name, S, T)
    # frames in eight blocks, first to last
    edges = [int(e) for e in np.linspace(0, T, 9)]
    worst = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        a, b = d[lo * S:hi * S].astype(np.float64), ref[lo * S:hi * S]
        big = np.abs(b) > 1e-3
        worst.append((float(np.abs(a - b).max()), float(np.abs(a.sum(axis=1) - 1.0).max()),
                      float((np.abs(a[big] - b[big]) / np.abs(b[big])).max())))
    print("%s: log-prob %.9g, oracle %.9g; frames %s: worst |d - oracle| %s; worst |row sum - 1| %s; worst relative error above "
          "1e-3 %s" % ((what, r["logprob"], ref_lp, edges) + tuple(" ".join("%.2e" % w[i] for w in worst) for i in range(3))))
    check_den_at_size(r["logprob"], d, ref_lp, ref, what)
    # The ends against the middle.  The global bounds above are 1e-4 and the kernels' rounding is near 1e-6, so an end fifty
    # times worse than the rest would pass them.  Each end's worst absolute error and worst relative error above 1e-3 must lie
    # within ENDS_FACTOR of the median of the eight blocks' (far_rows_cases.py says what the factor rests on).
    for i, name in ((0, "worst |d - oracle|"), (2, "worst relative error above 1e-3")):
        median = float(np.median([w[i] for w in worst]))
        assert median > 0.0, (what, name)
        for end, block in (("first", 0), ("last", 7)):
            assert worst[block][i] <= fr.ENDS_FACTOR * median, (
                what, "%s eighth of the frames: %s %.3g, more than %g times the median block's %.3g" % (
                    end, name, worst[block][i], fr.ENDS_FACTOR, median))
