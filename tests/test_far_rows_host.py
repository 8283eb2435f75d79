"""The cases of tests/test_gpu_far_rows.py checked without a GPU (tests/far_rows_cases.py).

Geometry: for every family, matrix and placement each row's first element is recomputed in Python integers -- rows on both
sides of 2^29, 2^30, 2^31 and 2^32 floats, the last row beyond 2^32, no wrapped offset that could meet a row of the same
matrix -- and the buffer has the size the GPU test allocates, so a changed shape cannot quietly stop crossing a threshold.
Sizes: the four workspace-size functions are positive, strictly increasing in S and in T and at least their documented leading
term on both sides of 2^31, 2^32 and 2^33 bytes.  Arguments: the far channel-last strides pass tc_chain_step_strided's check,
strides beyond its 2^61 bound do not, and neither call launches anything."""
import ctypes as C

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import TC_DTYPE_BF16, TC_DTYPE_F32, lib

import far_rows_cases as fr
import num_elementwise_cases as nc
import row_contract_cases as rc


# ---- geometry --------------------------------------------------------------------------------------------------------------
def _matrices():
    """(what, rows, cols) of every matrix the GPU module places far."""
    out = []
    for f in rc.FAMILIES:
        out.append((f.name, f.S * f.T, rc.GRAPHS[f.graph][1][2]))
    out.append(("step, joint head", fr.STEP_B * fr.STEP_T, 2 * fr.STEP_P))
    sup = nc.regular_supervision(fr.NUM_REGULAR)
    out.append(("numerator, " + fr.NUM_REGULAR, sup.num_sequences * sup.frames_per_sequence, sup.label_dim))
    fsts, T, P = nc.E2E[fr.NUM_E2E]()
    out.append(("numerator, " + fr.NUM_E2E, len(fsts) * T, P))
    out.append(("tc_xent_objf",) + fr.XENT_SHAPE)
    return out


@pytest.mark.parametrize("path", fr.PATHS)
@pytest.mark.parametrize("what,rows,cols", _matrices(), ids=lambda v: v if isinstance(v, str) else None)
def test_far_placements_cross_every_threshold(what, rows, cols, path):
    place = fr.far_placement(rows, path)
    stride, offset = place.stride, place.offset
    assert stride >= cols and cols <= fr.MAX_COLS
    starts = [k * stride for k in range(rows)]                 # from the base pointer: what a kernel multiplies
    assert starts[0] < fr.B1 <= fr.B4 <= starts[-1]
    for lo, hi in ((fr.B1, fr.B2), (fr.B2, fr.B3), (fr.B3, fr.B4)):
        assert any(lo <= s < hi for s in starts), (what, path, lo)
    # the same from the buffer's first element
    assert offset + starts[0] < fr.B1 and offset + starts[-1] >= fr.B4
    # a row's offset with its upper bits lost -- as unsigned or signed bytes, as an unsigned or signed element index, whole or
    # one term of it -- is the true offset less a multiple of 2^30 floats: cols floats from there meet no row, nor its own
    lost = [m * fr.B2 for m in range(1, starts[-1] // fr.B2 + 2)]
    for k, s in enumerate(starts):
        for m in lost:
            w = s - m
            assert all(w + cols <= r or r + cols <= w for r in starts), (what, path, k, m)
    if path == "vector":
        assert stride % 8 == 0 and offset == 0
        assert cols % 4 == 0 or what.startswith("numerator")   # (the numerators read and write element by element)
    else:
        assert stride % 2 == 1 and offset == 1
    numel = fr.buffer_numel(rows, cols, place)
    assert numel == offset + starts[-1] + cols + rc.SLACK
    assert 2 ** 32 < numel < 2 ** 32 + 2 ** 29                 # 17.2 GB of float32 however few rows
    assert fr.need_bytes(rows, cols, place) == 4 * numel < 20e9
    assert fr.pool_numel(rows, cols) <= fr.POOL_NUMEL and 4 * fr.POOL_NUMEL < 17.2e9


def test_far_and_near_views_are_what_they_say():
    """On a small stand-in for ``far`` (the same code with a short stride) and on ``near``: shape, strides, base, path."""
    small = fr.Placement("scalar", 37, 1)
    buf, view = fr.far(11, 24, small, rc.SENTINEL, "cpu")
    assert buf.numel() == fr.buffer_numel(11, 24, small) == 1 + 10 * 37 + 24 + rc.SLACK
    assert view.shape == (11, 24) and view.stride() == (37, 1) and view.data_ptr() - buf.data_ptr() == 4
    assert fr.on_path(view, "scalar") and not fr.on_path(view, "vector")
    view.fill_(1.0)
    assert int((buf != rc.SENTINEL).sum()) == 11 * 24
    buf, view = fr.far(11, 24, fr.Placement("vector", 40, 0), rc.SENTINEL, "cpu")
    assert fr.on_path(view, "vector") and view.data_ptr() == buf.data_ptr()
    # out of a pool: the pool's first elements, filled anew; the rest of the pool is not the buffer's
    pool = torch.full((1000,), 1.0)
    buf, view = fr.far(11, 24, small, rc.SENTINEL, "cpu", pool=pool)
    assert buf.data_ptr() == pool.data_ptr() and buf.numel() == fr.buffer_numel(11, 24, small) and view.stride() == (37, 1)
    assert bool((buf == rc.SENTINEL).all()) and bool((pool[buf.numel():] == 1.0).all())
    assert fr.pool_numel(21, 100) == max(fr.buffer_numel(21, 100, fr.far_placement(21, p)) for p in fr.PATHS)
    for path in fr.PATHS:
        for dt in (torch.float32, torch.bfloat16):
            buf, view = fr.near(15, 24, path, 0.5, "cpu", dt)
            assert view.shape == (15, 24) and fr.on_path(view, path), (path, dt)
            assert view.data_ptr() + view.element_size() * (14 * view.stride(0) + 24) <= buf.data_ptr() + buf.numel() * buf.element_size()
    assert not fr.wrapped_clear(3, fr.B2)                      # rows 2^30 apart wrap onto each other
    assert fr.wrapped_clear(3, fr.B2 + fr.MAX_COLS) and not fr.wrapped_clear(3, fr.B2 + fr.MAX_COLS - 1)


def test_channel_last_strides_of_the_step_cases():
    B, T, P = fr.STEP_B, fr.STEP_T, fr.STEP_P
    for path in fr.PATHS:
        stride = fr.far_placement(B * T, path).stride
        for major in ("batch", "time"):
            sb, st = fr.channel_last_strides(major, B, T, stride)
            rows = sorted(b * sb + t * st for b in range(B) for t in range(T))
            assert rows == [k * stride for k in range(B * T)], (path, major)
            assert fr.strides_ok(B, T, P, sb, st)


# ---- the workspace sizes -----------------------------------------------------------------------------------------------------
SIZE_GRAPHS = (  # name, graph of rc.GRAPHS, switches read when the graph is built, stats()["tied"]
    ("tied_on_chip", "tied8", (), 1),
    ("plane_wise", "planes", (), 1),
    ("general_owner", "tied8", ("force_general",), 0),
    ("general_old", "tied8", ("force_general", "old_general"), 0),
    ("streamed", "tied8", ("force_streamed", "slab_narrow"), 2),
)
_size_graphs = {}


def _size_graph(name, force):
    _, graph, build, tied = next(g for g in SIZE_GRAPHS if g[0] == name)
    for key in build:
        force(key)
    if name not in _size_graphs:
        fst = rc.den_fst(graph)
        _size_graphs[name] = io.DenominatorGraph(fst, fst.num_pdfs)
    g = _size_graphs[name]
    assert g.stats()["tied"] == tied
    return g


def _leading_term(name, g, S, T):
    """include/torchain_hip.h, tc_chain_workspace_bytes: 4 (T + 1) S Hs on chip, Hs the states rounded up -- for tied graphs
    and the owner-computes general kernel layout positions in whole planes of 4096, of which there are at least as many as
    states; 4 (T + 1) S' H beyond LDS, S' whole slabs of 16 sequences, H at least the graph's states."""
    H = g.num_states
    if name in ("tied_on_chip", "plane_wise", "general_owner"):
        return 4 * (T + 1) * S * (-(-H // 4096) * 4096)
    if name == "general_old":
        return 4 * (T + 1) * S * (-(-H // 4) * 4)
    return 4 * (T + 1) * (-(-S // 16) * 16) * H


def _size_functions(g, P):
    """name -> (f(S, T), bytes of network-output copies it adds per S * T * P float32 matrix)"""
    return {
        "tc_chain_workspace_bytes": (lambda S, T: lib.tc_chain_workspace_bytes(g.ptr, S, T), 0),
        "tc_chain_step_workspace_bytes 2-D": (lambda S, T: lib.tc_chain_step_workspace_bytes(g.ptr, S, T, 0, 1), 0),
        "tc_chain_step_workspace_bytes 3-D": (lambda S, T: lib.tc_chain_step_workspace_bytes(g.ptr, S, T, 1, 1), 3),
        "tc_chain_step_typed_workspace_bytes bf16 2-D": (lambda S, T: lib.tc_chain_step_typed_workspace_bytes(g.ptr, S, T, 0, 1, TC_DTYPE_BF16), 4),
        "tc_chain_step_typed_workspace_bytes bf16 3-D": (lambda S, T: lib.tc_chain_step_typed_workspace_bytes(g.ptr, S, T, 1, 0, TC_DTYPE_BF16), 2),
        "tc_chain_step_strided_workspace_bytes": (lambda S, T: lib.tc_chain_step_strided_workspace_bytes(g.ptr, S, T, 2, 1, TC_DTYPE_F32), 3),
    }


def _first_at_or_above(f, lo, hi, want):
    """The smallest n in (lo, hi] with f(n) >= want; f(lo) < want <= f(hi)."""
    assert f(lo) < want <= f(hi), (f(lo), want, f(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if f(mid) >= want else (mid, hi)
    return hi


@pytest.mark.parametrize("name", [g[0] for g in SIZE_GRAPHS])
def test_workspace_sizes_either_side_of_32_bit_limits(kernel_family, name):
    g = _size_graph(name, kernel_family)
    P = g.n_pdf
    for fname, (f, copies) in _size_functions(g, P).items():
        for limit in (2 ** 31, 2 ** 32, 2 ** 33):
            # in T at two fixed batches (64: tied on-chip graphs get the second history of the two-CU forms up to 128 sequences,
            # the one step down in S there is; 512: none), then in S above 128 at the T found: two pairs below the limit and
            # two at or above it
            S = 512
            T0 = _first_at_or_above(lambda t: f(64, t), 1, 1 << 24, limit)
            T = _first_at_or_above(lambda t: f(S, t), 1, 1 << 24, limit)
            S2 = _first_at_or_above(lambda s: f(s, T), 130, S, limit)
            runs = ([(64, T0 - 2), (64, T0 - 1), (64, T0), (64, T0 + 1)], [(S, T - 2), (S, T - 1), (S, T), (S, T + 1)],
                    [(S2 - 2, T), (S2 - 1, T), (S2, T), (S2 + 1, T)])
            for run in runs:
                sizes = [f(s, t) for s, t in run]
                what = (name, fname, limit, run, sizes)
                assert all(isinstance(v, int) and v > 0 for v in sizes), what
                assert all(a < b for a, b in zip(sizes, sizes[1:])), what          # strictly increasing, no wrapped value
                assert sizes[1] < limit <= sizes[2], what                           # ... on both sides of the limit
                for (s, t), v in zip(run, sizes):
                    assert v >= _leading_term(name, g, s, t) + copies * 4 * s * t * P, what + (s, t)
                    assert v % 256 == 0
    # the step's sizes are the objective's and the copies: no term appears or disappears across the limits
    base = _size_functions(g, P)["tc_chain_workspace_bytes"][0]
    for S, T in ((256, 150), (256, 4000), (2048, 3000)):
        for fname, (f, copies) in _size_functions(g, P).items():
            extra = f(S, T) - base(S, T)
            assert copies * 4 * S * T * P <= extra <= copies * (4 * S * T * P + 256) + (1 << 16), (name, fname, S, T, extra)


def test_workspace_sizes_refuse_what_they_cannot_size(kernel_family):
    g = _size_graph("tied_on_chip", kernel_family)
    for S, T in ((0, 10), (10, 0), (-1, 10)):
        assert lib.tc_chain_workspace_bytes(g.ptr, S, T) == -1
        assert lib.tc_chain_step_strided_workspace_bytes(g.ptr, S, T, 2, 1, TC_DTYPE_F32) == -1
    assert lib.tc_chain_step_strided_workspace_bytes(g.ptr, 4, 4, 3, 1, TC_DTYPE_F32) == -1


# ---- the argument check that guards far strides ------------------------------------------------------------------------------
def test_far_channel_last_strides_pass_the_argument_check_and_2_61_does_not(kernel_family):
    """tc_chain_step_strided checks the strides before it looks at the workspace and long before it touches a device: with a
    NULL workspace a pair of strides it accepts is TC_ERR_WORKSPACE, one it refuses TC_ERR_INVALID_ARGUMENT.  Neither call
    launches anything or reads a pointer (they point at host arrays here)."""
    B, T, P = fr.STEP_B, fr.STEP_T, fr.STEP_P
    fst = synth.random_den_fst(40, 4, P, seed=6)
    kernel_family("no_tune")
    graph = io.DenominatorGraph(fst, P)
    sup = io.Supervision.from_synth(synth.random_supervision(fst, B, T, 2, seed=1))
    host = np.zeros(4096, np.float32)
    ptr = C.c_void_p(host.ctypes.data)
    launches = [lib.tc_debug_counter(k) for k in (b"den_launches", b"num_launches", b"layout_launches", b"channel_last_steps")]

    def step(sb, st, dtype=TC_DTYPE_F32):
        return lib.tc_chain_step_strided(graph.ptr, sup.ptr, ptr, ptr, 2, 0, sb, st, 1e-3, 0.1, 0.1, 1, ptr, ptr, ptr, ptr, ptr,
                                         None, 0.25, dtype, None, 0, 0, None)

    for path in fr.PATHS:
        stride = fr.far_placement(B * T, path).stride
        for major in ("batch", "time"):
            sb, st = fr.channel_last_strides(major, B, T, stride)
            assert fr.strides_ok(B, T, P, sb, st)
            for dtype in (TC_DTYPE_F32, TC_DTYPE_BF16):
                assert step(sb, st, dtype) == -4, (path, major, dtype)
    lim = (2 ** 63 - 1) // 4                                   # 2^61: every element offset fits 63 bits below it
    for sb, st, ok in ((lim // T, P, True), (lim // T + 1, P, False), (P, lim // B, True), (P, lim // B + 1, False),
                       (2 ** 62, P, False), (P, 2 ** 62, False), (2 ** 63 - 1, P, False), (-fr.B4, P, False)):
        assert fr.strides_ok(B, T, P, sb, st) == ok
        assert step(sb, st) == (-4 if ok else -1), (sb, st)
    assert [lib.tc_debug_counter(k) for k in (b"den_launches", b"num_launches", b"layout_launches", b"channel_last_steps")] == launches


# ---- the history at size -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fr.AT_SIZE, ids=lambda c: c.name)
def test_at_size_cases_pass_2_31_floats_of_history(kernel_family, case):
    kernel_family("no_tune")
    for key in case.build:
        kernel_family(key)
    fst = fr.at_size_fst(case.graph)
    g = io.DenominatorGraph(fst, fst.num_pdfs)
    assert g.stats()["tied"] == case.tied
    ws = lambda S, T: lib.tc_chain_workspace_bytes(g.ptr, S, T)  # noqa: E731
    # Hs as the workspace has it: the bytes one more frame adds, per (padded) sequence
    per_frame = (ws(case.S, case.T + 1) - ws(case.S, case.T)) // (4 * case.Sp)
    # (the streamed path also keeps exp(y) of every frame: P more floats per frame and sequence)
    assert case.Hs <= per_frame <= case.Hs + 128 + (fst.num_pdfs if case.tied == 2 else 0), (case.name, per_frame)
    assert fr.history_floats(case) > 2 ** 31 and ws(case.S, case.T) >= 4 * fr.history_floats(case) > 2 ** 33
    # ... and it is the smallest T of its batch that does, within a frame or two of slack; under 20 GB with y and the derivative
    assert (case.T - 2) * case.Sp * case.Hs < 2 ** 31
    assert ws(case.S, case.T) + 3 * 4 * case.S * case.T * fst.num_pdfs < 12e9
    # gamma's fixed point: 2^-31 per add stays below the 1e-7 absolute of the element-wise bound (far_rows_cases.py)
    assert fr.adds_per_entry(fst) * 2.0 ** -31 <= 0.5e-7
