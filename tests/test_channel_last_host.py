"""Channel-last views without a GPU: ``functions.classify_layout`` -- the one host-only predicate that decides which layout a
tensor goes to the step in -- on CPU tensors for every view the GPU test runs, degenerate shapes, overlapping rows and
strides no tensor should have; the numpy statement of the row gather / scatter; the header and the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import channel_last_cases as clc
from torchain_amd import functions
from torchain_amd._lib import LIB_PATH, lib
from torchain_amd.functions import classify_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "torchain_hip.h")
OTHER = ("other", 0, 0)


def _kind(t):
    return classify_layout(t.shape, t.stride())


@pytest.mark.parametrize("P,B,T", clc.SHAPES)
def test_every_view_of_the_gpu_test(P, B, T):
    rows = np.arange(T * B * P, dtype=np.float32).reshape(T * B, P)
    for dtype in (torch.float32, torch.bfloat16):
        for kind in clc.VIEWS:
            leaf = clc.make_leaf(kind, rows, B, T, "cpu", dtype)
            v = clc.region(kind, leaf.detach(), P)
            assert tuple(v.shape) == (B, P, T)
            got = _kind(v)
            if kind in clc.TIME_MAJOR or B == 1:  # (one sequence: its frames are a run of rows whatever the layout)
                rs = v.stride(2) if B == 1 else v.stride(0)
                assert got == ("time_major", rs, 0), (kind, got)
                # the 2-D tensor the step is handed: the same memory, row t*B + b
                two_d = v.as_strided((T * B, P), (rs, 1))
                assert torch.equal(two_d.float(), torch.from_numpy(rows).to(dtype).float())
            else:
                assert got == ("channel_last", v.stride(0), v.stride(2)), (kind, got)
                assert v.stride(1) == 1 and v.stride(2) >= P
            # the contiguous copy is the reference's layout, and 2-D rows stay 2-D rows
            assert _kind(v.contiguous()) == ("bct", 0, 0)
    assert _kind(torch.zeros(T * B, P)) == ("rows", P, 0)
    assert _kind(torch.zeros(T * B, P + 3)[:, :P]) == ("rows", P + 3, 0)


def test_contiguous_bct_is_always_bct():
    for shape in [(1, 1, 1), (1, 5, 1), (3, 1, 1), (1, 1, 4), (3, 1, 4), (1, 5, 4), (3, 5, 1), (3, 5, 4)]:
        x = torch.zeros(shape)
        assert x.is_contiguous() and _kind(x) == ("bct", 0, 0), shape
        # (a transposed view that happens to be contiguous -- C == 1 or T == 1 -- is the same memory either way)
        v = torch.zeros(shape[0], shape[2], shape[1]).transpose(1, 2)
        assert (_kind(v) == ("bct", 0, 0)) == v.is_contiguous(), shape


def test_degenerate_shapes():
    # B = 1: strides of the batch dimension are ignored; the frames are 2-D rows
    assert classify_layout((1, 7, 5), (12345, 1, 9)) == ("time_major", 9, 0)
    assert classify_layout((1, 7, 5), (0, 1, 7)) == ("time_major", 7, 0)
    assert classify_layout((1, 7, 5), (0, 1, 6)) == OTHER            # rows overlap
    # T = 1: strides of the frame dimension are ignored
    assert classify_layout((4, 7, 1), (9, 1, -3)) == ("time_major", 9, 0)
    assert classify_layout((4, 7, 1), (6, 1, 1)) == OTHER
    # C = 1: the channel stride is ignored
    assert classify_layout((3, 1, 4), (4, 999, 1)) == ("bct", 0, 0)
    assert classify_layout((3, 1, 4), (8, 999, 2)) == ("channel_last", 8, 2)
    assert classify_layout((3, 1, 4), (1, 999, 3)) == ("time_major", 1, 0)
    # B = T = 1 with a padded row
    assert classify_layout((1, 7, 1), (50, 1, 50)) == ("bct", 0, 0)


def test_overlapping_zero_and_negative_strides_are_other():
    B, T, P = 3, 5, 8
    e = torch.zeros(1, T, P).expand(B, T, P).transpose(1, 2)          # every sequence the same memory
    assert e.stride(0) == 0 and _kind(e) == OTHER
    e = torch.zeros(B, 1, P).expand(B, T, P).transpose(1, 2)          # every frame the same memory
    assert _kind(e) == OTHER
    assert _kind(torch.zeros(B, T, 1).expand(B, T, P).transpose(1, 2)) == OTHER   # channel stride 0
    assert _kind(torch.zeros(B, P, 2 * T)[:, :, ::2]) == OTHER                    # channel stride not 1
    assert _kind(torch.zeros(B, T, 2 * P)[..., ::2].transpose(1, 2)) == OTHER
    for sb, st in [(-P * T, P), (P * T, -P), (P * T, P - 1), (P - 1, P * B), (P * T - 1, P), (P, P * B - 1), (2 * P, 3 * P),
                   (0, P), (P, 0)]:
        assert classify_layout((B, P, T), (sb, 1, st)) == OTHER, (sb, st)
    # the two nestings, exactly at their limits
    assert classify_layout((B, P, T), ((T - 1) * (P + 2) + P, 1, P + 2)) == ("channel_last", (T - 1) * (P + 2) + P, P + 2)
    assert classify_layout((B, P, T), (P + 2, 1, (B - 1) * (P + 2) + P + 1))[0] == "channel_last"  # time-major, padded frames
    assert classify_layout((B, P, T), (P + 2, 1, B * (P + 2))) == ("time_major", P + 2, 0)
    for bad in [(), (4,), (2, 3, 4, 5), (0, 3, 4), (2, 0)]:
        assert classify_layout(bad, (1,) * len(bad)) == OTHER


def test_pairs_that_go_together_and_pairs_that_do_not():
    """``_step_plan`` needs CUDA tensors (there is no CPU step), so the pairing rule is checked on the layouts."""
    B, T, P = 3, 5, 20
    joint = torch.zeros(B, T, 2 * P)
    lo, hi = joint[..., :P].transpose(1, 2), joint[..., P:].transpose(1, 2)
    assert _kind(lo) == _kind(hi) and _kind(lo)[0] == "channel_last"
    dense = torch.zeros(B, T, P).transpose(1, 2)
    assert _kind(dense) != _kind(lo)
    geo = lambda t: (tuple(t.shape), tuple(t.stride()))  # noqa: E731
    assert functions.pair_layout(geo(lo), geo(hi)) == _kind(lo) == functions.pair_layout(geo(lo))
    assert functions.pair_layout(geo(dense), geo(lo)) is None and functions.pair_layout(geo(lo), geo(dense)) is None
    assert functions.pair_layout(geo(lo), geo(hi[:2])) is None  # (the same strides, another shape)
    assert functions._step_plan(lo, hi) is None and not functions._one_call(lo)  # CPU tensors are never taken
    assert not functions._step_view(lo) and functions._step_plan(lo, None) is None


def test_numpy_statement_of_gather_and_scatter():
    B, T, P = 3, 5, 7
    rng = np.random.default_rng(1)
    rows = rng.normal(size=(T * B, P)).astype(np.float32)
    for kind in clc.VIEWS:
        leaf = clc.make_leaf(kind, rows, B, T, "cpu", torch.float32).detach()
        v = clc.region(kind, leaf, P)
        flat = leaf.reshape(-1).numpy()
        got = clc.gather_np(flat, v.storage_offset(), B, T, P, v.stride(0), v.stride(2), P + 4, -7.0)
        np.testing.assert_array_equal(got[:, :P], rows)
        assert (got[:, P:] == -7.0).all()
    # the scatter is the inverse permutation with the step's arithmetic
    w = rng.choice(np.array([0.0, 0.5, 1.0, 3.25], np.float32), size=T * B)
    y = (rows * 20).astype(np.float32)
    y_btp = y.reshape(T, B, P).transpose(1, 0, 2)
    back = clc.scatter_np(rows, B, T, P, -1.0)
    np.testing.assert_array_equal(back.transpose(1, 0, 2).reshape(T * B, P), -rows)
    weighted = clc.scatter_np(rows, B, T, P, -1.0, w=w)
    np.testing.assert_array_equal(weighted.transpose(1, 0, 2).reshape(T * B, P), (-w)[:, None] * rows)
    pen = clc.scatter_np(rows, B, T, P, -1.0, w=w, c=0.25, y_btp=y_btp)
    want = w[:, None] * clc.oor.penalized(-rows, y, 0.25)
    np.testing.assert_array_equal(pen.transpose(1, 0, 2).reshape(T * B, P), want.astype(np.float32))
    assert (np.abs(y) > 30).any() and not np.array_equal(pen, weighted)


def test_header_declares_the_entries_with_a_citation():
    text = open(HEADER).read()
    raw = C.CDLL(LIB_PATH)
    for name in ("tc_chain_step_strided", "tc_chain_step_strided_workspace_bytes", "tc_rows_gather", "tc_rows_scatter"):
        m = re.search(r"\b(?:int|int64_t) %s\(" % name, text)
        assert m, name
        assert hasattr(raw, name), name
    doc = text[:text.index("int64_t tc_chain_step_strided_workspace_bytes(")].rsplit("/* tc_chain_step_penalized with a layout", 1)[1]
    doc = " ".join(doc.replace("*", " ").split())  # (the comment's line breaks and margin)
    assert "torchain/functions.py:118-125" in doc
    for word in ("TC_LAYOUT_CHANNEL_LAST", "batch_stride", "frame_stride", "TC_ERR_INVALID_ARGUMENT", "bit for bit",
                 "channel_last_steps"):
        assert word in doc, word
    for name, value in (("TC_LAYOUT_ROWS", 0), ("TC_LAYOUT_BCT", 1), ("TC_LAYOUT_CHANNEL_LAST", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    gather_doc = text[:text.index("int tc_rows_gather(")].rsplit("/*", 1)[1]
    assert "torchain/functions.py:118-125" in gather_doc
    assert lib.tc_debug_counter(b"channel_last_steps") >= 0  # (a known key)


def test_bad_arguments_are_refused_on_the_host():
    """Unknown layouts and bad strides are refused before a device or a workspace is looked at."""
    from torchain_amd import io, synth
    fst = synth.random_den_fst(20, 3, 10, seed=2)
    g = io.DenominatorGraph(fst, 10)
    B, T, P = 2, 8, 10
    s = io.Supervision.from_synth(synth.random_supervision(fst, B, T, 2, seed=3))
    assert lib.tc_chain_step_strided_workspace_bytes(g.ptr, B, T, 3, 0, 0) == -1
    for layout in (0, 1, 2):
        assert lib.tc_chain_step_strided_workspace_bytes(g.ptr, B, T, layout, 1, 7) == -1  # unknown dtype
    for dtype in (0, 1, 2):
        for xent in (0, 1):
            assert (lib.tc_chain_step_strided_workspace_bytes(g.ptr, B, T, 2, xent, dtype)
                    == lib.tc_chain_step_typed_workspace_bytes(g.ptr, B, T, 1, xent, dtype) > 0)
            assert (lib.tc_chain_step_strided_workspace_bytes(g.ptr, B, T, 0, xent, dtype)
                    == lib.tc_chain_step_typed_workspace_bytes(g.ptr, B, T, 0, xent, dtype))
    ws = (C.c_char * 256)()
    p = C.cast(ws, C.c_void_p)

    def step(layout, sb, st, ptr=p):
        return lib.tc_chain_step_strided(g.ptr, s.ptr, ptr, None, layout, 0, sb, st, 0.0, 0.1, 0.0, 1, None, None, p, None, None,
                                         None, 0.0, 0, p, 256, 0, None)
    assert step(3, T * P, P) == -1 and step(-1, T * P, P) == -1
    for sb, st in [(T * P, P - 1), (T * P - 1, P), (-T * P, P), (T * P, -P), (0, P), (P, 0), (P - 1, B * P), (3 * P, 2 * P)]:
        assert step(2, sb, st) == -1, (sb, st)
    assert step(2, T * P, P, ptr=C.c_void_p(p.value + 2)) == -1  # a float32 tensor at an odd half-word
    assert lib.tc_rows_gather(p, 0, B, P, T, T * P, P - 1, p, P, 0, None) == -1
    assert lib.tc_rows_gather(p, 0, B, P, T, T * P, P, p, P - 1, 0, None) == -1
    assert lib.tc_rows_gather(p, 5, B, P, T, T * P, P, p, P, 0, None) == -1
    assert lib.tc_rows_scatter(p, P - 1, 0, B, P, T, -1.0, None, 0.0, None, 0, 0, p, 0, None) == -1
    assert lib.tc_rows_scatter(p, P, 0, B, P, T, -1.0, None, 0.25, None, T * P, P, p, 0, None) == -1  # penalty without input
    assert lib.tc_rows_scatter(p, P, 0, B, P, T, -1.0, None, -1.0, p, T * P, P, p, 0, None) == -1
