"""The planner of ``chain_loss`` without a GPU: ``functions.plan_step_inputs`` -- the one pure function of shapes, strides and
dtypes that decides what becomes of any ``(input, xent_input)`` pair -- over a table of pairs.  For each: the operations chosen,
and, with the operations applied to CPU tensors of that geometry, that the pair which comes out is one ``_run_step`` accepts
(``functions._step_plan`` without its CUDA requirement: one dtype the step takes, one layout that goes together) in the layout
the planner announced.  And what every route keeps: CPU tensors are an ``AssertionError``."""
import numpy as np
import pytest
import torch

import channel_last_cases as clc
from torchain_amd import functions
from torchain_amd.functions import chain_loss

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
P, B, T = 20, 3, 5


def _accepted(x, xe):
    """What ``_run_step`` accepts, but for the device: the layout, or None."""
    if x.dtype not in functions._STEP_DTYPES or (xe is not None and xe.dtype != x.dtype):
        return None
    geo = lambda t: (tuple(t.shape), tuple(t.stride()))  # noqa: E731
    return functions.pair_layout(geo(x), geo(xe) if xe is not None else None)


def _planned(x, xe, want_grad=True):
    ops, xent_ops, layout = functions.plan_step_inputs(functions._spec(x), functions._spec(xe), want_grad)
    a, b = x, xe
    for op in ops:
        a = functions._OPS[op](a)
    for op in xent_ops:
        b = functions._OPS[op](b)
    assert _accepted(a, b) == layout, (ops, xent_ops, layout, a.stride(), None if b is None else b.stride())
    # (values: every operation is a copy or a cast of the same elements, in the frame-major order of to2d)
    assert torch.equal(functions.to2d(a).float(), functions.to2d(x).float())
    return ops, xent_ops, layout


def _view(kind, dtype=F32, seed=0, shape=(P, B, T)):
    p, b, t = shape
    rows = np.random.default_rng(seed).normal(size=(t * b, p)).astype(np.float32)
    return clc.region(kind, clc.make_leaf(kind, rows, b, t, "cpu", dtype).detach(), p)


def _bct(dtype=F32):
    return torch.randn(B, P, T).to(dtype)


def _rows(dtype=F32, pad=0):
    return torch.randn(T * B, P + pad).to(dtype)[:, :P]


@pytest.mark.parametrize("shape", clc.SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_every_channel_last_view_goes_as_it_is(shape, dtype):
    """Alone and with a view of the same strides: no operation, in the layout ``classify_layout`` finds."""
    for kind in clc.VIEWS:
        x, xe = _view(kind, dtype, 0, shape), _view(kind, dtype, 1, shape)
        want = functions.classify_layout(x.shape, x.stride())
        assert want[0] in ("time_major", "channel_last")
        assert _planned(x, None) == ((), (), want), kind
        assert _planned(x, xe) == ((), (), want), kind
        assert _planned(x, xe, want_grad=False) == ((), (), want), kind
    joint = torch.randn(shape[1], shape[2], 2 * shape[0]).to(dtype)
    lo, hi = joint[..., :shape[0]].transpose(1, 2), joint[..., shape[0]:].transpose(1, 2)
    assert _planned(lo, hi) == _planned(hi, lo) == ((), (), functions.classify_layout(lo.shape, lo.stride()))


def test_the_reference_layouts_go_as_they_are():
    for dtype in (F32, BF16, F16):
        assert _planned(_bct(dtype), None) == _planned(_bct(dtype), _bct(dtype)) == ((), (), ("bct", 0, 0))
        assert _planned(_rows(dtype), _rows(dtype)) == ((), (), ("rows", P, 0))
        assert _planned(_rows(dtype, 4), _rows(dtype, 4)) == ((), (), ("rows", P + 4, 0))
        assert _planned(_rows(dtype, 4), None) == ((), (), ("rows", P + 4, 0))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_mixed_pairs(dtype):
    c, bct, rows = ("contiguous",), ("bct", 0, 0), ("rows", P, 0)
    # 2-D rows with different row strides: the pair is made contiguous (whichever is not)
    assert _planned(_rows(dtype, 4), _rows(dtype)) == (c, (), rows)
    assert _planned(_rows(dtype), _rows(dtype, 4)) == ((), c, rows)
    assert _planned(_rows(dtype, 4), _rows(dtype, 8)) == (c, c, rows)
    # (B, C, T) with 2-D: to2d on the 3-D tensor, whatever its layout; the 2-D one then has to have its row stride
    for three_d in (_bct(dtype), _view("dense", dtype), _view("time_major", dtype), torch.randn(B, P, 2 * T).to(dtype)[:, :, ::2]):
        assert _planned(three_d, _rows(dtype)) == (("to2d",), (), rows)
        assert _planned(_rows(dtype), three_d) == ((), ("to2d",), rows)
        assert _planned(three_d, _rows(dtype, 4)) == (("to2d",), c, rows)
        assert _planned(_rows(dtype, 4), three_d, want_grad=False) == (c, ("to2d",), rows)
    # any other 3-D pair: every tensor that is not contiguous (B, C, T) is made so
    assert _planned(_view("dense", dtype), _bct(dtype)) == (c, (), bct)                      # channel-last + contiguous
    assert _planned(_bct(dtype), _view("head_lo", dtype)) == ((), c, bct)
    assert _planned(_view("dense", dtype), _view("batch_pad", dtype)) == (c, c, bct)         # different strides
    assert _planned(_view("time_major", dtype), _view("dense", dtype)) == (c, c, bct)        # time-major + batch-first
    assert _planned(_view("time_major", dtype), _view("time_major_pad", dtype)) == (c, c, bct)
    wide = torch.randn(B, P, 2 * T).to(dtype)[:, :, ::2]                                     # channel stride not 1
    assert _planned(wide, None) == (c, (), bct)
    assert _planned(wide, _bct(dtype)) == (c, (), bct)
    assert _planned(wide, wide) == (c, c, bct)
    assert _planned(torch.randn(1, T, P).to(dtype).expand(B, T, P).transpose(1, 2), None) == (c, (), bct)  # overlapping rows
    # a 2-D tensor whose column stride is not 1
    assert _planned(torch.randn(P, T * B).to(dtype).t(), None) == (c, (), rows)


def test_size_one_dimensions():
    c = ("contiguous",)
    one_seq = torch.randn(1, T, P).transpose(1, 2)   # B = 1: its frames are a run of rows whatever the layout
    assert _planned(one_seq, None) == ((), (), ("time_major", P, 0))
    assert _planned(one_seq, torch.randn(1, T, P).transpose(1, 2)) == ((), (), ("time_major", P, 0))
    assert _planned(one_seq, torch.randn(1, P, T)) == (c, (), ("bct", 0, 0))
    one_frame = torch.randn(B, 1, P).transpose(1, 2)  # T = 1: contiguous either way
    assert _planned(one_frame, None) == ((), (), ("bct", 0, 0))
    assert _planned(torch.randn(B, 1, P + 4)[..., :P].transpose(1, 2), None) == ((), (), ("time_major", P + 4, 0))
    assert _planned(one_frame, torch.randn(B, P)) == (("to2d",), (), ("rows", P, 0))
    assert _planned(torch.randn(B, T, 1).transpose(1, 2), None) == ((), (), ("bct", 0, 0))  # C = 1: contiguous either way
    assert _planned(torch.randn(1, P), torch.randn(1, P + 4)[:, :P]) == ((), (), ("rows", P, 0))  # one row: no row stride
    assert _planned(torch.randn(1, 1, 1), torch.randn(1, 1)) == (("to2d",), (), ("rows", 1, 0))


def test_sixteen_bit_with_thirty_two_bit():
    f, c = ("float",), ("contiguous",)
    assert _planned(_bct(BF16), _bct(F32)) == (f, (), ("bct", 0, 0))
    assert _planned(_bct(F32), _bct(F16)) == ((), f, ("bct", 0, 0))
    assert _planned(_bct(BF16), _bct(F16)) == (f, f, ("bct", 0, 0))
    assert _planned(_rows(F16), _rows(F32), want_grad=False) == (f, (), ("rows", P, 0))
    # a dense view keeps its strides through the cast: a channel-last pair still goes together
    x, xe = _view("dense", BF16), _view("dense", F32)
    assert _planned(x, xe) == (f, (), functions.classify_layout(xe.shape, xe.stride()))
    assert _planned(_view("time_major", F32), _view("time_major", F16))[:2] == ((), f)
    # a view with gaps is made contiguous in front of the cast, and so is then its partner
    assert _planned(_view("head_lo", BF16), _view("head_lo", F32)) == (c + f, c, ("bct", 0, 0))
    assert _planned(_rows(BF16, 4), _rows(F32, 4)) == (c + f, c, ("rows", P, 0))
    # with another layout on top
    assert _planned(_bct(BF16), _rows(F32)) == (("float", "to2d"), (), ("rows", P, 0))
    assert _planned(_view("dense", F32), _bct(F16)) == (c, f, ("bct", 0, 0))


def test_other_dtypes_ranks_and_empty_tensors():
    """A dtype the step does not take: ``ValueError`` when a gradient is wanted, up-cast otherwise."""
    d = torch.randn(B, P, T, dtype=torch.float64)
    for xe in (None, _bct(F32), _bct(BF16), d):
        with pytest.raises(ValueError):
            functions.plan_step_inputs(functions._spec(d), functions._spec(xe), True)
    assert _planned(d, None, want_grad=False) == (("float",), (), ("bct", 0, 0))
    assert _planned(d, _bct(F32), want_grad=False) == (("float",), (), ("bct", 0, 0))
    assert _planned(_bct(BF16), d, want_grad=False) == (("float",), ("float",), ("bct", 0, 0))
    for bad in (torch.zeros(P), torch.zeros(2, B, P, T), torch.zeros(0, P), torch.zeros(B, 0, T)):
        with pytest.raises(ValueError):
            functions.plan_step_inputs(functions._spec(bad), None, True)
        with pytest.raises(ValueError):
            functions.plan_step_inputs(functions._spec(_bct(F32)), functions._spec(bad), False)


@pytest.mark.parametrize("grad", [True, False])
def test_cpu_tensors_keep_the_assertion(grad):
    """No CPU implementation, on any route: an ``AssertionError`` before the graph or the supervision is looked at."""
    for x, xe in ((_bct(), None), (_rows(), None), (_bct(), _bct()), (_rows(), _rows(pad=4)), (_bct(BF16), None),
                  (_view("dense"), _view("dense", seed=1))):
        x = x.clone().requires_grad_(grad) if x.is_contiguous() else x.requires_grad_(grad)
        with pytest.raises(AssertionError):
            if grad:
                chain_loss(x, None, None, xent_regularize=0.1 if xe is not None else 0.0, xent_input=xe)
            else:
                with torch.no_grad():
                    chain_loss(x, None, None, xent_regularize=0.1 if xe is not None else 0.0, xent_input=xe)
