"""``xent_log_softmax`` without a GPU (cases: ``tests/xent_log_softmax_cases.py``): the float64 numpy statement of the contract
against torch's CPU float64 autograd, keyword validation before any library call, the C entry in header and library, and the
workspace sizes -- the older entries' unchanged, the new one's with room for the row statistics."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from torchain_amd import functions, io, parallel
from torchain_amd._lib import LIB_PATH, TC_DTYPE_BF16, TC_DTYPE_F16, TC_DTYPE_F32, lib

import xent_log_softmax_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "torchain_hip.h")


@pytest.mark.parametrize("name", xc.CASES)
def test_numpy_statement_is_the_gradient_of_the_log_softmax_objective(name):
    """``grad64`` / ``objective64`` against autograd of ``sum(wgamma * log_softmax(x))`` in float64 on the CPU, to 1e-12 of
    the largest row mass: V = -xent_regularize * dw * wgamma is the gradient the library descends along, so G is
    -xent_regularize * dw[row] times the objective's gradient."""
    S, T, P = xc.SHAPES[name]
    wg = xc.random_wgamma(name)
    x = np.asarray(xc.xent_input(name), np.float64)
    dw = np.random.default_rng(5).uniform(0.25, 2.0, size=S * T)
    dw[4 % (S * T)] = 0.0
    xt = torch.from_numpy(x).requires_grad_(True)
    objf = (torch.from_numpy(wg) * torch.log_softmax(xt, dim=1)).sum()
    objf.backward()
    want_objf = float(objf.detach())
    got_objf = xc.objective64(wg, x)
    assert abs(got_objf - want_objf) <= 1e-12 * abs(want_objf), (got_objf, want_objf)
    V = -xc.XREG * dw[:, None] * wg
    want = -xc.XREG * dw[:, None] * xt.grad.numpy()
    got = xc.grad64(V, x)
    err = np.abs(got - want).max() / xc.row_mass(V)
    print("%s: objective %.15g (autograd %.15g), gradient error / row mass %.3g" % (name, got_objf, want_objf, err))
    assert err <= 1e-12
    # live rows sum to 0; the row of no mass and the row of deriv_weight 0 are exactly +0, also under a NaN in x
    assert np.abs(got.sum(axis=1)).max() <= 1e-12 * xc.row_mass(V)
    poisoned = x.copy()
    poisoned[3] = np.nan
    poisoned[4 % (S * T)] = np.nan
    again = xc.grad64(V, poisoned)
    for r in {3, 4 % (S * T)}:
        assert not again[r].any() and not np.signbit(again[r]).any()
    keep = np.ones(S * T, bool)
    keep[[3, 4 % (S * T)]] = False
    assert np.array_equal(again[keep], got[keep])


def test_keyword_is_checked_before_any_library_call():
    """A value that is not a bool, and ``kaldi_way=False`` with the option, are ValueErrors raised in front of everything else
    (CPU tensors and a graph that is none reach no further check)."""
    x = torch.zeros(4, 3)
    for fn in (functions.chain_loss, parallel.chain_loss_data_parallel):
        for bad in (1, 0, "yes", None, 1.0, np.True_):
            with pytest.raises(ValueError, match="xent_log_softmax"):
                fn(x, None, None, xent_regularize=0.1, xent_input=x, kaldi_way=True, xent_log_softmax=bad)
        with pytest.raises(ValueError, match="kaldi_way"):
            fn(x, None, None, xent_regularize=0.1, xent_input=x, kaldi_way=False, xent_log_softmax=True)
        with pytest.raises(ValueError, match="kaldi_way"):
            fn(x, None, None, xent_log_softmax=True)  # (kaldi_way defaults to False)
    assert functions._xent_options({}, False) is False
    assert functions._xent_options({"xent_log_softmax": False}, False) is False
    rest = {"xent_log_softmax": True, "out_of_range_regularize": 0.5}
    assert functions._xent_options(rest, True) is True and rest == {"out_of_range_regularize": 0.5}
    with pytest.raises(TypeError, match="unexpected keyword"):
        functions.chain_loss(x, None, None, xent_logsoftmax=True)


def test_header_declares_and_library_exports_the_entry():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int tc_chain_step_log_softmax\((.*?)\);", code, flags=re.S)
    assert m, "tc_chain_step_log_softmax is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    older = [p.strip() for p in re.search(r"int tc_chain_step_per_sequence\((.*?)\);", code, flags=re.S).group(1).split(",")]
    assert params[:len(older)] == older and params[len(older):] == ["int xent_log_softmax"]
    assert re.search(r"int64_t tc_chain_step_log_softmax_workspace_bytes\(", code)
    dll = C.CDLL(LIB_PATH)
    assert hasattr(dll, "tc_chain_step_log_softmax") and hasattr(dll, "tc_chain_step_log_softmax_workspace_bytes")
    assert len(lib.tc_chain_step_log_softmax.argtypes) == len(lib.tc_chain_step_per_sequence.argtypes) + 1
    doc = text[:text.index("int64_t tc_chain_step_log_softmax_workspace_bytes(")].rsplit("/*", 1)[1]
    for word in ("xent_log_softmax", "log-softmax", "torchain/functions.py:88-89", "forward.py:67", "stream capture", "select",
                 "xent_log_softmax_launches", "TC_ERR_INVALID_ARGUMENT"):
        assert word in doc, word
    assert lib.tc_debug_counter(b"xent_log_softmax_launches") == 0  # (a known key; nothing has been launched here)


def _align256(n):
    return (n + 255) & ~255


@pytest.mark.parametrize("name", ("ragged_float4", "tile_edge"))
def test_workspace_sizes(name):
    """The older entries' sizes by the formula they had -- the objective's workspace, the scratch of the xent objective, then
    one float32 matrix for each of: the frame-major copies of input and gradient (3-D or 16-bit), the copy of xent_input
    (with them and the xent branch), the float32 xent gradient (16-bit and the xent branch).  The new entry's: that, plus
    two floats a row behind it with the xent branch -- at least the ``4 * S * T`` the statistics cannot do without."""
    S, T, P = xc.SHAPES[name]
    g = io.DenominatorGraph(xc.den_fst(name), P)
    for s, t in ((S, T), (4, 9)):
        chain = lib.tc_chain_workspace_bytes(g.ptr, s, t)
        assert chain > 0 and chain % 256 == 0
        base = lib.tc_chain_step_workspace_bytes(g.ptr, s, t, 0, 0)
        assert base > chain and (base - chain) % 256 == 0  # (the scratch of the xent objective: the same for every shape)
        assert base - chain == lib.tc_chain_step_workspace_bytes(g.ptr, 1, 1, 0, 0) - lib.tc_chain_workspace_bytes(g.ptr, 1, 1)
        mat = _align256(s * t * P * 4)
        for three_d in (0, 1):
            for xent in (0, 1):
                for dtype in (TC_DTYPE_F32, TC_DTYPE_BF16, TC_DTYPE_F16):
                    half = dtype != TC_DTYPE_F32
                    copies = bool(three_d) or half
                    want = base + mat * ((2 if copies else 0) + (1 if copies and xent else 0) + (1 if half and xent else 0))
                    assert lib.tc_chain_step_typed_workspace_bytes(g.ptr, s, t, three_d, xent, dtype) == want
                    if not half:
                        assert lib.tc_chain_step_workspace_bytes(g.ptr, s, t, three_d, xent) == want
                    for layout in ((0,) if not three_d else (1, 2)):
                        assert lib.tc_chain_step_strided_workspace_bytes(g.ptr, s, t, layout, xent, dtype) == want
                        new = lib.tc_chain_step_log_softmax_workspace_bytes(g.ptr, s, t, layout, xent, dtype)
                        assert new == want + (_align256(8 * s * t) if xent else 0)
                        assert new >= want + (4 * s * t if xent else 0)
    assert lib.tc_chain_step_log_softmax_workspace_bytes(g.ptr, S, T, 3, 1, TC_DTYPE_F32) < 0
    assert lib.tc_chain_step_log_softmax_workspace_bytes(g.ptr, 0, T, 0, 1, TC_DTYPE_F32) < 0
    assert lib.tc_chain_step_log_softmax_workspace_bytes(g.ptr, S, T, 0, 1, 7) < 0
