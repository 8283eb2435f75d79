"""Best-path alignment without a GPU: the float64 reference of the GPU tests (``tests/best_path_reference.py``) against
brute-force enumeration of every path, and ``tc_supervision_best_path``'s export and argument checks, which the library
makes before its first device call."""
import ctypes as C

import numpy as np
import pytest

from torchain_amd import io, synth
from torchain_amd._lib import TC_DTYPE_BF16, TC_DTYPE_F16, TC_DTYPE_F32, lib

import best_path_reference as bp
import e2e_reference as ref

TC_ERR_INVALID_ARGUMENT = -1
P = 7


def _tiny_acceptors():
    """Acceptors of at most 5 states with cycles, parallel arcs of one pdf and several final states; and time-unfolded tries."""
    rng = np.random.default_rng(11)
    out = []
    for i in range(24):
        n = int(rng.integers(1, 6))
        out.append(ref.random_fst(n, int(rng.integers(n + 1, 9)), P, rng))
    den = synth.random_den_fst(6, 3, P, seed=2)
    for i, T in enumerate((1, 2, 3, 5)):
        sup = synth.random_supervision(den, 1, T, 2, seed=30 + i, final_weights=True)
        if sup.num_states <= 5 or T <= 2:
            out.append((sup.arc_begin, sup.ilabel, sup.arc_weight, sup.nextstate, sup.final))
    # a linear acceptor of 5 states: exactly one path, of 4 arcs
    out.append(ref._csr(5, [(i, i + 1, i % P, 0.5 * i) for i in range(4)], [np.inf] * 4 + [0.25]))
    return out


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_reference_agrees_with_enumeration_of_all_paths(T):
    rng = np.random.default_rng(100 + T)
    feasible = 0
    for fst in _tiny_acceptors():
        assert len(fst[-1]) <= 5
        y = (rng.normal(size=(T, P)) * 2.0).astype(np.float32)
        want, arg = bp.brute_force(fst, y)
        got = bp.best_score64(fst, y)
        if want == -np.inf:
            assert got == -np.inf
            continue
        feasible += 1
        # (the two add the same float64 terms in the same order along a path: no tolerance)
        assert got == want
        for pdfs in arg:
            assert bp.path_score64(fst, y, np.array(pdfs)) == want
        # a pdf sequence that no best path emits scores lower, one that no path emits at all -inf
        other = tuple((p + 1) % P for p in next(iter(arg)))
        if other not in arg:
            assert bp.path_score64(fst, y, np.array(other)) < want
    assert feasible >= 8
    # the linear acceptor has no path but at T = 4, and then one pdf sequence only
    linear = _tiny_acceptors()[-1]
    y = np.zeros((T, P), np.float32)
    assert (bp.best_score64(linear, y) > -np.inf) == (T == 4)
    if T == 4:
        assert bp.path_score64(linear, y, np.arange(4)) == -(0.0 + 0.5 + 1.0 + 1.5) - 0.25
        assert bp.path_score64(linear, y, np.array([0, 1, 2, 4])) == -np.inf


def test_split_of_a_merged_supervision_keeps_every_sequences_paths():
    den = synth.random_den_fst(40, 3, P, seed=4)
    S, T = 3, 4
    sup = synth.random_supervision(den, S, T, 3, seed=8)
    pieces = bp.split_merged(sup)
    assert len(pieces) == S
    y = synth.random_nnet_output(S, T, P, seed=9)
    merged = (sup.arc_begin, sup.ilabel, sup.arc_weight, sup.nextstate, sup.final)
    # the merged FST walks sequence after sequence: its best path is the sequences' best paths in a row
    in_a_row = np.concatenate([y[np.arange(T) * S + s] for s in range(S)])
    total = sum(bp.best_score64(piece, y[np.arange(T) * S + s]) for s, piece in enumerate(pieces))
    assert np.isfinite(total)
    assert abs(bp.best_score64(merged, in_a_row) - total) <= 1e-12 * abs(total)


def test_entry_is_exported():
    assert hasattr(lib, "tc_supervision_best_path")
    assert lib.tc_debug_counter(b"best_path_launches") >= 0  # (-1: an unknown key)


def test_bad_arguments_are_refused_before_any_device_call():
    S, T = 2, 5
    den = synth.random_den_fst(20, 3, P, seed=1)
    handles = [io.Supervision.from_synth(synth.random_supervision(den, S, T, 2, seed=3)),
               io.Supervision.from_e2e_fsts(1.0, T, P, ref.batch("random", S, P, seed=4)),
               io.Supervision.from_e2e_fsts(1.0, [T, 2], P, ref.batch("random", S, P, seed=4))]
    # host buffers of the right sizes: a call that is refused reads and writes none of them
    y = np.zeros((S * T, P), np.float32)
    pdfs = np.full(S * T, -7, np.int32)
    scores = np.full(S, 7.0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    launches = lib.tc_debug_counter(b"best_path_launches")

    def call(h, y_ptr=vp(y), dtype=TC_DTYPE_F32, bct=0, rows=S * T, cols=P, stride=P, pdf_ptr=vp(pdfs), score_ptr=vp(scores)):
        return lib.tc_supervision_best_path(h, y_ptr, dtype, bct, rows, cols, stride, pdf_ptr, score_ptr, 0, None)

    for h in handles:
        assert call(None) == TC_ERR_INVALID_ARGUMENT
        assert call(h.ptr, y_ptr=None) == TC_ERR_INVALID_ARGUMENT
        assert call(h.ptr, pdf_ptr=None) == TC_ERR_INVALID_ARGUMENT
        assert call(h.ptr, score_ptr=None) == TC_ERR_INVALID_ARGUMENT
        for bct in (0, 1):
            assert call(h.ptr, bct=bct, rows=S * T + 1) == TC_ERR_INVALID_ARGUMENT
            assert call(h.ptr, bct=bct, rows=S * T - S) == TC_ERR_INVALID_ARGUMENT
            assert call(h.ptr, bct=bct, cols=P + 1) == TC_ERR_INVALID_ARGUMENT
            assert call(h.ptr, bct=bct, cols=P - 1, stride=P) == TC_ERR_INVALID_ARGUMENT
            for dtype in (-1, 3, 100):
                assert call(h.ptr, bct=bct, dtype=dtype) == TC_ERR_INVALID_ARGUMENT
        for dtype in (TC_DTYPE_BF16, TC_DTYPE_F16):
            assert call(h.ptr, bct=0, dtype=dtype) == TC_ERR_INVALID_ARGUMENT
        assert call(h.ptr, stride=P - 1) == TC_ERR_INVALID_ARGUMENT
    assert (pdfs == -7).all() and (scores == 7.0).all()
    assert lib.tc_debug_counter(b"best_path_launches") == launches


def test_python_entry_checks_shape_and_device():
    import torch
    from torchain_amd.functions import best_path
    den = synth.random_den_fst(20, 3, P, seed=1)
    h = io.Supervision.from_synth(synth.random_supervision(den, 2, 5, 2, seed=3))
    with pytest.raises(ValueError):
        h.best_path(torch.zeros(10, P))  # not a CUDA tensor
    with pytest.raises(TypeError):
        best_path(torch.zeros(10, P), h.ptr)
