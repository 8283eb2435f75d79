"""The alignment entropy of end-to-end supervisions, without a GPU: the mean-form recursion of
``tests/num_entropy_reference.py`` (what the GPU tests compare with) against the list of every path of a tiny FST, and what
``tc_supervision_path_entropy`` refuses before any device call -- regular supervisions among it."""
import ctypes as C

import numpy as np
import pytest

from torchain_amd import io, synth
from torchain_amd._lib import lib

import num_entropy_reference as ner

INVALID, UNSUPPORTED, WORKSPACE = -1, -3, -4  # TC_ERR_*


@pytest.mark.parametrize("T", (1, 2, 5, 6))
def test_recursion_against_every_path(T):
    fst, y = ner.tiny_fst(), np.random.default_rng(T).normal(0.0, 2.0, size=(T, 4))
    h, logz, grad = ner.by_enumeration(fst, y)
    got = ner.by_recursion(fst, y)
    assert h > 0.1 and np.abs(grad).max() > 1e-2  # (the comparison is of something)
    assert abs(got["entropy"] - h) <= 1e-12 * T and abs(got["logprob"] - logz) <= 1e-12 * T
    assert np.abs(got["grad"] - grad).max() <= 1e-12 * T


def test_entry_checks_its_arguments_and_refuses_regular_supervisions():
    S, T, P = 2, 5, 4
    sup = io.Supervision.from_e2e_fsts(1.0, T, P, [ner.tiny_fst()] * S)
    need, need_grad = (int(lib.tc_supervision_path_entropy_workspace_bytes(sup.ptr, g)) for g in (0, 1))
    assert need == 0 and need_grad >= 16 * T * 3 * S  # (two doubles a (frame, state))
    assert lib.tc_supervision_path_entropy_workspace_bytes(None, 1) == INVALID
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails before a device call
    before = int(lib.tc_debug_counter(b"num_entropy_launches"))

    def call(s=sup.ptr, y=fake, dtype=0, bct=0, rows=S * T, cols=P, stride=P, ent=fake, lp=fake, grad=fake, gs=P, go=None,
             ws=fake, nbytes=need_grad):
        return lib.tc_supervision_path_entropy(s, y, dtype, bct, rows, cols, stride, ent, lp, grad, gs, go, ws, nbytes, 0, None)

    for bad in (dict(s=None), dict(y=None), dict(ent=None), dict(lp=None), dict(dtype=3), dict(dtype=1), dict(rows=S * T + 1),
                dict(cols=P + 1), dict(stride=P - 1), dict(gs=P - 1), dict(grad=None, go=fake), dict(y=C.c_void_p(4098)),
                dict(ent=C.c_void_p(4100)), dict(go=C.c_void_p(4100))):
        assert call(**bad) == INVALID, bad
    for bad in (dict(ws=None), dict(ws=C.c_void_p(4100)), dict(nbytes=need_grad - 1)):
        assert call(**bad) == WORKSPACE, bad
    fst = synth.random_den_fst(20, 3, 10, seed=3)
    regular = io.Supervision.from_synth(synth.random_supervision(fst, 2, 6, 2, seed=4))
    assert lib.tc_supervision_path_entropy_workspace_bytes(regular.ptr, 1) == UNSUPPORTED
    assert call(s=regular.ptr, rows=2 * 6, cols=10, stride=10, gs=10) == UNSUPPORTED
    assert before >= 0 and int(lib.tc_debug_counter(b"num_entropy_launches")) == before  # nothing was launched
