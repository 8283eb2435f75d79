"""The alignment entropy of regular supervisions, without a GPU: what ``tc_supervision_path_entropy_regular`` and its workspace
query answer from host arithmetic alone -- the history's size, end-to-end handles and levels beyond the size rule, bad
arguments -- all before any device call."""
import ctypes as C

import numpy as np
import pytest

from torchain_amd import io, synth
from torchain_amd._lib import lib

import num_entropy_reference as ner

INVALID, UNSUPPORTED, WORKSPACE = -1, -3, -4  # TC_ERR_*


@pytest.mark.parametrize("with_grad", (0, 1))
def test_entries_answer_before_any_device_call(with_grad):
    S, T, P = 2, 6, 10
    merged = synth.random_supervision(synth.random_den_fst(20, 3, P, seed=3), S, T, 2, seed=4)
    sup = io.Supervision.from_synth(merged)
    query = lib.tc_supervision_path_entropy_regular_workspace_bytes
    need = int(query(sup.ptr, with_grad))
    total_states = sup.stats()["history_bytes"] // 8  # (the numerator's history: one double a state)
    assert total_states >= merged.num_states and (need >= 16 * total_states if with_grad else need == 0)
    assert query(None, with_grad) == INVALID
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails before a device call
    before = int(lib.tc_debug_counter(b"num_entropy_regular_launches"))

    def call(s=sup.ptr, y=fake, dtype=0, bct=0, rows=S * T, cols=P, stride=P, ent=fake, lp=fake, gs=P, go=None, ws=fake,
             nbytes=need, grad=fake if with_grad else None):
        return lib.tc_supervision_path_entropy_regular(s, y, dtype, bct, rows, cols, stride, ent, lp, grad, gs, go, ws, nbytes, 0,
                                                       None)

    for bad in (dict(s=None), dict(y=None), dict(ent=None), dict(lp=None), dict(dtype=3), dict(dtype=1), dict(rows=S * T + 1),
                dict(cols=P + 1), dict(stride=P - 1), dict(y=C.c_void_p(4098)), dict(ent=C.c_void_p(4100)),
                dict(lp=C.c_void_p(4100))) + ((dict(gs=P - 1), dict(go=C.c_void_p(4100))) if with_grad else (dict(go=fake),)):
        assert call(**bad) == INVALID, bad  # (the last: a grad_output without a gradient)
    for bad in (dict(ws=None), dict(ws=C.c_void_p(4100)), dict(nbytes=need - 1)) if with_grad else ():
        assert call(**bad) == WORKSPACE, bad
    e2e = io.Supervision.from_e2e_fsts(1.0, T, 4, [ner.tiny_fst()] * S)
    assert query(e2e.ptr, with_grad) == UNSUPPORTED and call(s=e2e.ptr, cols=4, stride=4, gs=4) == UNSUPPORTED
    # one frame whose level of 4000 states breaks 48 * L + 4 * U + 4 * A + 2048 <= 163840 (the numerator itself takes it)
    L = 4000
    wide = io.Supervision.from_fst(1.0, 1, 1, P, np.r_[0, np.full(L + 1, L)], np.ones(L, np.int32), np.zeros(L, np.float32),
                                   np.arange(1, L + 1), np.r_[np.inf, np.zeros(L)])
    assert wide.stats()["kernel"] == "resident"
    assert query(wide.ptr, with_grad) == UNSUPPORTED and call(s=wide.ptr, rows=1) == UNSUPPORTED
    assert before >= 0 and int(lib.tc_debug_counter(b"num_entropy_regular_launches")) == before  # nothing was launched
