"""The wide-level route of ``tc_supervision_path_entropy_regular`` without a GPU: what the kernel query, the workspace query and
the entry answer from host arithmetic alone for the 4000-state one-frame handle of ``tests/test_num_entropy_regular_host.py``,
built with and without ``any_width=True`` -- all before any device call."""
import ctypes as C

import numpy as np

from torchain_amd import io
from torchain_amd._lib import lib

import num_entropy_reference as ner

INVALID, UNSUPPORTED, WORKSPACE = -1, -3, -4  # TC_ERR_*
L, P = 4000, 10


def _handle(**kw):
    return io.Supervision.from_fst(1.0, 1, 1, P, np.r_[0, np.full(L + 1, L)], np.ones(L, np.int32), np.zeros(L, np.float32),
                                   np.arange(1, L + 1), np.r_[np.inf, np.zeros(L)], **kw)


def test_a_wide_level_is_answered_only_with_any_width():
    query, kernel = lib.tc_supervision_path_entropy_regular_workspace_bytes, lib.tc_supervision_path_entropy_regular_kernel
    counters = lambda: [int(lib.tc_debug_counter(k)) for k in (b"num_entropy_wide_launches", b"num_entropy_regular_launches")]  # noqa: E731
    before = counters()
    assert min(before) >= 0 and lib.tc_debug_counter(b"num_entropy_wide_launchez") == -1
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails before a device call

    def call(sup, nbytes, grad=fake, cols=P):
        return lib.tc_supervision_path_entropy_regular(sup.ptr, fake, 0, 0, 1, cols, cols, fake, fake, grad, cols, None, fake, nbytes, 0, None)

    wide, plain = _handle(any_width=True), _handle()
    value, with_grad = int(query(wide.ptr, 0)), int(query(wide.ptr, 1))
    assert wide.path_entropy_regular_kernel() == 1
    assert value >= 2 * 16 * L and with_grad >= value + 16 * (L + 1)  # two level rows of pairs; the history beside them
    assert call(wide, value - 1, grad=None) == WORKSPACE and call(wide, with_grad - 1) == WORKSPACE
    assert kernel(plain.ptr) == query(plain.ptr, 0) == query(plain.ptr, 1) == call(plain, 1 << 30) == UNSUPPORTED
    e2e = io.Supervision.from_e2e_fsts(1.0, 6, 4, [ner.tiny_fst()] * 2)
    assert kernel(e2e.ptr) == UNSUPPORTED and kernel(None) == INVALID
    try:  # the switches: known keys, read by the queries; the plain handle is then served too
        assert lib.tc_debug_set(b"force_num_entropy_wide_", 1) == lib.tc_debug_set(b"force_num_entropy_wide_streamed_", 1) == INVALID
        assert lib.tc_debug_set(b"force_num_entropy_wide", 1) == 0 and kernel(plain.ptr) == 1 and query(plain.ptr, 0) == value
        assert lib.tc_debug_set(b"force_num_entropy_wide_streamed", 1) == 0 and kernel(plain.ptr) == kernel(wide.ptr) == 2
        assert query(wide.ptr, 1) == with_grad and kernel(e2e.ptr) == UNSUPPORTED
    finally:
        assert lib.tc_debug_set(b"force_num_entropy_wide", 0) == lib.tc_debug_set(b"force_num_entropy_wide_streamed", 0) == 0
    assert kernel(plain.ptr) == UNSUPPORTED and counters() == before  # nothing was launched
