"""Which kernel ``tc_supervision_path_entropy`` takes and what workspace it asks for, without a GPU: handles with a sequence
beyond the resident kernel's rule ``32 * ceil4(states) + 4 * ceil4(pdfs) + 2048 <= 163840`` take
``num_entropy_large_kernels.hip``, whose means live in the workspace -- the value call's too.

The rule's edge with 8 pdfs is ``ceil4(states) <= 5055``: 5052 states is the largest resident handle (``32 * 5052 + 32 + 2048 =
163744``), and 5056 is already past it (``163872``), as is 5060."""
import ctypes as C

import numpy as np
import pytest

from torchain_amd import io
from torchain_amd._lib import lib

import e2e_large_cases as lc
import e2e_reference as e2e

UNSUPPORTED, WORKSPACE = -3, -4  # TC_ERR_*
# name: (FSTs, frames, pdfs, the kernel)
HANDLES = {
    "states5052": lambda: ([e2e.random_fst(5052, 16000, 8, np.random.default_rng(1))], 10, 8, 0),
    "states5056": lambda: ([e2e.random_fst(5056, 16000, 8, np.random.default_rng(1))], 10, 8, 1),
    "states5060": lambda: ([e2e.random_fst(5060, 16000, 8, np.random.default_rng(1)), e2e.random_fst(5, 12, 8, np.random.default_rng(2))], 10, 8, 1),
    "mixed_states": lambda: ([lc.mixed_fsts()[0]], lc.MIXED_T, lc.MIXED_P, 1),
    "mixed_pdfs": lambda: ([lc.mixed_fsts()[1]], lc.MIXED_T, lc.MIXED_P, 1),
    "mixed_both": lambda: (list(lc.mixed_fsts()), lc.MIXED_T, lc.MIXED_P, 1),
}


@pytest.mark.parametrize("name", list(HANDLES))
def test_kernel_and_workspace_of_a_handle(name):
    fsts, T, P, kernel = HANDLES[name]()
    sup = io.Supervision.from_e2e_fsts(1.0, T, P, fsts, any_size=True)
    states = sum(lc.sizes(f)[0] for f in fsts)
    need, need_grad = (int(lib.tc_supervision_path_entropy_workspace_bytes(sup.ptr, g)) for g in (0, 1))
    assert sup.path_entropy_kernel() == kernel
    if kernel == 0:
        assert need == 0 and need_grad >= 16 * T * states
        return
    assert need >= 16 * states and need_grad >= need + 16 * T * states  # (two mean rows; the history; one float an arc)
    # a workspace one byte short is refused before any launch
    counters = lambda: [int(lib.tc_debug_counter(k)) for k in (b"num_entropy_launches", b"num_entropy_large_launches")]  # noqa: E731
    fake, before = C.c_void_p(4096), counters()  # (never dereferenced)
    S = len(fsts)
    for grad, nbytes in ((None, need - 1), (fake, need_grad - 1)):
        assert lib.tc_supervision_path_entropy(sup.ptr, fake, 0, 0, S * T, P, P, fake, fake, grad, P, None, fake, nbytes, 0,
                                               None) == WORKSPACE
    assert lib.tc_supervision_path_entropy(sup.ptr, fake, 0, 0, S * T, P, P, fake, fake, None, P, None, None, 0, 0, None) == WORKSPACE
    assert min(before) >= 0 and counters() == before


def test_the_switch_moves_a_resident_handle_and_regular_ones_stay_refused():
    sup = io.Supervision.from_e2e_fsts(1.0, 5, 9, [e2e.random_fst(7, 25, 9, np.random.default_rng(3))] * 2)
    assert sup.path_entropy_kernel() == 0 and lib.tc_supervision_path_entropy_workspace_bytes(sup.ptr, 0) == 0
    assert lib.tc_debug_set(b"force_num_entropy_large", 1) == 0
    try:
        assert sup.path_entropy_kernel() == 1 and lib.tc_supervision_path_entropy_workspace_bytes(sup.ptr, 0) >= 16 * 14
    finally:
        assert lib.tc_debug_set(b"force_num_entropy_large", 0) == 0
    assert sup.path_entropy_kernel() == 0
    assert lib.tc_supervision_path_entropy_kernel(None) == -1
    from torchain_amd import synth
    regular = io.Supervision.from_synth(synth.random_supervision(synth.random_den_fst(20, 3, 10, seed=3), 2, 6, 2, seed=4))
    assert lib.tc_supervision_path_entropy_kernel(regular.ptr) == UNSUPPORTED
