"""Host side of ``tc_supervision_arc_posteriors_regular``: its two size rules at their edges, its workspace, the arc list of
``tc_supervision_arcs`` against the caller's FSTs, and the refusals of end-to-end handles.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from torchain_amd import io
from torchain_amd._lib import lib

import e2e_reference as e2e
from test_gpu_num_arc_post_regular import EXTRA
from test_gpu_num_entropy_regular import _setup

LIMIT, U = 163840, 4
r2, r4, r256 = (lambda x: x + 1 & ~1), (lambda x: x + 3 & ~3), (lambda x: x + 255 & ~255)


def fan(arcs, states):
    """one frame: ``arcs`` arcs from the start state, dealt over ``states`` final states and ``U`` pdfs"""
    k = np.arange(arcs)
    fst = (np.r_[0, np.full(states + 1, arcs)], 1 + k % U, np.zeros(arcs), 1 + np.sort(k % states), np.r_[np.inf, np.zeros(states)])
    return io.Supervision.from_fsts(1.0, [1], U, [tuple(np.asarray(a, t) for a, t in zip(fst, "iifif"))])


def test_size_rules_at_their_edges_and_workspace():
    kernel, need = lib.tc_supervision_arc_posteriors_regular_kernel, lib.tc_supervision_arc_posteriors_regular_workspace_bytes
    last_a = (LIMIT - 2048 - 24 * r2(2) - 4 * r4(U)) // 8  # the last A with resident terms beside L = 2 (a multiple of 4)
    last_l = (LIMIT - 2048 - 4 * r4(U)) // 24 & ~1         # the last L the spill rule admits
    assert 24 * r2(2) + 8 * last_a + 4 * r4(U) + 2048 <= LIMIT < 24 * r2(2) + 8 * r4(last_a + 1) + 4 * r4(U) + 2048
    assert 24 * last_l + 4 * r4(U) + 2048 <= LIMIT < 24 * r2(last_l + 1) + 4 * r4(U) + 2048
    resident, spills, widest, refused = fan(last_a, 2), fan(last_a + 1, 2), fan(last_l, last_l), fan(last_l + 1, last_l + 1)
    assert [kernel(s.ptr) for s in (resident, spills, widest, refused)] == [0, 1, 1, -3]  # (-3: TC_ERR_UNSUPPORTED)
    assert need(resident.ptr) == r256(8 * 3) and need(spills.ptr) == r256(8 * 3) + r256(8 * (last_a + 1))
    assert need(widest.ptr) == r256(8 * (last_l + 1)) + r256(8 * last_l) and need(refused.ptr) == -3
    sup = io.Supervision.from_synth(EXTRA["spill_only"]())  # beyond the resident rule, within the numerator's
    assert kernel(sup.ptr) == 1 and sup.stats()["kernel"] in ("resident", "windowed") and sup.stats()["max_level_arcs"] == 20800
    assert lib.tc_debug_set(b"force_num_arc_post_regular_spill", 1) == 0
    try:
        assert kernel(resident.ptr) == 1 and need(resident.ptr) == r256(8 * 3) + r256(8 * last_a)
    finally:
        assert lib.tc_debug_set(b"force_num_arc_post_regular_spill", 0) == 0


@pytest.mark.parametrize("case", ["trie7", "merged", "ragged"])
def test_arcs_are_the_callers_fsts_in_their_order(case):
    sup, _, frames, _, fsts = _setup(case)
    arc, off = sup.arcs(), np.zeros(len(fsts) + 1, np.int64)
    assert lib.tc_supervision_arc_posteriors_offsets(sup.ptr, off.ctypes.data_as(C.c_void_p), np.zeros_like(off).ctypes.data_as(C.c_void_p)) == 0
    for s, (_, ab, il, cost, nxt, final) in enumerate(fsts):
        src = np.repeat(np.arange(len(final)), np.diff(ab))
        time = np.zeros(len(final), np.int64)
        for a in range(len(src)):
            time[nxt[a]] = time[src[a]] + 1
        got = [getattr(arc, k)[off[s]:off[s + 1]] for k in arc._fields]
        want = [np.full(len(src), s), time[src], src, nxt, il - 1, -np.asarray(cost, np.float32)]
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and time[src].max() == frames[s] - 1


def test_end_to_end_handles_are_refused():
    sup = io.Supervision.from_e2e_fsts(1.0, 5, 9, [e2e.random_fst(6, 20, 9, np.random.default_rng(5))])
    assert lib.tc_supervision_arc_posteriors_regular_kernel(sup.ptr) == -3
    assert lib.tc_supervision_arc_posteriors_regular_workspace_bytes(sup.ptr) == -3
    assert lib.tc_supervision_arcs(sup.ptr, None, None, None, None, None, None) == -3
    fake = C.c_void_p(4096)  # (refused by the handle's kind, in front of the first device call: nothing is dereferenced)
    assert lib.tc_supervision_arc_posteriors_regular(sup.ptr, fake, 0, 0, 5, 9, 9, fake, fake, fake, fake, 1 << 20, 0, None) == -3
