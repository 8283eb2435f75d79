"""End-to-end supervisions of any size on the host (``tc_supervision_create_e2e_any``, ``tc_supervision_e2e_stats``,
``io.Supervision.from_e2e_fsts(..., any_size=True)``): creation at and past the resident kernel's limits and the new LDS rule,
the order of errors, the unchanged default, ragged handles and acceptors composed with a denominator graph."""
import ctypes as C

import numpy as np
import pytest

from torchain_amd import egs, io
from torchain_amd._lib import TorchainHipError, lib

import den_compose_cases as dc
import e2e_large_cases as lc
import e2e_reference as ref
from test_e2e_host import _loop_fst, _mutate, _sized

BAD_FST, UNSUPPORTED, INVALID = -2, -3, -1


def _make(fsts, T=10, P=1032, any_size=True, **kw):
    return io.Supervision.from_e2e_fsts(1.0, T, P, fsts, any_size=any_size, **kw)


def _code(fsts, **kw):
    with pytest.raises(TorchainHipError) as ei:
        _make(fsts, **kw)
    return ei.value.code


@pytest.mark.parametrize("what", ["states", "arcs", "pdfs"])
def test_one_past_each_resident_limit_is_taken(what):
    big = lc.planted(*lc.ONE_PAST[what], num_pdfs=1032, seed=3)
    assert lc.sizes(big) == lc.ONE_PAST[what]
    sup = _make([_loop_fst(), big])
    assert sup.is_e2e and sup.shape == (2, 10, 1032)
    st = sup.e2e_stats()
    assert st["kernel"] == "large" and st["route"] == 1 and st["sequences"] == 2
    assert (st["max_states"], st["max_arcs"], st["max_pdfs"]) == lc.ONE_PAST[what]
    n4, p4 = (st["max_states"] + 3) // 4 * 4, (st["max_pdfs"] + 3) // 4 * 4
    assert st["large_lds_bytes"] == 16 * n4 + 4 * p4 == lc.lds_rule(st["max_states"], st["max_pdfs"]) - 2048
    assert st["resident_lds_bytes"] == st["large_lds_bytes"] + 4 * st["max_arcs"]
    # scratch: (T + 1) x states doubles, T x distinct pdfs floats, one float per arc, each rounded up to 256 bytes
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    states, arcs, pdfs = (a + b for a, b in zip(lc.ONE_PAST[what], (3, 3, 1)))
    assert st["scratch_bytes"] == up(11 * states * 8) + up(10 * pdfs * 4) + up(arcs * 4)
    # the default call still refuses it
    assert _code([_loop_fst(), big], any_size=False) == UNSUPPORTED


def test_a_batch_within_the_limits_is_the_resident_handle():
    at = lc.planted(lc.MAX_STATES, lc.MAX_ARCS, lc.MAX_PDFS, num_pdfs=1032, seed=4)
    a, b = _make([_loop_fst(), at]), _make([_loop_fst(), at], any_size=False)
    st = a.e2e_stats()
    assert st == b.e2e_stats() and st["kernel"] == "resident" and st["route"] == 0
    up = lambda x: (x + 255) // 256 * 256  # noqa: E731
    assert st["scratch_bytes"] == up(11 * (lc.MAX_STATES + 3) * 8) + up(10 * (lc.MAX_PDFS + 1) * 4)  # (no arc occupations)
    # the switch that sends such a handle to the large kernel shows in the route (and in the slot's size)
    assert lib.tc_debug_set(b"force_num_e2e_large", 1) == 0
    try:
        forced = a.e2e_stats()
    finally:
        assert lib.tc_debug_set(b"force_num_e2e_large", 0) == 0
    assert forced["kernel"] == "large" and forced["scratch_bytes"] == st["scratch_bytes"] + up(4 * (lc.MAX_ARCS + 3))
    assert a.e2e_stats() == st


@pytest.mark.parametrize("at,past", [((8192, 9000, 7680), (8192, 9000, 7681)), ((8192, 9000, 7680), (8193, 9000, 7680)),
                                     ((10108, 12000, 4), (10109, 12000, 4))])
def test_the_lds_rule_at_and_one_past(at, past):
    """A ring plus extra arcs, as ``test_e2e_host._sized`` builds its sequences; the arc count is not limited."""
    P = 7700
    assert lc.lds_rule(at[0], at[2]) <= lc.LDS_LIMIT < lc.lds_rule(past[0], past[2])
    fst = _sized(*at)
    assert lc.sizes(fst) == at
    sup = _make([_loop_fst(), fst], P=P)
    assert sup.e2e_stats()["kernel"] == "large" and sup.e2e_stats()["large_lds_bytes"] + 2048 <= lc.LDS_LIMIT
    fst = _sized(*past)
    assert lc.sizes(fst) == past
    assert _code([_loop_fst(), fst], P=P) == UNSUPPORTED
    assert _code([fst, _loop_fst()], P=P) == UNSUPPORTED


def test_the_rule_is_per_sequence():
    """The largest state count and the largest pdf count of a batch may belong to two sequences, each at the rule."""
    for sizes in (lc.MIXED, ((9000, 9500, 500), (5000, 6000, 4500))):
        assert all(lc.lds_rule(n, d) <= lc.LDS_LIMIT for n, _, d in sizes)
        assert lc.lds_rule(max(n for n, _, _ in sizes), max(d for _, _, d in sizes)) > lc.LDS_LIMIT
        for order in (sizes, sizes[::-1]):
            st = _make([_sized(*z) for z in order], P=lc.MIXED_P).e2e_stats()
            assert st["kernel"] == "large"
            assert (st["max_states"], st["max_pdfs"]) == (max(n for n, _, _ in sizes), max(d for _, _, d in sizes))
            assert st["large_lds_bytes"] == max(lc.lds_rule(n, d) for n, _, d in sizes) - 2048 <= lc.LDS_LIMIT - 2048


def test_many_arcs_are_not_a_size():
    fst = _sized(300, 200000, 50)
    assert lc.sizes(fst) == (300, 200000, 50)
    st = _make([fst], T=3, P=50).e2e_stats()
    assert st["kernel"] == "large" and st["max_arcs"] == 200000


def test_bad_fst_wins_over_size():
    big = _sized(*lc.ONE_PAST["states"])
    too_big = _sized(10109, 12000, 4)
    bad = _mutate(2, 0, 0)  # (an epsilon arc)
    assert _code([too_big, bad, big]) == BAD_FST
    assert _code([bad, too_big]) == BAD_FST
    assert _code([too_big, _mutate(4, 0, 3)]) == BAD_FST  # (a next state out of range)
    no_final = _mutate(5, 0, np.inf, fst=big)
    assert _code([_loop_fst(), no_final]) == BAD_FST
    assert _code([too_big, _loop_fst()]) == UNSUPPORTED


def test_scratch_and_minibatch_rules_still_refuse():
    big = _sized(*lc.ONE_PAST["states"])
    # (T + 1) x states x 8 bytes of history above 4 GiB
    T = (4 << 30) // (8 * 2049) + 1
    assert _code([big], T=T) == UNSUPPORTED
    assert _make([big], T=T // 2).n_frame == T // 2
    # sequences x frames above 2^26
    assert _code([_loop_fst()] * 2, T=(1 << 25) + 1, P=50) == UNSUPPORTED


@pytest.mark.parametrize("what", ["states", "arcs", "pdfs"])
def test_default_call_is_unchanged(what):
    past = _sized(*lc.ONE_PAST[what])
    assert _code([_loop_fst(), past], any_size=False) == UNSUPPORTED
    assert _code([_loop_fst(), past], T=[4, 10], any_size=False) == UNSUPPORTED
    assert _make([_loop_fst(), past], T=[4, 10]).e2e_stats()["kernel"] == "large"


def test_null_and_argument_checks_of_the_new_entries():
    h = C.c_void_p()
    z = np.zeros(4, np.int32)
    zp = z.ctypes.data
    f = lib.tc_supervision_create_e2e_any
    assert f(None, 1.0, 1, 5, None, 10, zp, zp, zp, None, None, None, zp) == INVALID
    assert f(C.byref(h), 1.0, 0, 5, None, 10, zp, zp, zp, None, None, None, zp) == INVALID      # no sequences
    assert f(C.byref(h), 1.0, 1, 0, None, 10, zp, zp, zp, None, None, None, zp) == INVALID      # no frames
    assert f(C.byref(h), 1.0, 1, 5, None, 0, zp, zp, zp, None, None, None, zp) == INVALID       # no labels
    assert f(C.byref(h), 1.0, 1, 5, None, 10, None, zp, zp, None, None, None, zp) == INVALID
    assert f(C.byref(h), 1.0, 1, 5, None, 10, zp, None, zp, None, None, None, zp) == INVALID
    assert f(C.byref(h), 1.0, 1, 5, None, 10, zp, zp, None, None, None, None, zp) == INVALID
    assert f(C.byref(h), 1.0, 1, 5, None, 10, zp, zp, zp, None, None, None, None) == INVALID
    assert f(C.byref(h), 1.0, 1, 5, zp, 10, zp, zp, zp, None, None, None, zp) == INVALID        # a length of 0 frames
    assert f(C.byref(h), 1.0, 0, 5, zp, 10, zp, zp, zp, None, None, None, zp) == INVALID
    assert not h
    # arcs without their arrays
    sb, ab = np.array([0, 1], np.int32), np.array([0, 1], np.int32)
    fin = np.zeros(1, np.float32)
    assert f(C.byref(h), 1.0, 1, 5, None, 10, sb.ctypes.data, zp, ab.ctypes.data, None, None, None, fin.ctypes.data) == INVALID
    out = np.zeros(8, np.int64)
    g = lib.tc_supervision_e2e_stats
    assert g(None, out.ctypes.data) == INVALID
    sup = _make([_loop_fst()], P=50)
    assert g(sup.ptr, None) == INVALID
    assert g(sup.ptr, out.ctypes.data) == 0 and out[0] == 1 and out[7] == 0
    # a regular handle: its own stats entry, and the other way round
    from torchain_amd import synth
    fst = synth.random_den_fst(20, 3, 10, seed=2)
    reg = io.Supervision.from_synth(synth.random_supervision(fst, 2, 6, 2, seed=3))
    assert g(reg.ptr, out.ctypes.data) == INVALID
    with pytest.raises(TorchainHipError):
        reg.e2e_stats()
    with pytest.raises(TorchainHipError):
        sup.stats()
    with pytest.raises(ValueError):
        io.Supervision.from_e2e_fsts(1.0, 5, 10, [], any_size=True)
    header = open(io.__file__.replace("io.py", "../include/torchain_hip.h")).read()
    for name in ("tc_supervision_create_e2e_any", "tc_supervision_e2e_stats", '"force_num_e2e_large"', '"num_e2e_large_launches"'):
        assert name in header
    assert lib.tc_debug_counter(b"num_e2e_large_launches") >= 0


def test_ragged_any_size_handle():
    big = _sized(*lc.ONE_PAST["arcs"])
    lens = [37, 1, 20, 5]
    sup = _make([_loop_fst(), _loop_fst(), big, _loop_fst()], T=lens)
    assert sup.is_ragged and sup.is_e2e and sup.n_frame == 37
    assert sup.frames.tolist() == lens
    assert sup.e2e_stats()["kernel"] == "large"
    uniform = _make([_loop_fst(), big], T=20)
    assert not uniform.is_ragged and uniform.frames.tolist() == [20, 20]
    equal = _make([_loop_fst(), big], T=[20, 20])
    assert equal.is_ragged
    with pytest.raises(ValueError):
        _make([_loop_fst(), big], T=[20])


def test_from_synth_passes_any_size_on():
    big = _sized(*lc.ONE_PAST["pdfs"])
    e = egs.E2eSup(weight=1.0, num_sequences=2, frames_per_sequence=10, label_dim=1032, fsts=[_loop_fst(), big])
    with pytest.raises(TorchainHipError) as ei:
        io.Supervision.from_synth(e)
    assert ei.value.code == UNSUPPORTED
    assert io.Supervision.from_synth(e, any_size=True).e2e_stats()["kernel"] == "large"


def test_composed_acceptor_beyond_the_resident_limits():
    fst = lc.composed_input()
    g = dc.graph(lc.COMPOSED_GRAPH)
    out, info = g.normalize_fsts([fst], e2e=True)
    assert info["status"][0] == 0 and info["states_in"][0] == 60 <= lc.MAX_STATES < info["states_out"][0]
    assert io.Supervision.from_e2e_fsts(1.0, lc.COMPOSED_T, dc.P, [fst]).e2e_stats()["kernel"] == "resident"
    with pytest.raises(TorchainHipError) as ei:
        io.Supervision.from_e2e_fsts(1.0, lc.COMPOSED_T, dc.P, [fst], den_graph=g)
    assert ei.value.code == UNSUPPORTED
    for T in (lc.COMPOSED_T, [lc.COMPOSED_T]):
        sup = io.Supervision.from_e2e_fsts(1.0, T, dc.P, [fst], den_graph=g, any_size=True)
        st = sup.e2e_stats()
        assert st["kernel"] == "large" and st["max_states"] == info["states_out"][0] and st["max_arcs"] == info["arcs_out"][0]
