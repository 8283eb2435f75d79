"""Host side of the level-windowed numerator (no GPU): ``io.Supervision.stats()`` / ``tc_supervision_stats`` against a numpy
count from the merged FST, the kernel each supervision of ``wide_supervisions`` will take, and the diagnostics."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from torchain_amd import io
from torchain_amd._lib import lib

import e2e_reference as ref
import wide_supervisions as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TC_ERR_INVALID_ARGUMENT, TC_ERR_UNSUPPORTED = -1, -3


@pytest.mark.parametrize("name", ws.CASES)
def test_stats_match_a_numpy_count_of_the_fst(name):
    """Every case: accepted by tc_supervision_create (distinct final weights, a level of one state between wide ones
    included), and every size and both LDS figures as counted from the FST."""
    sup = ws.supervision(name)
    got = io.Supervision.from_synth(sup).stats()
    want = ws.count_stats(sup)
    print(name, got)
    for key, value in want.items():
        assert got[key] == value, (name, key, got[key], value)
    assert got["route"] == (0 if want["kernel"] == ws.RESIDENT else 1)


@pytest.mark.parametrize("name", ws.CASES)
def test_route(name):
    """(150 frames, 40 paths) still fits the resident kernel; 64 paths, 600 x 16, 1500 x 8, 3000 x 4 and the wide, long,
    pinched and mixed lattices do not, and their widest level fits LDS many times over."""
    st = io.Supervision.from_synth(ws.supervision(name)).stats()
    assert st["kernel"] == ws.expected_kernel(name), st
    if name in ws.WIDE:
        assert st["resident_lds_bytes"] > ws.LDS_LIMIT and st["windowed_lds_bytes"] < ws.LDS_LIMIT // 4, st
    else:
        assert st["resident_lds_bytes"] <= ws.LDS_LIMIT, st
    assert st["history_bytes"] >= 8 * st["max_states"]


def test_issue_table_sizes():
    """The sizes that motivated the kernel: 40 paths of 150 frames lie just under the limit, 64 paths well above."""
    a = io.Supervision.from_synth(ws.supervision("trie_150x40")).stats()
    b = io.Supervision.from_synth(ws.supervision("trie_150x64")).stats()
    assert 5900 <= a["max_states"] <= 6001 and 0.8 * ws.LDS_LIMIT < a["resident_lds_bytes"] <= ws.LDS_LIMIT
    assert 9400 <= b["max_states"] <= 9601 and b["max_level_states"] <= 64
    wide = io.Supervision.from_synth(ws.supervision("lattice_wide")).stats()
    assert wide["max_states"] > 10000 and wide["resident_lds_bytes"] > 2 * ws.LDS_LIMIT
    bursty = io.Supervision.from_synth(ws.supervision("lattice_bursty")).stats()
    assert bursty["max_level_states"] == 400 and bursty["max_level_states"] > wide["max_level_states"]


def test_a_single_level_beyond_lds_is_reported_unsupported():
    """One level of 12000 states: the sequence does not fit the resident kernel (16 bytes a state) and the level does not
    fit the window (32 bytes a state)."""
    sup = ws.lattice_supervision(1, 3, ws.P, lambda q, t, r: 12000 if t == 2 else 4, 1, seed=1)
    st = io.Supervision.from_synth(sup).stats()
    assert st["max_level_states"] == 12000 and st["resident_lds_bytes"] > ws.LDS_LIMIT and st["route"] == TC_ERR_UNSUPPORTED and st["kernel"] == "unsupported"


def test_e2e_supervisions_have_no_levels():
    sup = io.Supervision.from_e2e_fsts(1.0, 20, 30, ref.batch("chain", 2, 30, seed=3))
    out = np.zeros(12, np.int64)
    assert lib.tc_supervision_stats(sup.ptr, out.ctypes.data_as(C.c_void_p)) == TC_ERR_INVALID_ARGUMENT
    with pytest.raises(Exception):
        sup.stats()
    assert lib.tc_supervision_stats(None, out.ctypes.data_as(C.c_void_p)) == TC_ERR_INVALID_ARGUMENT
    reg = io.Supervision.from_synth(ws.supervision("trie_150x3"))
    assert lib.tc_supervision_stats(reg.ptr, None) == TC_ERR_INVALID_ARGUMENT


def test_switch_and_counter_exist():
    assert lib.tc_debug_counter(b"num_windowed_launches") >= 0
    assert lib.tc_debug_counter(b"num_windowed_launchez") == -1
    assert lib.tc_debug_set(b"force_num_windowed_", 1) == TC_ERR_INVALID_ARGUMENT
    sup = io.Supervision.from_synth(ws.supervision("trie_150x3"))
    assert sup.stats()["kernel"] == ws.RESIDENT
    assert lib.tc_debug_set(b"force_num_windowed", 1) == 0
    try:
        assert sup.stats()["kernel"] == ws.WINDOWED  # (the route is launch_num's, switch included)
    finally:
        assert lib.tc_debug_set(b"force_num_windowed", 0) == 0
    assert sup.stats()["kernel"] == ws.RESIDENT


def test_header_declares_and_documents_them():
    with open(os.path.join(ROOT, "include", "torchain_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint tc_supervision_stats\(const tc_supervision \*\w+, int64_t \*\w+\);", header)
    assert hasattr(lib, "tc_supervision_stats")
    assert '"force_num_windowed"' in header and '"num_windowed_launches"' in header
