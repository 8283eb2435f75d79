"""Host side of the wide-level numerator (no GPU): ``any_width=True`` and what ``stats()`` / ``wide_stats()`` report."""
import pytest

from torchain_amd import io
from torchain_amd._lib import lib

import wide_supervisions as ws

TC_ERR_INVALID_ARGUMENT, TC_ERR_UNSUPPORTED = -1, -3


def _one_wide_level(width=12000):
    return ws.lattice_supervision(1, 3, ws.P, lambda q, t, r: width if t == 2 else 4, 1, seed=1)


def test_a_12000_state_level_is_wide_only_when_allowed():
    sup = _one_wide_level()
    plain, wide = io.Supervision.from_synth(sup), io.Supervision.from_synth(sup, any_width=True)
    assert [(h.stats()["route"], h.stats()["kernel"]) for h in (plain, wide)] == [(TC_ERR_UNSUPPORTED, "unsupported"), (2, "wide")]
    assert all(plain.stats()[k] == v for k, v in wide.stats().items() if k not in ("route", "kernel"))
    assert plain.wide_stats() == dict(wide.wide_stats(), any_width=False, form=None)
    lds = 8 * 12000 + 4 * ((wide.stats()["max_frame_uniq"] + 3) & ~3)
    assert wide.wide_stats() == dict(any_width=True, form="lds", lds_bytes=lds, scratch_bytes=wide.wide_stats()["scratch_bytes"])
    assert wide.wide_stats()["scratch_bytes"] >= 16 * 12000 + 4 * wide.stats()["max_level_arcs"] + 4 * wide.stats()["max_frame_uniq"]
    assert io.Supervision.from_synth(_one_wide_level(21000), any_width=True).wide_stats()["form"] == "slot"


@pytest.mark.parametrize("name", ["trie_150x3", "lattice_bursty", "trie_150x64", "lattice_wide"])
def test_an_allowed_handle_that_fits_keeps_its_kernel(name):
    h = io.Supervision.from_synth(ws.supervision(name), any_width=True)
    assert h.stats() == io.Supervision.from_synth(ws.supervision(name)).stats()
    assert h.stats()["kernel"] == ws.expected_kernel(name) and h.wide_stats()["any_width"] and h.wide_stats()["form"] is None


def test_switches_and_counter_exist():
    assert lib.tc_debug_counter(b"num_wide_launches") >= 0 and lib.tc_debug_counter(b"num_wide_launchez") == -1
    assert lib.tc_debug_set(b"force_num_wide_", 1) == lib.tc_debug_set(b"force_num_wide_streamed_", 1) == TC_ERR_INVALID_ARGUMENT
    plain, wide = (io.Supervision.from_synth(ws.supervision("trie_150x3"), any_width=w) for w in (False, True))
    assert lib.tc_debug_set(b"force_num_wide", 1) == 0
    try:
        assert plain.stats()["kernel"] == ws.RESIDENT and wide.stats()["kernel"] == "wide" and wide.wide_stats()["form"] == "lds"
        assert lib.tc_debug_set(b"force_num_wide_streamed", 1) == 0
        assert wide.wide_stats()["form"] == "slot"
    finally:
        assert lib.tc_debug_set(b"force_num_wide", 0) == lib.tc_debug_set(b"force_num_wide_streamed", 0) == 0
    assert wide.stats()["kernel"] == ws.RESIDENT
    assert lib.tc_supervision_allow_wide_levels(None, 1) == TC_ERR_INVALID_ARGUMENT
