"""The fused tied kernel's backward gamma frames take alpha'_t of the owned states from LDS, where a DMA requested a frame
earlier (from frame t+1's per-state pass; row T-1 from the backward prologue) has landed it, and keep it in registers as the
next frame's alpha'_{t+1} (den_tied_frames.h: TiedSeq::kHistByDma).  A row that lands late, in another lane's slot, one frame
off or not at all fails element-wise, since every derivative row depends on its history row.  The shapes are the smallest at
which that shows: T = 1 (the prologue's DMA only, and the request of no bytes at frame 0), T = 2 (the first DMA a frame
issues), T = 3 and 5; one graph per layout class that the constant selects (2-4 planes of states a thread, 1-3 planes of pdfs,
hub states) and the tight layout, which it excludes; the accumulating kernel with an l2 term; a ragged batch whose sequences
reach frame 0 at different frames.  Against the oracle with the bounds of tests/test_gpu_store_placement.py (REL = 1e-4 on
log-prob and derivative, every frame's gamma row summing to 1 within 1e-4).  Rows beyond 2^31 bytes: tests/test_gpu_far_rows.py."""
import numpy as np
import pytest
import torch

from torchain_amd import synth

import ragged_cases as rc
import row_contract_cases as rcc
from helpers import REL, rel_err
from test_gpu_store_placement import LAYOUTS, _check, den_ragged

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEAKY = rcc.LEAKY
FUSED = ("no_phase_split",)  # (_check adds no_tune)


@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_first_and_last_fetched_rows(oracle, kernel_family, T):
    _check(oracle, rcc.den_fst("tied8"), 3, T, kernel_family, FUSED)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_every_layout(oracle, kernel_family, layout):
    """pv2_tight re-reads the history in its per-state pass as before; every other one takes the DMA."""
    assert sorted(LAYOUTS) == ["hub_states", "jv2_pv1_roomy", "jv3", "jv4", "pv2_roomy", "pv2_tight", "pv3"]
    _check(oracle, LAYOUTS[layout](), 3, 4, kernel_family, FUSED)


def test_accumulate_with_l2(oracle, kernel_family):
    """ACCUM: the tail's load of the derivative row is issued behind the DMA and waited for at once"""
    _check(oracle, rcc.den_fst("tied8"), 3, 3, kernel_family, FUSED, accumulate=True, l2=0.01)


def test_ragged_batch(kernel_family):
    """Lengths 1, 2 and 5 in one batch (below 8 sequences: the fused RAGGED instantiation): each sequence's request of no
    bytes falls at a different frame of the batch."""
    lens = (1, 2, 5)
    graph = rcc.den_graph(rcc.BY_NAME["tied8_fused"], kernel_family)
    fst = rcc.den_fst("tied8")
    S, T = len(lens), max(lens)
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=78)
    from oracle import pyoracle
    pyoracle.build()
    want_lp, want_d = rc.den_reference(pyoracle.DenGraph(fst), lens, y, LEAKY, 1.0)
    yt = torch.from_numpy(rc.with_padding(y, lens, np.nan)).to(DEV)
    deriv = torch.full((S * T, fst.num_pdfs), 7.0, device=DEV)
    lp, st = den_ragged(graph, lens, yt, deriv, LEAKY, 1.0)
    got = deriv.cpu().numpy()
    assert st == 0
    assert abs(lp - want_lp) <= REL * abs(want_lp)
    assert rel_err(got, want_d) <= REL
    live = np.ones(S * T, bool)
    live[rc.padding_rows(lens)] = False
    assert np.abs(got[live].sum(axis=1, dtype=np.float64) - 1.0).max() <= 1e-4  # [K]: sum_pdf gamma_t = 1 in every frame
    assert not got[~live].view(np.int32).any()
