"""Where the tied frames (den_tied_frames.h) issue their global stores: the alpha' history row of frame t-1 from frame t's
per-state pass (the fused kernel) or from under its arc walk (the two-workgroup roles), the derivative row of frame t+1 (and
the cross-entropy output's zero row with it) and role B's B-history row from under frame t's walk; the first and the last row
of a phase from the phase's prologue and epilogue.  A row stored late, twice, to the wrong frame or not at all fails element-wise: every
frame's derivative row depends on its history row.  The shapes are the smallest at which that shows -- T = 1 (no row between
row 0 and row T), T = 2 (the first frame that stores), T = 3 (a store before and after a stored row), the meeting frames
M = 1 and 3 of the two-workgroup form, one graph per layout class of the dispatcher -- against the oracle with the bounds of
tests/test_gpu_tied.py for the same kernels (REL = 1e-4; log-prob relative, derivative matrix-wise)."""
import ctypes as C

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd.functions import ChainResults, compute_chain_objf_and_deriv

import ragged_cases as rc
import row_contract_cases as rcc
from helpers import REL, hip_den, hip_den_on, rel_err
from torchain_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEAKY = rcc.LEAKY

# name -> graph of one layout class (TiedSeq<JV, PV, ALPHA_LDS>): states per thread 8 / 12 / 16, planes of pdfs 1 / 2 / 3,
# the roomy and the tight LDS layout (the tight one: tests/test_gpu_tied.py::test_tied_tight_layout_mid_vocab's graph),
# hub states whose secondary rows are folded between the walk and the per-state pass
LAYOUTS = {
    "jv2_pv1_roomy": lambda: rcc.den_fst("tied8"),
    "jv3": lambda: rcc.den_fst("tied12"),
    "jv4": lambda: rcc.den_fst("tied16"),
    "pv2_roomy": lambda: rcc.den_fst("pdfs2"),
    "pv3": lambda: rcc.den_fst("pdfs3"),
    "pv2_tight": lambda: synth.random_den_fst(8192, 3, 6000, seed=41),
    "hub_states": lambda: synth.skewed_tied_den_fst(400, 7000, 150, seed=8),
}


def den_ragged(graph, lens, yt, deriv, leaky, deriv_weight):
    """tc_den_forward_backward_ragged on device tensors where they lie; returns (log-prob, status)."""
    rows, cols = yt.shape
    n, tmax = len(lens), max(lens)
    graph.prepare(yt.device)
    frames = torch.tensor(list(lens), dtype=torch.int32, device=yt.device)
    nbytes = lib.tc_chain_workspace_bytes(graph.ptr, n, tmax)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=yt.device)
    lp = torch.full((1,), -123.0, dtype=torch.float64, device=yt.device)
    st = torch.full((1,), -1, dtype=torch.int32, device=yt.device)
    rcode = lib.tc_den_forward_backward_ragged(
        graph.ptr, n, C.c_void_p(yt.data_ptr()), rows, cols, yt.stride(0), leaky, deriv_weight, 0.0, 0,
        C.c_void_p(deriv.data_ptr()), deriv.stride(0), C.c_void_p(frames.data_ptr()), tmax, C.c_void_p(lp.data_ptr()),
        C.c_void_p(st.data_ptr()), C.c_void_p(ws.data_ptr()), nbytes, torch.cuda.current_device(),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rcode == 0, rcode
    return float(lp.item()), int(st.item())


def _check(oracle, fst, S, T, force, switches, seed=3, accumulate=False, l2=0.0):
    force("no_tune")
    for key in switches:
        force(key)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    assert graph.stats()["tied"] == 1
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=seed)
    ref = oracle.den_forward_backward(oracle.DenGraph(fst), y, S, leaky=LEAKY, deriv_weight=1.0)
    assert ref["ok"]
    init = 0.25 if accumulate else None
    out = hip_den(fst, y, S, leaky=LEAKY, deriv_weight=1.0, l2_scale=l2, accumulate=accumulate, init=init, graph=graph)
    want = ref["deriv"] - l2 * y + (0.25 if accumulate else 0.0)
    err_lp, err_d = abs(out["logprob"] - ref["logprob"]) / abs(ref["logprob"]), rel_err(out["deriv"], want)
    print("S=%d T=%d %s: log-prob rel %.2e, derivative rel %.2e" % (S, T, "+".join(switches), err_lp, err_d))
    assert out["status"] == 0
    assert err_lp <= REL
    assert err_d <= REL
    rows = (out["deriv"] - (want - ref["deriv"])).sum(axis=1, dtype=np.float64)
    assert np.abs(rows - 1.0).max() <= 1e-4  # [K]: sum_pdf gamma_t = 1 in every frame
    return out


@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_fused_kernel_first_frames(oracle, kernel_family, T):
    """The fused kernel forced onto a batch of three: no stored row between row 0 and row T, the first frame that stores, a
    store on both sides of a stored row, and a few more."""
    _check(oracle, rcc.den_fst("tied8"), 3, T, kernel_family, ("no_phase_split",))


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_fused_kernel_every_layout(oracle, kernel_family, layout):
    _check(oracle, LAYOUTS[layout](), 2, 4, kernel_family, ("no_phase_split",), l2=1e-3)


@pytest.mark.parametrize("layout", ["jv2_pv1_roomy", "pv2_tight", "jv4"])
@pytest.mark.parametrize("T", [2, 3, 7])
def test_meet_in_the_middle(oracle, kernel_family, T, layout):
    """Meeting frames 1, 1 and 3: role B's B-history rows and role F's gamma frames on either side of it."""
    _check(oracle, LAYOUTS[layout](), 2, T, kernel_family, ("force_mitm",))


@pytest.mark.parametrize("form", ["fused", "two_workgroups"])
def test_ragged_batch(form, kernel_family):
    """The RAGGED instantiations: lengths 1, 2 and 5 in one batch on the fused kernel; the same lengths among the eight
    sequences that the two-workgroup form takes."""
    lens = (1, 2, 5) if form == "fused" else (1, 2, 5, 3, 7, 2, 5, 1)
    fam = rcc.BY_NAME["tied8_fused" if form == "fused" else "tied8_two_cu"]
    graph = rcc.den_graph(fam, kernel_family)
    fst = rcc.den_fst("tied8")
    S, T = len(lens), max(lens)
    y = synth.random_nnet_output(S, T, fst.num_pdfs, seed=77)
    from oracle import pyoracle
    pyoracle.build()
    want_lp, want_d = rc.den_reference(pyoracle.DenGraph(fst), lens, y, LEAKY, -0.8)
    yt = torch.from_numpy(rc.with_padding(y, lens, np.nan)).to(DEV)
    deriv = torch.full((S * T, fst.num_pdfs), 7.0, device=DEV)
    lp, st = den_ragged(graph, lens, yt, deriv, LEAKY, -0.8)
    got = deriv.cpu().numpy()
    assert st == 0
    assert abs(lp - want_lp) <= REL * abs(want_lp)
    assert rel_err(got, want_d, floor=0.8) <= REL  # (tests/test_gpu_ragged.py: the floor is the derivative weight)
    assert not got[rc.padding_rows(lens)].view(np.int32).any()


@pytest.mark.parametrize("form", ["no_phase_split", "force_mitm"])
def test_accumulate(oracle, kernel_family, form):
    """ACCUM: the row's store follows the load of the same row"""
    _check(oracle, rcc.den_fst("tied8"), 3, 3, kernel_family, (form,), accumulate=True, l2=1e-3)


@pytest.mark.parametrize("form", ["no_phase_split", "force_mitm"])
@pytest.mark.parametrize("variant", ["odd_bases_both_scalar", "y_vector_d_scalar"])
def test_unaligned_rows(oracle, kernel_family, form, variant):
    """y_vec / d_vec = 0: the four-dword form of the row's store, in its new place"""
    fam = rcc.BY_NAME["tied8_fused" if form == "no_phase_split" else "tied8_mitm"]
    graph = rcc.den_graph(fam, kernel_family)
    fst = rcc.den_fst("tied8")
    S, T, P = 3, 3, fst.num_pdfs
    (ys, yo, ds, do), (y_vec, d_vec) = rcc.row_variants(P)[variant]
    y = synth.random_nnet_output(S, T, P, seed=12)
    ybuf, yt = rcc.strided(S * T, P, ys, yo, 0.0, device=DEV)
    yt.copy_(torch.from_numpy(y))
    dbuf, dview = rcc.strided(S * T, P, ds, do, rcc.SENTINEL, device=DEV)
    assert rcc.vector_path(yt) == y_vec and rcc.vector_path(dview) == d_vec
    out = hip_den_on(graph, S, yt, dview, leaky=LEAKY, deriv_weight=1.0)
    ref = oracle.den_forward_backward(oracle.DenGraph(fst), y, S, leaky=LEAKY, deriv_weight=1.0)
    assert out["status"] == 0 and ref["ok"]
    assert abs(out["logprob"] - ref["logprob"]) <= REL * abs(ref["logprob"])
    assert rel_err(dview.cpu().numpy(), ref["deriv"]) <= REL
    assert np.all(rcc.outside(dbuf, dview).cpu().numpy() == np.float32(rcc.SENTINEL).view(np.int32))


def test_xent_zero_rows(oracle, kernel_family):
    """The cross-entropy output's rows go out with the derivative's: over a matrix of 0xFF bytes (NaN) every element that no
    numerator arc carries is +0 afterwards and every other one is its posterior -- each row was written, once, with zeros,
    before the numerator added to it."""
    fam = rcc.BY_NAME["tied8_fused"]
    graph = rcc.den_graph(fam, kernel_family)
    fst = rcc.den_fst("tied8")
    S, T, P = 3, 3, fst.num_pdfs
    sup = rcc.supervision("tied8", S, T)
    y = synth.random_nnet_output(S, T, P, seed=13)
    ref = oracle.compute_chain_objf_and_deriv(oracle.DenGraph(fst), sup, y, 0.0, LEAKY, want_xent=True)
    yt = torch.from_numpy(y).to(DEV)
    deriv = torch.full((S * T, P), 7.0, device=DEV)
    xd = torch.full((S * T * P * 4,), 255, dtype=torch.uint8, device=DEV).view(torch.float32).view(S * T, P)
    assert torch.isnan(xd).all()
    res = ChainResults()
    compute_chain_objf_and_deriv(graph, io.Supervision.from_synth(sup), yt, res.data, deriv, xd, 0.0, LEAKY, 0.1)
    torch.cuda.synchronize()
    got = xd.cpu().numpy()
    carried = rcc.carried(sup)
    assert carried.any(axis=1).all() and not carried.all()
    assert not got[~carried].view(np.int32).any()
    assert np.isfinite(got).all()
    assert rel_err(got, ref["xent_deriv"], floor=0.5) <= REL
    assert rel_err(deriv.cpu().numpy(), ref["deriv"], floor=0.5) <= REL
