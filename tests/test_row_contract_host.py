"""The cases of tests/test_gpu_row_contract.py checked without a GPU (tests/row_contract_cases.py): every stride variant is in
the row-path state it is meant to exercise under api.cpp's rule, ``strided`` and ``outside`` account for every float of a
buffer, the graph with unused pdfs has some, every family's graph reports the kernel class the table expects, the picks cover
the classes they promise, and the float64 reference the GPU tests hold the kernels to is itself a set of posteriors."""
import numpy as np
import pytest
import torch

import row_contract_cases as rc


@pytest.mark.parametrize("P", [40, 100, 600, 4100])
def test_stride_variants_land_in_their_row_path_states(P):
    rows = 21
    seen = set()
    for name, ((ys, yo, ds, do), (want_y, want_d)) in rc.row_variants(P).items():
        _, y = rc.strided(rows, P, ys, yo, float("nan"))
        _, d = rc.strided(rows, P, ds, do, rc.SENTINEL)
        assert (rc.vector_path(y), rc.vector_path(d)) == (want_y, want_d), name
        seen.add((want_y, want_d))
    assert seen == {(True, True), (False, True), (True, False), (False, False)}
    seen = set()
    for name, (places, want) in rc.OBJECTIVE_PLACEMENTS.items():
        views = [rc.strided(rows, P, P + pad, off, 0.0)[1] for pad, off in places]
        assert tuple(rc.vector_path(v) for v in views) == want, name
        seen.add(want[1:])
    assert seen == {(True, True), (True, False), (False, True), (False, False)}  # (d_vec, x_vec)
    # each placement is one of the four variants' (stride, offset) pairs
    pairs = {(s - P, o) for (ys, yo, ds, do), _ in rc.row_variants(P).values() for s, o in ((ys, yo), (ds, do))}
    assert all(place in pairs for places, _ in rc.OBJECTIVE_PLACEMENTS.values() for place in places)


def test_vector_path_needs_all_three_conditions():
    assert rc.vector_path(rc.strided(5, 8, 8, 0, 0.0)[1])
    assert not rc.vector_path(rc.strided(5, 7, 8, 0, 0.0)[1])    # cols
    assert not rc.vector_path(rc.strided(5, 8, 10, 0, 0.0)[1])   # stride
    assert not rc.vector_path(rc.strided(5, 8, 8, 2, 0.0)[1])    # base address: 8 bytes off
    assert rc.vector_path(rc.strided(5, 8, 12, 4, 0.0)[1])       # 16 bytes off is aligned again


@pytest.mark.parametrize("rows,cols,stride,offset", [(4, 8, 8, 0), (4, 8, 11, 0), (21, 100, 104, 3), (1, 5, 9, 1)])
def test_strided_and_outside_account_for_every_float(rows, cols, stride, offset):
    buf, view = rc.strided(rows, cols, stride, offset, rc.SENTINEL)
    assert buf.numel() == offset + rows * stride + rc.SLACK and buf.dim() == 1 and buf.dtype == torch.float32
    assert view.shape == (rows, cols) and view.stride() == (stride, 1)
    assert view.data_ptr() - buf.data_ptr() == 4 * offset
    out = rc.outside(buf, view)
    assert out.numel() == buf.numel() - rows * cols
    bits = torch.tensor([rc.SENTINEL], dtype=torch.float32).view(torch.int32).item()
    assert bool((out == bits).all())
    view.fill_(1.0)                          # writing the view leaves the outside alone ...
    assert bool((rc.outside(buf, view) == bits).all())
    buf[offset + cols if stride > cols else buf.numel() - 1] = 1.0   # ... and one float of padding (or slack) is seen
    assert int((rc.outside(buf, view) != bits).sum()) == 1
    if offset:
        buf[offset - 1] = 2.0                # the float in front of the first row counts too
        assert int((rc.outside(buf, view) != bits).sum()) == 2
    nan_buf, nan_view = rc.strided(rows, cols, stride, offset, float("nan"))
    nan_view.fill_(0.0)
    assert int(torch.isnan(nan_buf).sum()) == nan_buf.numel() - rows * cols


def test_unused_pdf_graph_has_unused_columns():
    fst = rc.den_fst("unused")
    cols = rc.unused_pdfs(fst)
    assert len(cols) >= 100 and len(cols) + len(set(fst.ilabel.tolist())) == fst.num_pdfs
    assert not np.isin(cols + 1, fst.ilabel).any()
    for fam in rc.BAD_VALUE_FAMILIES:
        if fam.graph == "unused":
            assert all(c in cols for _, _, c in rc.bad_value_picks(fam) + rc.objective_picks(fam)), fam.name
    # every other graph of the table uses every column it could (2 * states >= pdfs) or is too small to: no accident
    assert len(rc.unused_pdfs(rc.den_fst("tied8"))) == 0


@pytest.mark.parametrize("family", rc.BAD_VALUE_FAMILIES, ids=lambda f: f.name)
def test_picks_cover_their_classes(family):
    S, T = family.S, family.T
    P = rc.den_fst(family.graph).num_pdfs
    M = T // 2
    picks = rc.bad_value_picks(family)
    assert 6 <= len(picks) <= 14 and len(set(picks)) == len(picks)
    assert all(0 <= t < T and 0 <= s < S and 0 <= c < P for t, s, c in picks)
    assert {t for t, _, _ in picks} >= {0, 1, M - 1, M, M + 1, T - 1}
    assert {s for _, s, _ in picks} == {0, S - 1}
    if family.graph != "unused":
        assert {0, P - 1} <= {c for _, _, c in picks}
        assert {c // 4096 for _, _, c in picks} == set(range((P + 4095) // 4096))   # every plane of 4096 pdfs
        if P % 4:
            assert P - P % 4 in {c for _, _, c in picks}   # the first column of the ragged last float4
    three = rc.objective_picks(family)
    assert [t for t, _, _ in three] == [0, M, T - 1]
    assert all(0 <= s < S and 0 <= c < P for _, s, c in three)
    if family in rc.FAMILIES:
        assert P % 4 == 0   # a 16-byte row path exists


def test_batches_of_the_streamed_families_pass_a_whole_slab():
    for fam in rc.BAD_VALUE_FAMILIES:
        if "slab_narrow" in fam.build:
            assert fam.S == 17 and fam.tied == 2
        elif "slab_wide" in fam.build:
            assert fam.S == 33 and fam.tied == 2
        else:
            assert (fam.S, fam.T) == (3, 7) and fam.tied in (0, 1)   # an odd batch, meeting frame 3


@pytest.mark.parametrize("family", rc.BAD_VALUE_FAMILIES, ids=lambda f: f.name)
def test_family_graphs_report_their_kernel_class(kernel_family, family):
    """What is known on the host: 0 general, 1 tied on chip, 2 streamed (the launch-time switches choose among the forms of one
    class and leave no trace here)."""
    graph = rc.den_graph(family, kernel_family)
    st = graph.stats()
    assert st["tied"] == family.tied, (family.name, st)
    if family.tied != 2:
        assert 0 < st["lds_bytes"] <= 160 * 1024 + 1024, st
    assert graph.n_pdf == rc.den_fst(family.graph).num_pdfs


@pytest.mark.parametrize("graph,batch", sorted({(f.graph, (f.S, f.T)) for f in rc.FAMILIES}))
def test_float64_reference_is_a_set_of_posteriors(graph, batch):
    S, T = batch
    lp, gam = rc.float64_reference(graph, S, T)
    assert np.isfinite(lp) and gam.shape == (S * T, rc.den_fst(graph).num_pdfs)
    assert gam.min() >= 0.0
    assert np.abs(gam.sum(axis=1) - 1.0).max() <= 1e-9
    assert np.all(gam[:, rc.unused_pdfs(rc.den_fst(graph))] == 0.0)


def test_carried_entries_of_the_supervisions():
    for fam in rc.OBJECTIVE_FAMILIES:
        sup = rc.supervision(fam.graph, fam.S, fam.T)
        mask = rc.carried(sup)
        assert mask.shape == (fam.S * fam.T, rc.den_fst(fam.graph).num_pdfs)
        per_row = mask.sum(axis=1)
        assert per_row.min() >= 1 and per_row.max() <= 2      # two paths per sequence: one or two pdfs per frame
        assert sup.weight == 0.5
