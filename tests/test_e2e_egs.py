"""End-to-end chain egs (``<End2End>`` true): the native reader (csrc/egs_reader.cpp) and the numpy statement
(torchain_amd/egs.py) read what tests/e2e_egs_writer.py writes to the same per-sequence FSTs, merging concatenates the FST
lists, a minibatch mixing e2e and regular egs is refused, and the handles built from them are e2e."""
import numpy as np
import pytest

from torchain_amd import egs, io, synth

import e2e_egs_writer as ew
import e2e_reference as ref
import kaldi_egs_writer as kw

P, F = 40, 6


def _fsts(n, seed, T):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        f = ref.chain_fst(P, rng, words=2, max_phones=2, start_state=1 + i % 3)  # (start state != 0)
        assert f[0] != 0 and ref.shortest_path_arcs(f) <= T
        out.append(f)
    return out


def _same_fst(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("matrix_kind", ["FM", "CM"])
@pytest.mark.parametrize("alignment_pdfs", [False, True])
def test_native_and_numpy_readers_agree(tmp_path, matrix_kind, alignment_pdfs):
    T = 12
    fsts = _fsts(3, 1, T)
    keyed = [("utt%d" % i, ew.example(f, T, P, F, seed=i)) for i, f in enumerate(fsts)]
    ark, scp = str(tmp_path / "e2e.ark"), str(tmp_path / "e2e.scp")
    ew.write_ark(ark, keyed, scp_path=scp, matrix_kind=matrix_kind, alignment_pdfs=alignment_pdfs)
    py = list(egs.iter_archive(ark))
    nat = list(egs.iter_archive_native(ark))
    assert [k for k, _ in py] == [k for k, _ in nat] == [k for k, _ in keyed]
    for (_, a), (_, b), f in zip(py, nat, fsts):
        for e in (a, b):
            sup = e["outputs"][0]["supervision"]
            assert isinstance(sup, egs.E2eSup)
            assert (sup.num_sequences, sup.frames_per_sequence, sup.label_dim) == (1, T, P)
            _same_fst(sup.fsts[0], f)
        np.testing.assert_array_equal(a["inputs"][0]["features"], b["inputs"][0]["features"])


def test_merge_concatenates_fst_lists(tmp_path):
    T = 10
    fsts = _fsts(4, 2, T)
    keyed = [("utt%d" % i, ew.example(f, T, P, F, seed=i, weight=0.5)) for i, f in enumerate(fsts)]
    ark, scp = str(tmp_path / "e2e.ark"), str(tmp_path / "e2e.scp")
    ew.write_ark(ark, keyed, scp_path=scp)
    entries = [(p, int(o)) for p, o in (line.split()[1].rsplit(":", 1) for line in open(scp))]
    nat = egs.read_merged_native(entries)
    py = egs.merge_chain_examples([egs.read_scp_entry(p, o) for p, o in entries])
    for m in (nat, py):
        sup = m["outputs"][0]["supervision"]
        assert isinstance(sup, egs.E2eSup)
        assert (sup.num_sequences, sup.frames_per_sequence, sup.label_dim, sup.weight) == (4, T, P, 0.5)
        for got, want in zip(sup.fsts, fsts):
            _same_fst(got, want)
    np.testing.assert_array_equal(nat["outputs"][0]["indexes"], py["outputs"][0]["indexes"])
    h = io.Supervision.from_synth(nat["outputs"][0]["supervision"])
    assert h.is_e2e and h.shape == (4, T, P)


def test_mixed_e2e_and_regular_merge_is_refused(tmp_path):
    T = 8
    fst = synth.random_den_fst(30, 3, P, seed=3)
    reg = synth.random_supervision(fst, 1, T, 2, seed=4)
    reg_eg = ew.example(_fsts(1, 5, T)[0], T, P, F, seed=1)
    reg_eg["outputs"][0]["supervision"] = reg
    e2e_eg = ew.example(_fsts(1, 6, T)[0], T, P, F, seed=2)
    a1, a2 = str(tmp_path / "reg.ark"), str(tmp_path / "e2e.ark")
    kw.write_ark(a1, [("r", reg_eg)], scp_path=a1 + ".scp")
    ew.write_ark(a2, [("e", e2e_eg)], scp_path=a2 + ".scp")
    entries = [(p, int(o)) for s in (a1, a2) for p, o in (line.split()[1].rsplit(":", 1) for line in open(s + ".scp"))]
    with pytest.raises(egs.EgsFormatError):
        egs.read_merged_native(entries)
    with pytest.raises(egs.EgsFormatError):
        egs.merge_chain_examples([egs.read_scp_entry(p, o) for p, o in entries])


def test_example_and_rand_example_yield_e2e_supervisions(tmp_path):
    T = 10
    fsts = _fsts(6, 7, T)
    keyed = [("utt%d" % i, ew.example(f, T, P, F, seed=i)) for i, f in enumerate(fsts)]
    ark, scp = str(tmp_path / "e2e.ark"), str(tmp_path / "e2e.scp")
    ew.write_ark(ark, keyed, scp_path=scp, len_path=scp + ".len")
    n = 0
    for (inp, _aux), sup in io.Example("ark:" + ark):
        assert sup.is_e2e and sup.shape == (1, T, P)
        n += 1
    assert n == len(fsts)
    seen = 0
    for (inp, _aux), sup in io.RandExample(scp, 0, 3):
        assert sup.is_e2e and sup.shape[1:] == (T, P)
        seen += sup.shape[0]
    assert seen == len(fsts)


def test_start_state_out_of_range_is_a_format_error(tmp_path):
    T = 8
    f = list(_fsts(1, 8, T)[0])
    f[0] = len(f[5])  # start = number of states
    ark = str(tmp_path / "bad.ark")
    ew.write_ark(ark, [("bad", ew.example(tuple(f), T, P, F, seed=1))])
    with pytest.raises(egs.EgsFormatError):
        list(egs.iter_archive(ark))
    with pytest.raises(egs.EgsFormatError):
        list(egs.iter_archive_native(ark))


def test_from_e2e_fsts_checks_each_sequence_arc_count():
    fsts = _fsts(2, 9, 10)
    a = list(fsts[0])
    b = list(fsts[1])
    # one extra arc in the first sequence's arrays, one missing in the second: equal totals, shifted sequences
    a[2], a[3], a[4] = np.append(a[2], 1), np.append(a[3], 0.0), np.append(a[4], 0)
    b[2], b[3], b[4] = b[2][:-1], b[3][:-1], b[4][:-1]
    with pytest.raises(ValueError):
        io.Supervision.from_e2e_fsts(1.0, 10, P, [tuple(a), tuple(b)])
