"""``tc_den_compose`` / ``io.DenominatorGraph.normalize_fsts`` and the constructors' ``den_graph`` argument, without a GPU:
the library against the plain-Python restatement of ``den_compose_reference`` (structure identical, costs within one float32
ulp), path weights by enumeration of every label sequence, trimming, empty products and limits, independence, determinism,
``den_graph=None`` and ``from_alignments``.  Cases: ``den_compose_cases``."""
import ctypes as C

import numpy as np
import pytest

from torchain_amd import io
from torchain_amd._lib import TorchainHipError, lib

import den_compose_cases as dc
import den_compose_reference as dr

GRAPHS = ("random", "phone_lm")


def _batch(name, e2e, seed, count=12):
    """(fsts, lengths) -- lengths only for regular ones."""
    rng = np.random.default_rng(seed)
    fst = dc.den_fst(name)
    if e2e:
        fsts = [dc.e2e_fst(fst, rng, n=int(rng.integers(1, 8)), junk=int(rng.integers(0, 5))) for _ in range(count - 2)]
        # ... and two whose only paths are twelve random labels: not in the graph
        fsts += [(0,) + dr.union_of_paths([[int(x) for x in rng.integers(1, dc.P + 1, size=12)]]) for _ in range(2)]
        return fsts, None
    pairs = [dc.regular_fst(fst, rng) for _ in range(count)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _same(got, want, what):
    """Structure identical, costs within one float32 ulp."""
    assert (got is None) == (want is None), what
    if got is None:
        return
    assert len(got) == len(want)
    if len(got) == 6:
        assert int(got[0]) == int(want[0]) == 0, what
        got, want = got[1:], want[1:]
    for k in (0, 1, 3):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(got[4], want[4]), what  # final costs are copied
    a, b = got[2].astype(np.float32), want[2].astype(np.float32)
    assert a.shape == b.shape
    assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all(), what


def _bytes(fst):
    return None if fst is None else b"|".join(np.ascontiguousarray(x).tobytes() for x in (fst if len(fst) == 5 else fst[1:]))


# ---- the same result as the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("e2e", [False, True])
@pytest.mark.parametrize("name", GRAPHS)
def test_same_result_as_the_restatement(name, e2e, scale):
    g = dc.graph(name)
    fsts, _ = _batch(name, e2e, seed=11 + e2e)
    got, info = g.normalize_fsts(fsts, e2e=e2e, scale=scale)
    want, status = dr.normalize(g, fsts, e2e=e2e, scale=scale)
    assert list(info["status"]) == status
    assert 0 in status and 1 in status, "the batch must hold both an accepted and a rejected supervision"
    for s, (a, b) in enumerate(zip(got, want)):
        _same(a, b, (name, e2e, scale, s))
        ab = fsts[s][1 if e2e else 0]
        assert (info["states_in"][s], info["arcs_in"][s]) == (len(ab) - 1, ab[-1])
        if a is not None:
            oab = a[1 if e2e else 0]
            assert (info["states_out"][s], info["arcs_out"][s]) == (len(oab) - 1, oab[-1])
        else:
            assert (info["states_out"][s], info["arcs_out"][s]) == (0, 0)
    if e2e:
        loops = [f is not None and (f[4] == np.repeat(np.arange(len(f[5])), np.diff(f[1]))).any() for f in got]
        assert any(loops), "no self-loop survived"


# ---- path weights by enumeration ------------------------------------------------------------------------------------------------
def _small():
    fst = dc.small_den_fst()
    g = io.DenominatorGraph(fst, 3)
    pi = g.initial_probs()
    assert pi[5] == 0 and (pi[:5] > 0).all()
    return fst, g


def _enumerate(g, sup, out, e2e, T, scale):
    norm = dr.NormFst(g)
    cmax = max(1.0, float(out[3 if e2e else 2].max())) if out is not None else 1.0
    tol = T * 2.0 ** -23 * cmax
    accepted = 0
    for labels in dr.label_sequences(3, T):
        a, b = dr.path_logsum(sup, labels, e2e), dr.norm_logsum(norm, labels, scale)
        got = -np.inf if out is None else dr.path_logsum(out, labels, e2e)
        if a == -np.inf or b == -np.inf:
            assert got == -np.inf, labels  # what either side rejects is rejected
        else:
            accepted += 1
            assert abs(got - (a + b)) <= tol, (labels, got, a + b, tol)
    return accepted


@pytest.mark.parametrize("scale", [1.0, 0.5, 0.0])
def test_path_weights_by_enumeration_regular(scale):
    fst, g = _small()
    T = 4
    rng = np.random.default_rng(5)
    table = rng.uniform(0, 3, size=(T, 4))
    # 2 1 x x reads the two arcs that share source and label; 3 3 x x is readable from state 5 alone (pi = 0)
    paths = [[1, 1, 2, 1], [1, 3, 2, 2], [2, 1, 3, 1], [3, 3, 1, 1], [3, 2, 2, 2], [1, 2, 3, 2], [2, 2, 1, 3], [1, 1, 1, 1]]
    sup = dr.union_of_paths(paths, final_costs=rng.uniform(0, 2, size=len(paths)), cost=lambda t, lab: table[t, lab])
    (out,), info = g.normalize_fsts([sup], scale=scale)
    assert out is not None and info["status"][0] == 0
    accepted = _enumerate(g, sup, out, False, T, scale)
    norm = dr.NormFst(g)
    assert 0 < accepted < len(paths)
    assert dr.norm_logsum(norm, [3, 3, 1, 1]) == -np.inf and dr.path_logsum(out, [3, 3, 1, 1]) == -np.inf


@pytest.mark.parametrize("scale", [1.0, 0.5, 0.0])
def test_path_weights_by_enumeration_end_to_end(scale):
    fst, g = _small()
    rng = np.random.default_rng(6)
    sups = [dc.e2e_fst(fst, rng, n=4, junk=3) for _ in range(3)]
    outs, _ = g.normalize_fsts(sups, e2e=True, scale=scale)
    assert any(o is not None for o in outs)
    total = 0
    for sup, out in zip(sups, outs):
        for T in range(1, 6):
            total += _enumerate(g, sup, out, True, T, scale)
    assert total > 20


# ---- trim and validity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e2e", [False, True])
@pytest.mark.parametrize("name", GRAPHS)
def test_outputs_are_trim_and_the_create_calls_accept_them(name, e2e):
    g = dc.graph(name)
    fsts, lens = _batch(name, e2e, seed=21 + e2e)
    outs, info = g.normalize_fsts(fsts, e2e=e2e)
    keep = [s for s, o in enumerate(outs) if o is not None]
    assert len(keep) >= 3
    for s in keep:
        assert dr.on_accepted_path(outs[s], e2e), s
    if e2e:
        h = io.Supervision.from_e2e_fsts(1.0, 12, dc.P, [outs[s] for s in keep])
        assert h.is_e2e and h.n_batch == len(keep)
    else:
        h = io.Supervision.from_fsts(1.0, [lens[s] for s in keep], dc.P, [outs[s] for s in keep])
        assert not h.is_e2e and list(h.frames) == [lens[s] for s in keep]
        assert h.stats()["kernel"] == "resident"


# ---- empty products and limits --------------------------------------------------------------------------------------------------
def _good_and_bad(name, rng):
    fst = dc.den_fst(name)
    good = [dc.regular_fst(fst, rng, T=6, in_graph=2, junk=1)[0] for _ in range(3)]
    bad = dr.union_of_paths([[int(x) for x in rng.integers(1, dc.P + 1, size=6)]])
    assert dr.normalize(dc.graph(name), [bad])[1] == [dr.EMPTY]
    return good, bad


def test_a_supervision_outside_the_graph_is_reported_and_its_neighbours_keep_their_bytes():
    g = dc.graph("random")
    good, bad = _good_and_bad("random", np.random.default_rng(3))
    alone, _ = g.normalize_fsts(good)
    outs, info = g.normalize_fsts([good[0], bad, good[1], bad, good[2]])
    assert list(info["status"]) == [0, 1, 0, 1, 0] and outs[1] is None and outs[3] is None
    assert [_bytes(outs[i]) for i in (0, 2, 4)] == [_bytes(a) for a in alone]
    with pytest.raises(ValueError, match=r"\[1, 3\]"):
        io.Supervision.from_fsts(1.0, [6] * 5, dc.P, [good[0], bad, good[1], bad, good[2]], den_graph=g)
    with pytest.raises(ValueError, match=r"\[2\]"):
        io.Supervision.from_e2e_fsts(1.0, 6, dc.P, [(0,) + good[0], (0,) + good[1], (0,) + bad], den_graph=g)
    h = io.Supervision.from_fsts(1.0, [6] * 3, dc.P, good, den_graph=g, normalization_scale=0.5)
    assert h.n_batch == 3 and h.is_ragged


def test_max_states_is_honoured():
    g = dc.graph("random")
    rng = np.random.default_rng(4)
    sup = dc.regular_fst(dc.den_fst("random"), rng, T=10, in_graph=3, junk=1)[0]
    norm = dr.NormFst(g)
    need = next(k for k in range(1, 2000) if dr.compose(norm, sup, max_states=k)[1] != dr.TOO_LARGE)
    assert need > 10
    for k in (1, need // 2, need - 1):
        (out,), info = g.normalize_fsts([sup], max_states=k)
        assert out is None and info["status"][0] == 2, k
    (out,), info = g.normalize_fsts([sup], max_states=need)
    assert out is not None and info["status"][0] == 0 and info["states_out"][0] <= need
    # beside a sequence within the limit
    small = dr.union_of_paths([dr.graph_path(dc.den_fst("random"), 2, rng)])
    outs, info = g.normalize_fsts([sup, small], max_states=need - 1)
    assert list(info["status"]) == [2, 0] and _bytes(outs[1]) == _bytes(g.normalize_fsts([small])[0][0])


def test_malformed_input_is_refused():
    g = dc.graph("random")
    rng = np.random.default_rng(8)
    ab, il, aw, nx, fin = dc.regular_fst(dc.den_fst("random"), rng, T=5, in_graph=2, junk=0)[0]

    def code(fst, e2e=False, **kw):
        with pytest.raises(TorchainHipError) as e:
            g.normalize_fsts([fst], e2e=e2e, **kw)
        return e.value.code

    bad_il, bad_nx, bad_aw, bad_fin = il.copy(), nx.copy(), aw.copy(), fin.copy()
    bad_il[1], bad_nx[2], bad_aw[0], bad_fin[0] = dc.P + 1, len(fin), np.nan, -np.inf
    assert code((ab, bad_il, aw, nx, fin)) == -2
    zero = il.copy()
    zero[0] = 0
    assert code((ab, zero, aw, nx, fin)) == -2
    assert code((ab, il, aw, bad_nx, fin)) == -2
    neg = nx.copy()
    neg[0] = -1
    assert code((ab, il, aw, neg, fin)) == -2
    assert code((ab, il, bad_aw, nx, fin)) == -2
    assert code((ab, il, aw, nx, bad_fin)) == -2
    assert code((len(fin), ab, il, aw, nx, fin), e2e=True) == -2
    assert code((-1, ab, il, aw, nx, fin), e2e=True) == -2
    for kw in (dict(scale=-1.0), dict(scale=np.inf), dict(scale=np.nan), dict(max_states=0)):
        with pytest.raises(ValueError):
            g.normalize_fsts([(ab, il, aw, nx, fin)], **kw)
    # decreasing offsets, straight at the C entry (the Python layer concatenates offsets itself)
    sb = np.array([0, len(fin)], np.int32)
    dec = ab.astype(np.int32).copy()
    dec[1], dec[2] = 3, 1
    res = C.c_void_p()
    args = lambda a, s=sb: (C.byref(res), g.ptr, 1, dc.P, 0, io._p(s), None, io._p(a), io._p(il), io._p(aw), io._p(nx), io._p(fin), 1.0, 200000)  # noqa: E731
    assert lib.tc_den_compose(*args(dec)) == -2 and not res
    assert lib.tc_den_compose(*args(ab.astype(np.int32), np.array([0, 0], np.int32))) == -2
    assert lib.tc_den_compose(*args(ab.astype(np.int32), np.array([1, len(fin)], np.int32))) == -2
    assert lib.tc_den_compose(C.byref(res), None, 1, dc.P, 0, io._p(sb), None, io._p(dec), None, None, None, io._p(fin), 1.0, 10) == -1


# ---- independence and determinism -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e2e", [False, True])
def test_sequences_are_independent_and_the_bytes_are_reproducible(e2e):
    g = dc.graph("phone_lm")
    before = int(lib.tc_den_graph_hash(g.ptr))
    fsts, _ = _batch("phone_lm", e2e, seed=31 + e2e, count=8)
    both, info = g.normalize_fsts(fsts, e2e=e2e)
    again, _ = g.normalize_fsts(fsts, e2e=e2e)
    assert [_bytes(f) for f in both] == [_bytes(f) for f in again]
    for s, f in enumerate(fsts):
        (one,), i1 = g.normalize_fsts([f], e2e=e2e)
        assert _bytes(one) == _bytes(both[s]) and i1["status"][0] == info["status"][s]
    assert int(lib.tc_den_graph_hash(g.ptr)) == before != 0


def test_threads_share_one_graph_handle():
    from concurrent.futures import ThreadPoolExecutor
    g = dc.graph("random")
    fsts, _ = _batch("random", False, seed=41, count=6)
    want = [_bytes(f) for f in g.normalize_fsts(fsts)[0]]
    with ThreadPoolExecutor(4) as pool:
        for got in pool.map(lambda _: [_bytes(f) for f in g.normalize_fsts(fsts)[0]], range(8)):
            assert got == want


# ---- den_graph=None ------------------------------------------------------------------------------------------------------------
def _spy(monkeypatch, name, sizes):
    """Records the arrays that reach ``lib.<name>`` (``sizes``: argument index -> bytes) and passes the call on."""
    seen = []
    real = getattr(lib, name)

    def call(*args):
        seen.append({i: C.string_at(args[i], n) for i, n in sizes.items()})
        return real(*args)

    monkeypatch.setattr(lib, name, call)
    return seen


def test_without_a_graph_the_arrays_reach_the_library_as_before(monkeypatch):
    rng = np.random.default_rng(9)
    pairs = [dc.regular_fst(dc.den_fst("random"), rng) for _ in range(3)]
    fsts, lens = [p[0] for p in pairs], [p[1] for p in pairs]
    ns, na = sum(len(f[4]) for f in fsts), sum(len(f[1]) for f in fsts)
    sb = np.concatenate([[0], np.cumsum([len(f[4]) for f in fsts])]).astype(np.int32)
    offs = np.concatenate([[0], np.cumsum([len(f[1]) for f in fsts])])
    ab = np.concatenate([[0]] + [f[0][1:] + offs[i] for i, f in enumerate(fsts)]).astype(np.int32)
    cat = lambda k, dt: np.concatenate([f[k] for f in fsts]).astype(dt).tobytes()  # noqa: E731
    want = [np.asarray(lens, np.int32).tobytes(), sb.tobytes(), ab.tobytes(), cat(1, np.int32), cat(2, np.float32),
            cat(3, np.int32), cat(4, np.float32)]
    # tc_supervision_create_ragged(out, weight, S, frames, label_dim, seq_begin, arc_begin, ilabel, weight, next, final)
    seen = _spy(monkeypatch, "tc_supervision_create_ragged",
                {3: 12, 5: 16, 6: 4 * (ns + 1), 7: 4 * na, 8: 4 * na, 9: 4 * na, 10: 4 * ns})
    io.Supervision.from_fsts(1.0, lens, dc.P, fsts)
    io.Supervision.from_fsts(1.0, lens, dc.P, fsts, den_graph=None, normalization_scale=0.25)
    assert len(seen) == 2
    for call in seen:
        assert [call[i] for i in (3, 5, 6, 7, 8, 9, 10)] == want
    # ... end-to-end: (out, weight, S, T, label_dim, seq_begin, start, arc_begin, ilabel, weight, next, final)
    seen = _spy(monkeypatch, "tc_supervision_create_e2e",
                {5: 16, 6: 12, 7: 4 * (ns + 1), 8: 4 * na, 9: 4 * na, 10: 4 * na, 11: 4 * ns})
    io.Supervision.from_e2e_fsts(1.0, 12, dc.P, [(0,) + f for f in fsts], den_graph=None)
    assert [seen[0][i] for i in (5, 6, 7, 8, 9, 10, 11)] == [want[1], np.zeros(3, np.int32).tobytes()] + want[2:]


# ---- from_alignments -----------------------------------------------------------------------------------------------------------
def test_from_alignments(monkeypatch):
    fst, g = _small()
    src, dst, pdf, prob = g.arcs()
    pi = g.initial_probs().astype(np.float64)
    M = np.zeros((3, 6, 6))
    np.add.at(M, (pdf, src, dst), prob.astype(np.float64))
    ali = np.array([[0, 0, 1, 0, -1], [1, 0, 2, 1, 0]], np.int32)  # (pdfs: labels 1 1 2 1 and 2 1 3 2 1)
    want = []
    for row in ali:
        v = pi.copy()
        for p in row[row >= 0]:
            v = v @ M[p]
        assert v.sum() > 0
        want.append(-np.log(v.sum()))  # -log sum over start states and parallel arcs of pi * prod w
    seen = _spy(monkeypatch, "tc_den_compose", {})
    h = io.Supervision.from_alignments(1.0, ali, 3, den_graph=g)
    assert len(seen) == 1 and (h.n_batch, h.n_frame, h.n_pdf) == (2, 5, 3) and list(h.frames) == [4, 5] and not h.is_e2e
    # the FSTs behind the handle: the linear acceptors, normalized
    linear = []
    for row in ali:
        n = int((row >= 0).sum())
        linear.append(dr.union_of_paths([[int(p) + 1 for p in row[:n]]]))
    outs, _ = g.normalize_fsts(linear)
    for row, out, w in zip(ali, outs, want):
        labels = [int(p) + 1 for p in row[row >= 0]]
        assert abs(-dr.path_logsum(out, labels) - w) <= len(labels) * 2.0 ** -23 * max(1.0, float(out[2].max()))
        others = [s for s in dr.label_sequences(3, len(labels)) if list(s) != labels]
        assert all(dr.path_logsum(out, s) == -np.inf for s in others)  # one label path
    # without a graph: the linear acceptors themselves, at cost 0
    seen = _spy(monkeypatch, "tc_supervision_create_ragged", {7: 4 * 9, 8: 4 * 9})
    h0 = io.Supervision.from_alignments(0.5, ali, 3, frames=[4, 5])
    assert h0.weight == 0.5 and seen[0][7] == np.array([1, 1, 2, 1, 2, 1, 3, 2, 1], np.int32).tobytes()
    assert seen[0][8] == np.zeros(9, np.float32).tobytes()
    # padding and bad input
    for bad, kw in ((np.array([[0, -1, 1, 0]]), {}), (np.array([[0, 1, 3, 0]]), {}), (np.array([[-1, -1, -1]]), {}),
                    (np.array([[0, 1, 2, -1]]), dict(frames=[4])), (np.array([[0, 1, 2, 1]]), dict(frames=[3])),
                    (np.array([[0, 1, 2, 1]]), dict(frames=[5])), (np.array([0, 1, 2]), {}), (np.array([[0.0, 1.0]]), {})):
        with pytest.raises(ValueError):
            io.Supervision.from_alignments(1.0, bad, 3, **kw)
    with pytest.raises(ValueError, match=r"\[1\]"):  # an alignment the graph does not contain (3 3 from the start: state 5, pi = 0)
        io.Supervision.from_alignments(1.0, np.array([[0, 0, 1], [2, 2, 0]]), 3, den_graph=g)
    with pytest.raises(ValueError, match=r"\[0\]"):  # best_path's -1s of a sequence without a path
        io.Supervision.from_alignments(1.0, np.array([[-1, -1, -1], [0, 0, 1]]), 3, frames=[3, 3], den_graph=g)


def test_from_sequences_takes_the_graph():
    from torchain_amd import synth
    fst = dc.den_fst("random")
    sups = [synth.random_supervision(fst, 1, T, 3, seed=50 + T) for T in (5, 8)]
    g = dc.graph("random")
    stripped = [dr.strip_weights(s) for s in sups]
    bare = [s._replace(arc_weight=f[2], final=f[4]) for s, f in zip(sups, stripped)]
    h = io.Supervision.from_sequences(bare, den_graph=g)
    assert list(h.frames) == [5, 8]
    outs, info = g.normalize_fsts(stripped)
    assert (info["status"] == 0).all() and (info["states_out"] >= info["states_in"] - 1).all()
    import torchain.io as shim  # the reference's module name re-exports the additions
    assert shim.Supervision is io.Supervision and shim.DenominatorGraph is io.DenominatorGraph
