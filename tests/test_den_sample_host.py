"""The path sampler of the denominator graph without a GPU: the reference of ``tests/den_sample_reference.py`` (what the GPU
tests compare with) against an enumeration of every latent path and against the float64 posteriors and sMBR gradient of
``tests/den_accuracy_reference.py``; ``functions.sampled_risk_surrogate`` (plain torch) against the estimator it states; the
export and binding of ``tc_den_sample_paths`` and the checks made before any device call."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from torchain_amd import io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import den_sample_paths, sampled_risk_surrogate

import den_accuracy_reference as dar
import den_sample_reference as dsr

TC_ERR_INVALID_ARGUMENT = -1
TC_ERR_WORKSPACE = -4


def _uniforms(seed, *shape):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


# ---- the reference against enumeration ----
@pytest.mark.parametrize("leaky", [0.0, 0.1])
@pytest.mark.parametrize("states,seed", [(4, 12), (5, 16), (6, 13)])
def test_reference_samples_follow_the_enumerated_posterior(states, seed, leaky):
    """The graphs' seeds are fixed, and were chosen on the CPU: the binomial sigma below is no measure for ONE occurrence of a
    sequence with K * p << 1 (its z is 1 / sqrt(K p): 8 sigma at p = 3e-6, an event of probability K p = 1 %, and a graph with
    a hundred such sequences shows one).  Of 24 graphs tried, 5 had such a draw at c = 0.1 and none any other excess."""
    fst = synth.random_den_fst(states, 3, 5, seed=seed)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    pi = graph.initial_probs()
    T, K, P = 3, 4096, fst.num_pdfs
    y = synth.random_nnet_output(1, T, P, seed=3)
    tab = dsr.tables(fst, pi)
    pdfs, states_, close, leaks = dsr.batch(tab, y, 1, leaky, _uniforms(5, 1, K, T + 1, 3))
    assert (pdfs >= 0).all() and (states_ >= 0).all()
    assert (leaks.sum() > 0) == (leaky > 0)
    assert all(dsr.valid_sample(tab, pdfs[0, k], states_[0, k], leaky) for k in range(0, K, 64))
    # every pdf sequence's frequency against its enumerated probability
    exact = dsr.enumerate_paths(tab, y, leaky)
    assert abs(sum(exact.values()) - 1.0) <= 1e-12
    seen, counts = np.unique(pdfs[0], axis=0, return_counts=True)
    count = {tuple(int(v) for v in row): int(n) for row, n in zip(seen, counts)}
    assert set(count) <= set(exact)
    worst = 0.0
    for key, prob in exact.items():
        sigma = np.sqrt(prob * (1.0 - prob) / K)
        worst = max(worst, abs(count.get(key, 0) / K - prob) / sigma)
    # ... and the per-frame pdf occupancies against the float64 posteriors
    gamma = dar.recursion(dar.arcs_of(fst, tab[3]), tab[4], y, np.zeros(T, np.int64), None, leaky)["gamma"]
    occ = np.zeros((T, P))
    for t in range(T):
        occ[t] = np.bincount(pdfs[0, :, t], minlength=P) / K
    sigma = np.sqrt(np.maximum(gamma * (1.0 - gamma), 1e-300) / K)
    z = np.abs(occ - gamma) / sigma
    z[(gamma == 0) & (occ == 0)] = 0.0  # (a pdf that no path emits in that frame, and none was seen)
    print("%d paths enumerated, %d seen; worst sequence %.2f sigma, worst occupancy %.2f sigma" % (len(exact), len(count), worst, z.max()))
    assert worst <= 5.0
    assert z.max() <= 5.0


# ---- the estimator ----
@functools.lru_cache(maxsize=None)
def _estimator_case():
    fst = synth.random_den_fst(300, 5, 100, seed=32)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    tab = dsr.tables(fst, graph.initial_probs())
    leaky = 0.1
    y, ref, exact = dsr.boosted_reference(fst, tab, 8, leaky, path_seed=9, y_seed=21)
    return fst, graph, tab, y, ref, leaky, exact


def test_centred_estimator_reproduces_the_exact_smbr_gradient():
    fst, graph, tab, y, ref, leaky, exact = _estimator_case()
    T, P, K = 8, fst.num_pdfs, 2048
    assert 0.3 <= exact["acc"] / T <= 0.7
    pdfs, _, _, leaks = dsr.batch(tab, y, 1, leaky, _uniforms(6, 1, K, T + 1, 3))
    assert (pdfs >= 0).all() and leaks.sum() > 0
    risks = (pdfs[0] == ref[None, :]).sum(axis=1).astype(np.float64)  # the frame accuracy of each path
    assert abs(risks.mean() - exact["acc"]) <= 5.0 * risks.std(ddof=1) / np.sqrt(K)
    terms = dsr.estimator_terms(pdfs[0], risks, T, P)
    for i, (got, want, se) in enumerate(dsr.projections(terms, exact["grad"])):
        print("direction %d: estimate %+.5f, exact %+.5f, z = %+.2f" % (i, got, want, (got - want) / se))
        assert abs(got - want) <= 5.0 * se
    # the surrogate's gradient is the mean of those terms
    x = torch.from_numpy(y).requires_grad_(True)
    value = sampled_risk_surrogate(x, torch.from_numpy(pdfs), torch.from_numpy(risks[None]))
    assert value.dtype == torch.float64 and value.shape == (1,)
    value.sum().backward()
    # (float32: an element is a recursive sum of at most K rounded terms, so (K + 2) * 2^-24 of the sum of their magnitudes)
    assert (np.abs(x.grad.numpy() - terms.mean(axis=0)) <= (K + 2) * 2.0 ** -24 * np.abs(terms).mean(axis=0)).all()


def test_surrogate_layouts_padding_clamp_and_failed_sequences():
    rng = np.random.default_rng(2)
    B, K, T, P = 3, 4, 5, 7
    y = rng.normal(size=(T * B, P)).astype(np.float32)
    y[0 * B + 0, 2], y[1 * B + 0, 3] = 31.0, -40.0  # outside the denominator's clamp
    frames = np.array([5, 3, 4])
    pdfs = rng.integers(0, P, size=(B, K, T)).astype(np.int32)
    pdfs[0, :, 0], pdfs[0, :, 1] = 2, 3
    for b in range(B):
        pdfs[b, :, frames[b]:] = -1
    pdfs[2] = -1  # a failed sequence
    risks = rng.normal(size=(B, K))
    want = np.zeros(B)
    grad = np.zeros((T * B, P))
    yc = np.clip(y.astype(np.float64), -30, 30)
    for b in range(2):
        wgt = (risks[b] - risks[b].mean()) / (K - 1)
        for k in range(K):
            for t in range(frames[b]):
                want[b] += wgt[k] * yc[t * B + b, pdfs[b, k, t]]
                if abs(y[t * B + b, pdfs[b, k, t]]) <= 30:
                    grad[t * B + b, pdfs[b, k, t]] += wgt[k]
    x2 = torch.from_numpy(y).requires_grad_(True)
    v2 = sampled_risk_surrogate(x2, torch.from_numpy(pdfs), torch.from_numpy(risks), frames=frames)
    v2.sum().backward()
    assert np.abs(v2.detach().numpy() - want).max() <= 1e-12 and v2[2] == 0
    assert np.abs(x2.grad.numpy() - grad).max() <= 1e-6
    g = x2.grad.numpy()
    assert g[0, 2] == 0 and g[B, 3] == 0 and not np.signbit(g[0, 2]) and not np.signbit(g[B, 3])
    pad = np.ones((T, B), bool)
    for b in range(2):
        pad[:frames[b], b] = False
    assert (g.reshape(T, B, P)[pad] == 0).all() and not np.signbit(g.reshape(T, B, P)[pad]).any()
    # (B, C, T), and without `frames` (the -1 marks alone)
    x3 = torch.from_numpy(np.ascontiguousarray(y.reshape(T, B, P).transpose(1, 2, 0))).requires_grad_(True)
    v3 = sampled_risk_surrogate(x3, torch.from_numpy(pdfs), torch.from_numpy(risks))
    v3.sum().backward()
    assert torch.equal(v3, v2)
    assert torch.equal(x3.grad.permute(2, 0, 1).reshape(T * B, P), x2.grad)
    for bad in (lambda: sampled_risk_surrogate(x2, torch.from_numpy(pdfs[:, :1]), torch.from_numpy(risks[:, :1])),
                lambda: sampled_risk_surrogate(x2, torch.from_numpy(pdfs), torch.from_numpy(risks[:, :2])),
                lambda: sampled_risk_surrogate(x2, torch.from_numpy(pdfs.astype(np.float32)), torch.from_numpy(risks)),
                lambda: sampled_risk_surrogate(x2[:-1], torch.from_numpy(pdfs), torch.from_numpy(risks)),
                lambda: sampled_risk_surrogate(x2, torch.from_numpy(pdfs + P), torch.from_numpy(risks)),
                lambda: sampled_risk_surrogate(x2, torch.from_numpy(pdfs), torch.from_numpy(risks), frames=[5, 3, 9])):
        with pytest.raises(ValueError):
            bad()


# ---- the library's and the wrappers' checks in front of any device call ----
def test_entry_is_exported_and_checks_its_arguments():
    fst = synth.random_den_fst(40, 4, 24)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    S, T, K, P, H = 3, 11, 4, fst.num_pdfs, fst.num_states
    need = int(lib.tc_den_sample_paths_workspace_bytes(graph.ptr, S, T))
    per = ((T + 1) * ((H + 3) // 4 * 4) + (T + 1 + 3) // 4 * 4) * 4
    assert need == (S * per + 255) // 256 * 256
    assert int(lib.tc_den_sample_paths_workspace_bytes(None, S, T)) == TC_ERR_INVALID_ARGUMENT
    assert int(lib.tc_den_sample_paths_workspace_bytes(graph.ptr, 0, T)) == TC_ERR_INVALID_ARGUMENT
    assert int(lib.tc_den_sample_paths_workspace_bytes(graph.ptr, S, 0)) == TC_ERR_INVALID_ARGUMENT
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails before a device call
    keys = (b"den_sample_launches", b"den_sample_streamed_launches", b"den_launches")
    before = [int(lib.tc_debug_counter(key)) for key in keys]
    assert min(before) >= 0

    def call(g=graph.ptr, s=S, y=fake, rows=S * T, cols=P, stride=P, fr=None, t=T, leaky=1e-5, k=K, u=fake, pdf=fake, st=None,
             ws=fake, nbytes=need):
        return lib.tc_den_sample_paths(g, s, y, rows, cols, stride, fr, t, leaky, k, u, pdf, st, ws, nbytes, 0, None)

    for kwargs in (dict(g=None), dict(y=None), dict(u=None), dict(pdf=None), dict(s=0), dict(t=0), dict(k=0), dict(k=-1),
                   dict(rows=S * T + 1), dict(cols=P + 1), dict(cols=P - 1), dict(stride=P - 1), dict(leaky=-0.5),
                   dict(leaky=float("inf")), dict(leaky=float("nan")), dict(y=C.c_void_p(4098)), dict(fr=C.c_void_p(4098)),
                   dict(u=C.c_void_p(4097)), dict(pdf=C.c_void_p(4098)), dict(st=C.c_void_p(4099))):
        assert call(**kwargs) == TC_ERR_INVALID_ARGUMENT, kwargs
    assert call(ws=None) == TC_ERR_WORKSPACE
    assert call(ws=C.c_void_p(4100)) == TC_ERR_WORKSPACE
    assert call(nbytes=need - 1) == TC_ERR_WORKSPACE
    assert [int(lib.tc_debug_counter(key)) for key in keys] == before  # nothing was launched
    assert lib.tc_debug_set(b"force_den_sample_streamed", 0) == 0


def test_wrappers_check_before_any_library_call():
    fst = synth.random_den_fst(40, 4, 24)
    graph = io.DenominatorGraph(fst, fst.num_pdfs)
    x = torch.zeros(3 * 11, fst.num_pdfs)
    with pytest.raises(ValueError, match="CUDA tensor"):
        graph.sample_paths(x, 4, n_batch=3)
    with pytest.raises(TypeError, match="io.DenominatorGraph"):
        den_sample_paths(x, fst, 4, n_batch=3)
    import torchain.functions
    import torchain.io
    assert torchain.functions.den_sample_paths is den_sample_paths
    assert torchain.functions.sampled_risk_surrogate is sampled_risk_surrogate
    assert torchain.io.DenominatorGraph.sample_paths is io.DenominatorGraph.sample_paths
