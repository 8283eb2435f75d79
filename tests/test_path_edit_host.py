"""``tests/path_edit_reference.py`` -- the token rule, the textbook Levenshtein distance and the rounding of the fused
gradient -- on cases worked by hand, and what ``tc_paths_edit_distance`` / ``tc_sampled_risk_grad`` and their Python
wrappers refuse before any device call.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from torchain_amd._lib import TC_DTYPE_F32, lib
from torchain_amd.functions import path_edit_distance, path_tokens, sampled_risk_surrogate

import path_edit_reference as per

TC_ERR_INVALID_ARGUMENT = -1
TC_ERR_UNSUPPORTED = -3
TC_ERR_WORKSPACE = -4

# pdfs 0, 1: phone a (10) forward / self-loop; 2, 3: phone b (11); 4: silence
TOKEN_OF_PDF = [10, 10, 11, 11, -1]
STARTS = [1, 0, 1, 0, 0]
A, A_, B, B_, SIL = 0, 1, 2, 3, 4


# ---- the token rule ----
def test_collapse_mode_compares_with_the_frame_before():
    assert per.tokens_of([A, SIL, A], TOKEN_OF_PDF) == [10, 10]  # silence in between: two tokens
    assert per.tokens_of([A, A_, A, A_], TOKEN_OF_PDF) == [10]  # `a a` collapses
    assert per.tokens_of([SIL, A, A_, B, B_, B_, SIL, SIL, B], TOKEN_OF_PDF) == [10, 11, 11]
    assert per.tokens_of([A, B, A], TOKEN_OF_PDF) == [10, 11, 10]


def test_start_mode_keeps_repeats_apart():
    assert per.tokens_of([A, A_, A, A_], TOKEN_OF_PDF, STARTS) == [10, 10]
    assert per.tokens_of([A_, A_, SIL, B], TOKEN_OF_PDF, STARTS) == [11]  # a self-loop pdf alone emits nothing
    assert per.tokens_of([A, SIL, A], TOKEN_OF_PDF, STARTS) == [10, 10]
    silent_start = [1, 0, 1, 0, 1]  # a start flag on a pdf without a token emits nothing
    assert per.tokens_of([SIL, A, SIL], TOKEN_OF_PDF, silent_start) == [10]


def test_empty_silent_and_failed_paths():
    assert per.tokens_of([], TOKEN_OF_PDF) == []
    assert per.tokens_of([SIL, SIL, SIL], TOKEN_OF_PDF) == []
    assert per.tokens_of([SIL, SIL, SIL], TOKEN_OF_PDF, STARTS) == []
    assert per.tokens_of([A, -1, B], TOKEN_OF_PDF) is None
    assert per.tokens_of([A, 5, B], TOKEN_OF_PDF, STARTS) is None
    dist, lens, tokens = per.batch(np.array([[[A, SIL, A], [-1, -1, -1]], [[SIL, SIL, SIL], [B, 7, B]]]), TOKEN_OF_PDF,
                                   [[10, 11], [10, 0]], [2, 1])
    assert dist.tolist() == [[1, -1], [1, -1]] and lens.tolist() == [[2, -1], [0, -1]]
    assert tokens.tolist() == [[[10, 10, -1], [-1, -1, -1]], [[-1, -1, -1], [-1, -1, -1]]]
    # padding frames are not read
    dist, lens, tokens = per.batch(np.array([[[A, B, 99, -5]]]), TOKEN_OF_PDF, [[10, 11]], [2], frames=[2])
    assert dist.tolist() == [[0]] and lens.tolist() == [[2]] and tokens.tolist() == [[[10, 11, -1, -1]]]


# ---- the distance ----
def _codes(word):
    return [ord(c) for c in word]


@pytest.mark.parametrize("a, b, want", [
    ("kitten", "sitting", 3), ("saturday", "sunday", 3), ("flaw", "lawn", 2), ("intention", "execution", 5),
    ("", "", 0), ("", "abc", 3), ("abc", "", 3), ("abc", "abc", 0), ("abc", "acb", 2), ("a", "b", 1), ("ab", "ba", 2),
    ("abcdef", "azced", 3),
])
def test_known_distances(a, b, want):
    assert per.levenshtein(_codes(a), _codes(b)) == want


def test_distance_properties():
    rng = np.random.default_rng(3)
    for _ in range(200):
        n, m = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        h = rng.integers(0, 3, n).tolist()
        r = rng.integers(0, 3, m).tolist()
        d = per.levenshtein(h, r)
        assert per.levenshtein(h, h) == 0
        assert abs(n - m) <= d <= max(n, m)
        assert d == per.levenshtein(r, h)


# ---- the rounding of the fused gradient ----
def test_bfloat16_rounding_is_one_rounding_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 0.0, -0.0,
                  2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 3.3e38, 3.4e38, -3.4e38, 1e-50])
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -1.0, 0.0, -0.0, 2.0 ** -133, 0.0, 2.0 ** -132,
                     float(np.float32(3.2963e38)), np.inf, -np.inf, 0.0], np.float32)
    got = per.round_bfloat16(x)
    assert got.dtype == np.float32
    # 3.3e38 lies between the two largest bfloat16 values; the expected one is checked through torch's own cast
    want[10] = torch.tensor(3.3e38, dtype=torch.float64).to(torch.bfloat16).float().item()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # where one rounding and two differ: z lies just below a tie; float32 rounds it onto the tie, which then goes up to the
    # even neighbour 1 + 2^-6
    z = 1.0 + 3 * 2.0 ** -8 - 2.0 ** -40
    assert per.round_bfloat16([z])[0] == np.float32(1.0 + 2.0 ** -7)
    assert torch.tensor([z], dtype=torch.float64).float().to(torch.bfloat16).float().item() == 1.0 + 2.0 ** -6
    rng = np.random.default_rng(5)
    v = rng.standard_normal(2000).astype(np.float32)  # float32 values: torch's cast is then a single rounding too
    assert np.array_equal(per.round_bfloat16(v.astype(np.float64)), torch.from_numpy(v).to(torch.bfloat16).float().numpy())


def test_reference_gradient_on_a_case_worked_by_hand():
    # one sequence, two pdfs, two frames, K = 4; risks 0, 2, 4, 6: weights -1, -1/3, 1/3, 1
    y = np.array([[[0.0, 31.0], [30.0, -30.0]]])  # (B, C, T); (pdf 0, frame 1) is outside the clamp
    pdfs = np.array([[[0, 1], [0, 1], [1, 0], [-1, 0]]])
    w = per.risk_weights([[0, 2, 4, 6]])
    assert np.array_equal(w, np.array([[-1.0, -1.0 / 3.0, 1.0 / 3.0, 1.0]]))
    g = per.risk_grad(y, pdfs, w, [2.0], "float32")
    want = np.array([[[(0.0 + 2.0 * -1.0) + 2.0 * (-1.0 / 3.0), 0.0], [2.0 * (1.0 / 3.0), (0.0 + 2.0 * -1.0) + 2.0 * (-1.0 / 3.0)]]])
    assert g.dtype == np.float32 and np.array_equal(g, want.astype(np.float32))
    assert not np.signbit(g[0, 0, 1])
    g = per.risk_grad(y, pdfs, w, [2.0], "float32", frames=[1])
    assert np.array_equal(g[..., 1], np.zeros((1, 2), np.float32)) and g[0, 0, 0] == want.astype(np.float32)[0, 0, 0]


# ---- the library's checks in front of any device call ----
def test_edit_distance_entry_checks_its_arguments():
    S, K, T, P, M = 3, 5, 11, 12, 7
    need = int(lib.tc_paths_edit_distance_workspace_bytes(S, K, T))
    assert need == (4 * S * K * T + 255) // 256 * 256
    for bad in ((0, K, T), (S, 0, T), (S, K, 0), (-1, K, T)):
        assert int(lib.tc_paths_edit_distance_workspace_bytes(*bad)) == TC_ERR_INVALID_ARGUMENT
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails before a device call
    keys = (b"path_edit_launches", b"sampled_risk_grad_launches")
    before = [int(lib.tc_debug_counter(key)) for key in keys]
    assert min(before) >= 0

    def call(s=S, k=K, pdf=fake, fr=None, t=T, tok=fake, st=None, p=P, ref=fake, rl=fake, m=M, dist=fake, ln=fake, out=fake,
             ws=None, nbytes=0):
        return lib.tc_paths_edit_distance(s, k, pdf, fr, t, tok, st, p, ref, rl, m, dist, ln, out, ws, nbytes, 0, None)

    for kwargs in (dict(pdf=None), dict(tok=None), dict(dist=None), dict(ln=None), dict(ref=None), dict(rl=None), dict(s=0),
                   dict(k=0), dict(t=0), dict(p=0), dict(s=-2), dict(m=-1), dict(pdf=C.c_void_p(4098)), dict(fr=C.c_void_p(4097)),
                   dict(tok=C.c_void_p(4098)), dict(ref=C.c_void_p(4099)), dict(rl=C.c_void_p(4098)),
                   dict(dist=C.c_void_p(4098)), dict(ln=C.c_void_p(4097)), dict(out=C.c_void_p(4098))):
        assert call(**kwargs) == TC_ERR_INVALID_ARGUMENT, kwargs
    assert call(m=4097) == TC_ERR_UNSUPPORTED
    assert call(m=1 << 20) == TC_ERR_UNSUPPORTED
    assert call(s=1 << 20, k=1 << 12) == TC_ERR_UNSUPPORTED
    # without a token output the hypotheses need the workspace
    assert call(out=None, ws=None) == TC_ERR_WORKSPACE
    assert call(out=None, ws=fake, nbytes=need - 1) == TC_ERR_WORKSPACE
    assert call(out=None, ws=C.c_void_p(4100), nbytes=need) == TC_ERR_WORKSPACE
    assert [int(lib.tc_debug_counter(key)) for key in keys] == before  # nothing was launched


def test_risk_gradient_entry_checks_its_arguments():
    S, K, T, P = 3, 4, 6, 10
    fake = C.c_void_p(4096)
    keys = (b"path_edit_launches", b"sampled_risk_grad_launches")
    before = [int(lib.tc_debug_counter(key)) for key in keys]

    def call(s=S, k=K, t=T, p=P, pdf=fake, fr=None, w=fake, go=fake, x=fake, dtype=TC_DTYPE_F32, xs=(P * T, T, 1), g=fake,
             gs=(P * T, T, 1), n=S * P * T):
        return lib.tc_sampled_risk_grad(s, k, t, p, pdf, fr, w, go, x, dtype, xs[0], xs[1], xs[2], g, gs[0], gs[1], gs[2], n, 0,
                                        None)

    for kwargs in (dict(pdf=None), dict(w=None), dict(go=None), dict(x=None), dict(g=None), dict(s=0), dict(k=0), dict(t=0),
                   dict(p=0), dict(dtype=3), dict(dtype=-1), dict(xs=(-1, T, 1)), dict(gs=(P * T, 0, 1)), dict(gs=(P * T, T, -1)),
                   dict(n=S * P * T - 1), dict(n=0), dict(gs=(P * T + 1, T, 1)), dict(pdf=C.c_void_p(4098)),
                   dict(fr=C.c_void_p(4098)), dict(w=C.c_void_p(4100)), dict(go=C.c_void_p(4100)), dict(x=C.c_void_p(4098)),
                   dict(g=C.c_void_p(4097))):
        assert call(**kwargs) == TC_ERR_INVALID_ARGUMENT, kwargs
    assert call(k=1025) == TC_ERR_UNSUPPORTED
    assert [int(lib.tc_debug_counter(key)) for key in keys] == before


# ---- the wrappers' checks ----
def test_wrappers_check_before_any_library_call():
    pdfs = torch.zeros((2, 3, 5), dtype=torch.int32)
    refs = torch.tensor([[1, 2, -1], [3, -1, -1]])
    tok = torch.arange(4)
    before = int(lib.tc_debug_counter(b"path_edit_launches"))
    for bad, match in ((dict(pdfs=pdfs.float()), "int32 or int64"), (dict(pdfs=pdfs[0, 0]), "int32 or int64"),
                       (dict(pdfs=pdfs[:, :0]), "empty axis"), (dict(token_of_pdf=torch.zeros((2, 2), dtype=torch.int64)), "vector"),
                       (dict(token_of_pdf=torch.zeros(4)), "integers"), (dict(starts=[1, 0, 1]), "starts"),
                       (dict(frames=[5]), "frames"), (dict(refs=refs[0]), "refs"), (dict(refs=refs[:1]), "refs"),
                       (dict(refs=refs.float()), "refs"), (dict(refs=None), "refs is required"),
                       (dict(ref_lengths=[2, 1, 0]), "ref_lengths"), (dict(return_tokens=1), "return_tokens"),
                       (dict(refs=torch.tensor([[1, -1, 2], [3, -1, -1]])), "behind a negative"),
                       (dict(refs=torch.zeros((2, 4097), dtype=torch.int64), ref_lengths=[1, 1]), "4096"),
                       (dict(), "on the GPU")):
        kwargs = dict(pdfs=pdfs, token_of_pdf=tok, refs=refs)
        kwargs.update(bad)
        with pytest.raises(ValueError, match=match):
            path_edit_distance(**kwargs)
    with pytest.raises(ValueError, match="on the GPU"):
        path_tokens(pdfs, tok)
    with pytest.raises(ValueError, match="starts"):
        path_tokens(pdfs, tok, starts=[True])
    x = torch.zeros((2, 4, 5), requires_grad=True)
    risks = torch.tensor([[0.0, 1.0, 2.0], [1.0, 1.0, 0.0]])
    with pytest.raises(ValueError, match="fused must be a bool"):
        sampled_risk_surrogate(x, pdfs, risks, fused=1)
    with pytest.raises(ValueError, match="K >= 2"):
        sampled_risk_surrogate(x, pdfs[:, :1], risks[:, :1], fused=True)
    with pytest.raises(ValueError, match="on the GPU"):
        sampled_risk_surrogate(x, pdfs, risks, fused=True)
    # the default route is untouched: plain torch, CPU tensors included
    sampled_risk_surrogate(x, pdfs, risks).sum().backward()
    assert x.grad is not None
    assert int(lib.tc_debug_counter(b"path_edit_launches")) == before
    import torchain.functions
    assert torchain.functions.path_edit_distance is path_edit_distance
    assert torchain.functions.path_tokens is path_tokens
