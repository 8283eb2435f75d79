"""The out-of-range penalty (``chain_loss(..., out_of_range_regularize=c)``, ``tc_chain_step_penalized``) without a GPU: the
keyword on every entry point, its validation, the C entry and its documentation, the numpy statement of the term that the GPU
tests hold the kernels to, the definition against a float64 finite difference, the torch statement of the fallback routes,
and the CPU oracle on the GPU tests' small inputs (none of them may take the soft-failure route)."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import torchain.functions
from torchain_amd import functions, ops, parallel
from torchain_amd._lib import LIB_PATH, lib

import out_of_range_cases as oor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "torchain_hip.h")
REFERENCE = ["input", "den_graph", "supervision", "l2_regularize", "leaky_hmm_coefficient", "xent_regularize", "xent_input",
             "kaldi_way"]


@pytest.mark.parametrize("fn,before", [
    (functions.chain_loss, REFERENCE),
    (torchain.functions.chain_loss, REFERENCE),
    (ops.chain_loss_op, REFERENCE),
    (parallel.chain_loss_data_parallel, REFERENCE + ["group", "even_if_alone"]),
])
def test_keyword_is_trailing_and_keyword_only(fn, before):
    """The pinned signatures stay (tests/test_deriv_weights_host.py): the option comes behind them, through ``**options``.  It
    can only be passed by keyword, a misspelt one is the TypeError a declared keyword would give, and the default is 0.0."""
    code = fn.__code__
    assert list(code.co_varnames[:code.co_argcount]) == before
    assert fn.__kwdefaults__ == {"deriv_weights": None}
    assert code.co_flags & inspect.CO_VARKEYWORDS and not code.co_flags & inspect.CO_VARARGS
    assert code.co_varnames[code.co_argcount + code.co_kwonlyargcount] == "options"  # (behind everything declared)
    x = torch.zeros(4, 3, requires_grad=True)
    with pytest.raises(TypeError, match="out_of_range_regularise"):
        fn(x, None, None, out_of_range_regularise=0.01)
    with pytest.raises(TypeError):  # (not positional)
        fn(x, None, None, 0.0, 1e-5, 0.0, None, False, *([None, False] if "group" in before else []), None, 0.01)
    assert functions._options({}) == 0.0  # (the reference has no such option: not Kaldi's 0.01)
    assert functions._options({"out_of_range_regularize": 0.25}) == 0.25


def test_shim_and_low_level_call_take_the_keyword():
    assert torchain.functions.chain_loss is functions.chain_loss
    assert list(inspect.signature(functions.chain_loss).parameters) == REFERENCE  # (what introspection shows stays the reference's)
    p = inspect.signature(functions.compute_chain_objf_and_deriv).parameters["out_of_range_regularize"]
    assert p.kind is p.KEYWORD_ONLY and p.default == 0.0
    for fn in (functions.chain_loss, ops.chain_loss_op, parallel.chain_loss_data_parallel):
        assert "out_of_range_regularize" in (fn.__doc__ or "") + (functions.__doc__ or "")


def test_registered_operator_takes_the_factor():
    """An operator of its own, as the C entry is: ``chain_step`` keeps its schema and is the new one's c == 0 case."""
    old = str(torch.ops.torchain_amd.chain_step.default._schema)
    new = str(torch.ops.torchain_amd.chain_step_penalized.default._schema)
    args = lambda s: s.split("(", 1)[1].split(")")[0].split(", ")  # noqa: E731
    assert args(new)[:-1] == args(old) and args(new)[-1].startswith("float out_of_range_regularize=0"), (old, new)
    assert old.split(") -> ")[1] == new.split(") -> ")[1]


@pytest.mark.parametrize("bad", [-1e-3, -0.5, float("nan"), float("inf"), -float("inf"), 1e39, "much", None, True])
def test_bad_values_raise_before_the_gpu_is_touched(bad):
    """ValueError from every entry point, on CPU tensors and without a graph: nothing else has been looked at yet."""
    x = torch.zeros(4, 3, requires_grad=True)
    with pytest.raises(ValueError):
        functions._out_of_range(bad)
    for fn in (functions.chain_loss, ops.chain_loss_op, parallel.chain_loss_data_parallel):
        with pytest.raises(ValueError, match="out_of_range_regularize"):
            fn(x, None, None, out_of_range_regularize=bad)
    with pytest.raises(ValueError, match="out_of_range_regularize"):
        functions.compute_chain_objf_and_deriv(None, None, x, None, None, None, 0.0, 1e-5, 0.0, out_of_range_regularize=bad)


@pytest.mark.parametrize("ok", [0, 0.0, 0.01, 1, np.float32(0.25), torch.tensor(0.5)])
def test_good_values_come_back_as_floats(ok):
    got = functions._out_of_range(ok)
    assert isinstance(got, float) and got == float(ok)


def test_c_entry_is_declared_documented_and_validates():
    text = open(HEADER).read()
    assert "int tc_chain_step_penalized(" in text
    doc = text[:text.index("int tc_chain_step_penalized(")].rsplit("/*", 1)[1]
    for phrase in ("PenalizeOutOfRange", "restated", "p  = y > L ? y - L : (y < -L ? y + L : 0)", "fl32(2 * c)", "not fused",
                   "never xent_input", "random", "supervision's weight", "soft-failure", "p == 0", "untouched", "rounded once",
                   "three_d != 0", "three_d == 0, 16-bit", "three_d == 0, float32", "grad == NULL", "unchanged",
                   "TC_ERR_INVALID_ARGUMENT"):
        assert phrase in doc, phrase
    raw = C.CDLL(LIB_PATH)
    assert hasattr(raw, "tc_chain_step_penalized")
    # bad factors are refused at the C entry too (-1: TC_ERR_INVALID_ARGUMENT), whatever else is passed
    vp = C.c_void_p
    one = C.c_void_p(16)
    for bad in (-1.0, float("nan"), float("inf")):
        rc = lib.tc_chain_step_penalized(one, one, one, None, 0, 8, 0.0, 1e-5, 0.0, 0, None, None, one, None, None, None, bad, 0,
                                         vp(None), 0, 0, vp(None))
        assert rc == -1, (bad, rc)


def test_limit_is_one_named_constant():
    assert functions.OUTPUT_LIMIT == 30.0 == float(oor.LIMIT)
    src = open(os.path.join(ROOT, "torchain_amd", "csrc", "chain_internal.h")).read()
    assert "constexpr float kOutputLimit = 30.0f;" in src
    for name in ("half_io.h", "layout_kernels.hip", "layout_rows_kernels.hip"):  # (penalize, and the passes that call it)
        kernels = open(os.path.join(ROOT, "torchain_amd", "csrc", name)).read()
        assert "penalize(" in kernels or "last_elem<" in kernels, name
        assert "30.0f" not in kernels, name
    assert "kOutputLimit" in open(os.path.join(ROOT, "torchain_amd", "csrc", "half_io.h")).read().split("float penalize(")[1]


def _inputs():
    for spec in (oor.SMALL, oor.MEDIUM):
        for kind in oor.KINDS:
            yield oor.workload(spec, kind)[2]
    special = np.array([[30.0, -30.0, np.nextafter(np.float32(30), np.float32(31)), -30.000002, 31.5, -50.0, np.nan, np.inf,
                         -np.inf, 0.0, -0.0, 3.0e38, -3.0e38, 29.999998]], np.float32)
    yield special


@pytest.mark.parametrize("c", [0.01, 0.25, 1.0 / 3.0, 7.5])
def test_numpy_term_is_within_one_ulp_of_float64(c):
    """The float32 statement the GPU tests use, against 2 * c * p in float64 from the same float32 inputs: p is exact (the
    subtraction of two float32 values within a factor of two of each other, or of a small constant), and the product of two
    float32 factors of which one is itself rounded lands within 1 ulp."""
    for y in _inputs():
        t = oor.term(y, c)
        y64 = y.astype(np.float64)
        fin = np.isfinite(y64)
        p64 = np.where(fin, y64 - np.clip(y64, -30.0, 30.0), 0.0)
        np.testing.assert_array_equal(oor.excess(y).astype(np.float64)[fin], p64[fin])
        want = 2.0 * float(c) * p64
        big = np.abs(want) > float(np.finfo(np.float32).max)  # (the float32 product overflows: the term is +-inf there)
        assert np.all(np.isinf(t[big])) and np.all(np.sign(t[big]) == np.sign(want[big]))
        ulp = np.spacing(np.abs(want[~big]).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(t.astype(np.float64)[~big] - want[~big]) <= ulp), c
        assert np.all(t[~fin] == 0) and np.all(t[np.abs(y) <= 30] == 0)
        assert not np.signbit(t[np.abs(y) <= 30]).any()  # (c >= 0: where p == 0 the term is +0)


@pytest.mark.parametrize("c", [0.01, 0.5])
def test_term_is_the_gradient_of_the_penalty_function(c):
    """Central finite differences in float64 of F(y) = c * sum((y - clip(y))**2), element by element, against 2c * p."""
    for y in _inputs():
        y64 = y.astype(np.float64)
        fin = np.isfinite(y64) & (np.abs(y64) < 1e6)  # (a step of 1e-4 is below the spacing of 3e38)
        v = y64[fin]
        F = lambda z: c * (z - np.clip(z, -30.0, 30.0)) ** 2  # noqa: E731  (the sum's terms: each depends on one element)
        h = 1e-4
        on_kink = np.abs(np.abs(v) - 30.0) < h
        fd = (F(v + h) - F(v - h)) / (2 * h)
        want = oor.term(y, c).astype(np.float64)[fin]
        scale = np.maximum(np.abs(want), 1.0)
        assert np.all(np.abs(fd - want)[~on_kink] <= 1e-6 * scale[~on_kink])
        assert np.all(np.abs(fd - want)[on_kink] <= 2 * c * h)  # (F is C1: across the kink the slope moves by 2c per unit)


@pytest.mark.parametrize("c", [0.01, 0.25])
def test_torch_statement_of_the_fallback_routes_is_bit_for_bit(c):
    rng = np.random.default_rng(3)
    for y in _inputs():
        g = rng.normal(size=y.shape).astype(np.float32)
        g[..., ::5] = -0.0
        g[..., 1::7] = 0.0
        want = oor.penalized(g, y, c)
        got = functions._penalized(torch.from_numpy(g), torch.from_numpy(y), c).numpy()
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
        inside = ~(np.abs(y) > 30) | ~np.isfinite(y)
        np.testing.assert_array_equal(got.view(np.int32)[inside], g.view(np.int32)[inside])


@pytest.mark.parametrize("spec", [oor.SMALL, oor.MEDIUM] + list(oor.TILED.values()),
                         ids=["small", "medium"] + ["tiled%d" % T for T in oor.TILED])
def test_oracle_takes_no_soft_failure_on_the_gpu_tests_inputs(oracle, spec):
    """The inputs of the 'step succeeded' GPU tests: objf finite and not -10 * weight, for every kind of input."""
    objf = {}
    for kind in oor.KINDS:
        fst, sup, y, n = oor.workload(spec, kind)
        assert (n == 0) == (kind in ("none", "edge")), (kind, n)
        ref = oracle.compute_chain_objf_and_deriv(oracle.DenGraph(fst), sup, y, 0.0, 1e-5)
        assert not oor.took_soft_failure(ref["objf"], ref["weight"]), (kind, ref["objf"], ref["weight"])
        objf[kind] = ref["objf"]
    assert objf["none"] != objf["dense"]
