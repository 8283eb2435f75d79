"""The one route of ``chain_loss`` at its edges, on the GPU: evaluation steps on pairs that do not go to the step together
(they are normalised as the training step's are), the pairs ``_run_step`` and ``chain_loss_op`` refuse before any library call,
and the dtypes the step does not take.  Shapes: the channel-last tests' smallest (P = 20, B = 3, T = 5)."""
import pytest
import torch

from torchain_amd import functions, io, synth
from torchain_amd._lib import lib
from torchain_amd.functions import ChainResults, chain_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, B, T = 20, 3, 5
L2, LEAKY, XREG = 5e-4, 0.05, 0.1
_cache = {}


def _workload():
    if not _cache:
        fst = synth.random_den_fst(40, 4, P, seed=6)
        _cache.update(graph=io.DenominatorGraph(fst, P).prepare(DEV),
                      sup=io.Supervision.from_synth(synth.random_supervision(fst, B, T, 2, seed=1)),
                      y=torch.from_numpy(synth.random_nnet_output(B, T, P, seed=1)).to(DEV),
                      xe=torch.from_numpy(synth.random_nnet_output(B, T, P, seed=2)).to(DEV))
    return _cache


def _strided(rows, pad=4):
    wide = torch.full((rows.shape[0], rows.shape[1] + pad), 1e30, dtype=rows.dtype, device=rows.device)  # (a misread row shows)
    wide[:, :rows.shape[1]] = rows
    return wide[:, :rows.shape[1]]


def _bct(rows):
    return rows.view(T, B, P).permute(1, 2, 0).contiguous()


def _eval(x, xe, kaldi_way):
    s = _workload()
    with torch.no_grad():
        loss, res = chain_loss(x, s["graph"], s["sup"], L2, LEAKY, XREG, xe, kaldi_way)
    return loss, res.data.clone(), res.xent_objf


@pytest.mark.parametrize("kaldi_way", [True, False])
@pytest.mark.parametrize("pair", ["strided + contiguous", "contiguous + strided", "(B, C, T) + 2-D"])
def test_evaluation_normalises_mixed_pairs(pair, kaldi_way):
    """Under ``no_grad``: results, loss and xent_objf bit for bit those of the same call on contiguous copies."""
    s = _workload()
    x, xe = {"strided + contiguous": (_strided(s["y"]), s["xe"]), "contiguous + strided": (s["y"], _strided(s["xe"])),
             "(B, C, T) + 2-D": (_bct(s["y"]), s["xe"])}[pair]
    assert functions._step_plan(x, xe) is None
    got = _eval(x, xe, kaldi_way)
    want = _eval(s["y"].clone(), s["xe"].clone(), kaldi_way)
    assert got[0].dtype == want[0].dtype and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert got[2] == want[2] and got[2] is not None


def test_row_strides_that_differ_are_refused_before_any_library_call():
    from torchain_amd.ops import chain_loss_op
    s = _workload()
    for x, xe in ((_strided(s["y"]), s["xe"]), (s["y"], _strided(s["xe"])), (_strided(s["y"]), _strided(s["xe"], 8))):
        before = lib.tc_debug_counter(b"den_launches")
        for want_grad in (True, False):
            with pytest.raises(ValueError):
                functions._run_step(x, xe, ChainResults(), s["graph"], s["sup"], L2, LEAKY, XREG, True, want_grad=want_grad)
        with pytest.raises(ValueError):
            chain_loss_op(x.detach().requires_grad_(True), s["graph"], s["sup"], L2, LEAKY, XREG, xe, True)
        with pytest.raises(ValueError), torch.no_grad():
            chain_loss_op(x, s["graph"], s["sup"], L2, LEAKY, XREG, xe, True)
        assert lib.tc_debug_counter(b"den_launches") == before
    # ... and so is every other pair the planner would not have produced
    before = lib.tc_debug_counter(b"den_launches")
    for x, xe in ((_bct(s["y"]), s["xe"]), (_bct(s["y"]), _bct(s["xe"]).transpose(1, 2).contiguous().transpose(1, 2)),
                  (s["y"], s["xe"].bfloat16()), (s["y"].double(), None), (s["y"].cpu(), None)):
        with pytest.raises(ValueError):
            functions._run_step(x, xe, ChainResults(), s["graph"], s["sup"], L2, LEAKY, XREG, True, want_grad=False)
        with pytest.raises(ValueError):
            chain_loss_op(x, s["graph"], s["sup"], L2, LEAKY, XREG, xe, True)
    assert lib.tc_debug_counter(b"den_launches") == before


@pytest.mark.parametrize("three_d", [True, False])
def test_other_dtypes_keep_their_behaviour(three_d):
    """A dtype outside float32 / bfloat16 / float16: ``ValueError`` when a gradient is wanted, up-cast under ``no_grad``
    (the values of the call on ``input.float()``)."""
    s = _workload()
    y = _bct(s["y"]) if three_d else s["y"]
    with pytest.raises(ValueError):
        chain_loss(y.double().requires_grad_(True), s["graph"], s["sup"], L2, LEAKY)
    with torch.no_grad():
        loss, res = chain_loss(y.double(), s["graph"], s["sup"], L2, LEAKY)
        loss32, res32 = chain_loss(y, s["graph"], s["sup"], L2, LEAKY)
    assert torch.equal(res.data, res32.data) and float(loss) == float(loss32)
