"""``chain_loss`` / ``ChainResults``: the autograd wrapper of the reference
(``torchain/functions.py:9-138``) on top of the HIP C ABI.

Same names, argument meaning, defaults and quirks as the reference:

* ``ChainResults.data`` is a CPU float tensor ``[objf, l2_term, weight]``; ``loss = -objf/weight``
  (l2 not included, ``functions.py:19``).
* ``chain_loss`` accepts ``(B, C, T)`` or ``(T*B, C)`` input; 3-D input is permuted to frame-major
  rows ``t*B + b`` (``functions.py:118-125``) inside the library, which also permutes the gradients back.
* one route: ``plan_step_inputs`` decides, from shapes, strides and dtypes alone, how any ``(input, xent_input)`` pair becomes
  one the library takes in ONE call (``_ChainStep`` / ``_run_step``, ``tc_chain_step_strided``) -- as it is, or after
  ``.float()``, ``to2d`` or ``.contiguous()`` (tracked by autograd when a gradient is wanted).  Training, evaluation and
  ``ops.chain_loss_op`` share that plan; ``_run_step`` refuses whatever the planner would not have produced.
* backward returns ``-mmi_grad`` for the input and ``-xent_regularize * xent_grad`` for
  ``xent_input``; ``grad_output`` is ignored and nothing is divided by ``weight``
  (``functions.py:106-115``).
* ``kaldi_way=False`` re-runs the whole objective on ``xent_input`` and overwrites ``results`` and
  the MMI gradient with that second call's outputs, as the reference does (``functions.py:96-103``).
* bfloat16 / float16 inputs (a mixed-precision model's output) take the same one call (``tc_chain_step_typed``): the
  library widens them as it reads them and rounds the gradients once as it writes them, so ``results`` are those of
  ``input.float()``, the loss is that loss in the input's dtype and the gradients are the float32 ones ``.to(dtype)``.
  ``input`` and ``xent_input`` of different dtypes are up-cast to float32 first (correct, not the fast path).
* ``deriv_weights`` (Kaldi's per-frame ``<DW>`` / ``<DW2>`` weights, ``io.Example.deriv_weights``): a ``(T*B,)`` vector in
  the frame-major row order ``t*B + b``.  Each gradient element becomes ``w[row] * g``, one float32 multiply of the
  unweighted value (rounded once for 16-bit inputs), as Kaldi's ``MulRowsVec`` after ``ComputeChainObjfAndDeriv``;
  ``results``, the loss and ``xent_objf`` are unchanged.  ``None`` (the default) keeps the reference's behaviour, which
  drops the weights.  The one call applies them in the passes it makes anyway (``tc_chain_step_weighted``).
* ``out_of_range_regularize`` (after Kaldi's ``PenalizeOutOfRange``, restated in ``torchain_hip.h``): the kernels take
  ``exp(y)`` at ``clamp(y, -30, 30)``, so an output outside that range has lost the objective's restoring force.  With
  ``c > 0`` every gradient element of the chain output gets ``t = fl32(2c) * p`` added, ``p`` the part of ``y`` beyond
  ``+-30`` (0 inside, and for NaN / inf): descent on ``c * sum((y - clamp(y))**2)``, on every row, not scaled by the
  supervision's weight, in front of ``deriv_weights``.  ``results``, the loss, ``xent_objf`` and the xent gradient do not
  change; without a gradient the option does nothing.  ``0.0`` (the default, not Kaldi's 0.01) keeps the reference's
  behaviour.  The one call adds it in the passes it makes anyway (``tc_chain_step_penalized``).
* channel-last views: a 3-D input is still ``(B, C, T)``, but a view of that shape whose channel stride is 1 -- a batch-first
  model's ``out.transpose(1, 2)``, PyTorch's time-major ``out.permute(1, 2, 0)``, the two halves ``out[..., :P]`` /
  ``out[..., P:]`` of a joint head -- takes the one call as it is (``classify_layout``, ``tc_chain_step_strided``): a
  time-major view IS the 2-D layout and is passed as such, without a copy; any other one is gathered and its gradients
  scattered by the library, one pass each.  Values: bit for bit those of the call on ``input.contiguous()`` (float16: up to
  the sign of an exactly zero gradient element, where the view gives the float32 gradient's ``.to(float16)``).  ``xent_input``
  must be a view with the same strides (or absent); any other combination is made contiguous first (``plan_step_inputs``).
* ``per_sequence=True`` (keyword-only, through ``**options``): ``ChainResults.per_sequence`` holds every sequence's own
  ``num_logprob``, ``den_logprob``, ``objf``, ``frames``, ``xent_sum``, ``sum_y2`` and ``status`` (0 ok; bit 1 numerator, 2
  denominator, 4 alpha-beta check non-finite), read lazily like ``data``; ``ChainResults.failed`` the indices whose status is
  not 0.  Nothing else changes.  ``on_failure="sequence"`` (default ``"minibatch"``, the reference's behaviour) implies it and
  isolates a failed sequence: the objective, weight, l2 term, loss and cross-entropy objective are the survivors' and the failed
  sequence's gradient rows are ``+0`` like a ragged minibatch's padding; with nothing failed every output is bit for bit the
  default call's (``tc_chain_step_per_sequence``).
* ``xent_log_softmax=True`` (keyword-only, through ``**options``; needs ``kaldi_way=True``): Kaldi's cross-entropy head ends
  in a log-softmax, the objective ``sum(xent_output * xent_deriv)`` is taken on its log-probabilities and the derivative is
  back-propagated through it.  The reference has none in training (``torchain/functions.py:88-89`` is a TODO, only
  ``forward.py:67`` applies ``log_softmax``), so by default the gradient returned for ``xent_input`` is ``V = -xent_regularize
  * w * gamma_num`` (times ``deriv_weights``), descent on an objective linear in ``xent_input``.  With the option the call
  folds the log-softmax of the RAW ``xent_input`` in: the gradient becomes ``V - rowsum(V) * softmax(xent_input)`` row by row
  (dense; a row without posteriors -- padding, ``deriv_weights == 0``, a failed sequence -- is ``+0`` whatever ``xent_input``
  holds there) and ``results.xent_objf`` is taken on ``log_softmax(xent_input)``.  Everything formed from ``input`` keeps its
  bits.  It replaces ``F.log_softmax(xe, dim=1)`` in front of the call, its backward and the activation that backward keeps
  (``tc_chain_step_log_softmax``).  Not a bool, or ``kaldi_way=False`` with it: ``ValueError`` before any
  library call.  Without the xent branch it does nothing.  ``torchain_amd/ops.py`` and the split entries do not take it.
* ``boost=0.0, boost_ref=None, boost_pdf_class=None, boost_accuracy=None`` (keyword-only, through ``**options``): boosted
  LF-MMI (bMMI).  Every denominator path's weight is multiplied by ``exp(-boost * A(path))``, ``A`` the path's frame
  accuracy against a reference, so the model must beat a competitor by a margin that grows with its error.  The accuracy
  ``a_t(j)`` is ``den_expected_accuracy``'s: the hard form ``boost_ref`` (int32 / int64 ``(B, Tmax)``, as ``best_path`` returns
  it; ``-1`` or an out-of-range entry: the frame scores nothing) with an optional ``boost_pdf_class`` (int ``(P,)``, identity
  when None), ``a = 1`` iff ``class(j) == class(ref_t)``; or the dense form ``boost_accuracy``, a float32 ``(Tmax*B, C)`` matrix,
  row ``t*B + s``, unit column stride (``Supervision.posteriors``), any finite values, held constant.  The denominator alone
  runs on ``y_b = fl32(y.float() - fl32(boost) * a)`` (two float32 roundings); the numerator, the l2 term and its gradient,
  the penalty, ``deriv_weights`` and the cross-entropy branch act on the true ``y``: ``objf = w * (num_logprob(y) -
  den_logprob(y_b))``, which is no longer bounded by 0 -- for ``a`` in [0, 1] and ``boost >= 0`` on a composed supervision it
  is bounded by ``w * boost * sum(T_s)``.  ``results``, the loss, ``xent_objf`` and ``per_sequence`` keep their layout;
  ``den_logprob`` is the boosted denominator's.  ``boost == 0.0``, or neither reference given, is the call without the option,
  entry and bits.  Both references with ``boost != 0``, a ``boost`` that is not finite, wrong shapes / dtypes / devices, a
  ``boost_accuracy`` that requires grad, and ``boost != 0`` with the xent branch and ``kaldi_way=False``: ``ValueError`` before
  any library call.  Rows and entries of a ragged handle's padding frames are never read.  Under ``torch.no_grad()`` the
  forward-only step is boosted too.  No host synchronisation: the tensors are read where they lie (an int64 ``boost_ref`` is
  cast on the device), so the step stays capturable (``tc_chain_step_boosted``).  ``torchain_amd/ops.py``, the split entries and
  ``chain_loss_data_parallel`` do not take it.
"""
import ctypes as C
import inspect

import torch
from torch.autograd import Function

from . import io
from ._lib import (TC_DTYPE_BF16, TC_DTYPE_F16, TC_DTYPE_F32, TC_LAYOUT_BCT, TC_LAYOUT_CHANNEL_LAST, TC_LAYOUT_ROWS, check,
                   lib)

# element types tc_chain_step(_typed) takes as they are
_STEP_DTYPES = {torch.float32: TC_DTYPE_F32, torch.bfloat16: TC_DTYPE_BF16, torch.float16: TC_DTYPE_F16}
_HALF = (torch.bfloat16, torch.float16)


class ChainResults:
    def __init__(self):
        # ``data``: the CPU float tensor [objf, l2_term, weight] of the reference (functions.py:11-21).  It is read from
        # the device when it is first looked at (one 12-byte D2H), not inside ``chain_loss``: a training loop that
        # logs every few steps enqueues its steps without waiting for the GPU in between -- which is what lets the
        # reader's hand-over of the next minibatch (io.RandExample) hide behind the running step.
        self._host = torch.zeros(3)
        self._stale = False
        # Device-side originals: [objf, l2_term, weight] as the kernels left them (float32[3]) and Kaldi's
        # cross-entropy objective sum(xent_output * xent_deriv) (float64[1]; [K] nnet-chain-training.cc, a TODO in
        # the reference, functions.py:88-89).  The data-parallel wrapper reduces THESE (one collective, no host
        # round trip); ``xent_objf`` is read from the device only when somebody asks for it.
        self._dev = None
        self._ready = None       # event recorded on the stream that produced _dev: the lazy reads wait for it
        self._xent_dev = None
        self._xent_ready = None
        self._xent_scale = 1.0
        self._xent_host = None
        self._defer_host_copy = False  # set by chain_loss_data_parallel: the one D2H follows the all-reduce
        # ``chain_loss(..., per_sequence=True)``: the sequences' own values, float64 (S, 6) on the device as the library
        # wrote them (tc_chain_step_per_sequence), read when ``per_sequence`` is first looked at; local to the rank
        self._seq_dev = None
        self._seq_ready = None
        self._seq_weight = 1.0
        self._seq_host = None

    @property
    def data(self):
        if self._stale and not self._defer_host_copy and self._dev is not None:
            # the copy runs on whatever stream is current NOW, which need not be the one chain_loss ran on
            if self._ready is not None:
                torch.cuda.current_stream(self._dev.device).wait_event(self._ready)
            self._host.copy_(self._dev)
            self._stale = False
        return self._host

    def invalidate(self):
        """The device-side values changed behind this object -- a captured graph holding the step was replayed: the next
        read of ``data`` / ``xent_objf`` copies them again (on the current stream, behind the replay)."""
        if self._dev is not None:
            self._stale = True
        if self._xent_dev is not None:
            self._xent_host = None
        self._seq_host = None

    @property
    def per_sequence(self):
        """The sequences' own values (``PerSequence``), or None unless ``chain_loss`` was asked for them.  Lazy: one D2H of
        ``S * 48`` bytes behind the step when first read; ``invalidate()`` makes the next read copy again."""
        if self._seq_host is None and self._seq_dev is not None:
            if self._seq_ready is not None:
                torch.cuda.current_stream(self._seq_dev.device).wait_event(self._seq_ready)
            self._seq_host = PerSequence(self._seq_dev.cpu(), self._seq_weight)
        return self._seq_host

    @property
    def failed(self):
        """Indices of the sequences whose status is not 0 (an int64 tensor), or None without ``per_sequence``."""
        seq = self.per_sequence
        return None if seq is None else torch.nonzero(seq.status, as_tuple=False).flatten()

    @data.setter
    def data(self, value):
        self._host = value
        self._stale = False
        self._dev = None  # (callers that sum ChainResults.data over steps own the numbers from here on)
        self._ready = None

    @property
    def xent_objf(self):
        """Kaldi's cross-entropy objective, or None without a xent branch.  Lazy: the value stays on the device
        until it is read (one 8-byte D2H), so a training step has no second host sync."""
        if self._xent_host is None and self._xent_dev is not None:
            if self._xent_ready is not None:
                torch.cuda.current_stream(self._xent_dev.device).wait_event(self._xent_ready)
            self._xent_host = float(self._xent_dev.item()) * self._xent_scale
        return self._xent_host

    @xent_objf.setter
    def xent_objf(self, value):
        self._xent_host = value
        self._xent_dev = None

    def __repr__(self):
        return "ChainResults(loss=%f, objf=%f, l2_term=%f, weight=%lf)" % (
            self.loss, self.data[0], self.data[1], self.data[2])

    @property
    def loss(self):
        return -self.data[0] / self.data[2]

    @property
    def xent_loss(self):
        """-xent_objf / weight, the per-frame cross-entropy Kaldi logs as 'output-xent'; None without a xent branch."""
        return None if self.xent_objf is None else -self.xent_objf / float(self.data[2])


class PerSequence:
    """One minibatch's sequences, each for itself: float64 CPU tensors of ``S`` entries ``num_logprob`` and ``den_logprob``
    (unweighted), ``objf`` = weight * (num - den), ``frames`` (the sequence's own ``T_s``), ``xent_sum`` (its share of
    ``xent_objf``, as the library scales it: times ``-xent_regularize``; 0 without a xent branch) and ``sum_y2`` (the l2
    term's sum), and the int64 tensor ``status``: 0 ok, bit 1 numerator, 2 denominator, 4 alpha-beta check non-finite."""

    STATUS_NUMERATOR, STATUS_DENOMINATOR, STATUS_ALPHA_BETA = 1, 2, 4

    def __init__(self, rows, weight):
        rows = rows.double().reshape(-1, 6)
        self.weight = float(weight)
        self.num_logprob, self.den_logprob, self.sum_y2, self.xent_sum, self.frames = (rows[:, i].clone() for i in range(5))
        self.status = rows[:, 5].to(torch.int64)
        self.objf = self.weight * (self.num_logprob - self.den_logprob)

    def __len__(self):
        return int(self.status.numel())

    def __repr__(self):
        return "PerSequence(sequences=%d, failed=%s)" % (len(self), torch.nonzero(self.status).flatten().tolist())


_workspaces = {}  # (device, stream) -> workspace, most recently used last
_MAX_WORKSPACES = 4  # per process: a C3 workspace is 1.3 GB, and streams come and go


def _workspace(device, stream, nbytes):
    """The caller's workspace for (device, stream): reused from step to step, at most ``_MAX_WORKSPACES`` alive (least
    recently used dropped; the caching allocator keeps a dropped block away from other streams until the work
    queued on its own stream has passed)."""
    key = (device.index, stream)
    ws = _workspaces.pop(key, None)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    _workspaces[key] = ws
    while len(_workspaces) > _MAX_WORKSPACES:
        _workspaces.pop(next(iter(_workspaces)))
    return ws


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def compute_chain_objf_and_deriv(den_graph, supervision, nnet_output, results, nnet_output_deriv,
                                 xent_output_deriv, l2_regularize, leaky_hmm_coefficient, xent_regularize,
                                 as_gradients=False, holder=None, *, out_of_range_regularize=0.0):
    """The hot call: replaces ``my_lib.my_lib_ComputeChainObjfAndDeriv`` (``src/my_lib.h:33-42``).
    ``results`` is the CPU float[3] tensor of ``ChainResults`` and is filled on return.  ``as_gradients``: the two
    matrices come back as the reference's backward returns them (``functions.py:106-115``), ``-deriv`` and
    ``-xent_regularize * xent_deriv`` (``tc_chain_objf_and_grad``).  ``holder``: the ``ChainResults`` that keeps the
    device-side float[3]; when it asks for it (data-parallel use) the host copy is left to the caller.
    ``out_of_range_regularize``: the penalty of ``chain_loss`` on ``nnet_output_deriv`` (which is ``-g``, or ``g`` with
    ``as_gradients``), added with torch ops behind the call; ``results`` and ``xent_output_deriv`` do not change."""
    out_of_range_regularize = _out_of_range(out_of_range_regularize)
    assert nnet_output.is_cuda, "Only the HIP (ROCm) implementation is available"
    if nnet_output.dim() != 2 or nnet_output.stride(1) != 1 or nnet_output.dtype != torch.float32:
        raise ValueError("nnet_output must be a 2-D float32 tensor with unit column stride")
    if isinstance(den_graph, io.DenominatorGraph):
        den_graph.prepare(nnet_output.device)  # (a dictionary look-up after the first call on a device)
    den_ptr = den_graph.ptr if isinstance(den_graph, io.DenominatorGraph) else den_graph
    sup_ptr = supervision.ptr if isinstance(supervision, io.Supervision) else supervision
    rows, cols = nnet_output.shape
    device = nnet_output.device
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        n_seq = lib.tc_supervision_num_sequence(sup_ptr)
        n_frame = lib.tc_supervision_num_frame(sup_ptr)
        nbytes = lib.tc_chain_workspace_bytes(den_ptr, n_seq, n_frame)
        if nbytes < 0:
            check(int(nbytes), "tc_chain_workspace_bytes")
        ws = _workspace(device, stream, nbytes)
        res_dev = torch.empty(3, dtype=torch.float32, device=device)
        for t in (nnet_output_deriv, xent_output_deriv):
            if t is not None and (t.dim() != 2 or t.stride(1) != 1 or t.shape != nnet_output.shape):
                raise ValueError("derivative tensors must match nnet_output and have unit column stride")
        entry = lib.tc_chain_objf_and_grad if as_gradients else lib.tc_chain_objf_and_deriv
        rc = entry(
            den_ptr, sup_ptr, _ptr(nnet_output), rows, cols, nnet_output.stride(0), _ptr(res_dev),
            _ptr(nnet_output_deriv), nnet_output_deriv.stride(0) if nnet_output_deriv is not None else 0,
            _ptr(xent_output_deriv), xent_output_deriv.stride(0) if xent_output_deriv is not None else 0,
            float(l2_regularize), float(leaky_hmm_coefficient), float(xent_regularize), _ptr(ws), ws.numel(),
            device.index, C.c_void_p(stream))
        check(rc, "tc_chain_objf_and_grad" if as_gradients else "tc_chain_objf_and_deriv")
        if out_of_range_regularize > 0.0 and nnet_output_deriv is not None:
            g = nnet_output_deriv if as_gradients else -nnet_output_deriv
            g = _penalized(g, nnet_output, out_of_range_regularize)
            nnet_output_deriv.copy_(g if as_gradients else -g)
        if holder is not None:
            holder._dev = res_dev  # (ChainResults.data copies it to the host when it is read)
            holder._stale = True
            holder._ready = torch.cuda.Event()
            holder._ready.record(torch.cuda.current_stream(device))
        else:
            results.copy_(res_dev)  # 12-byte D2H, the one host sync of the call (reference: >= 4)
    return results


def xent_objective(xent_output, xent_output_deriv):
    """sum(xent_output * xent_output_deriv) on the device (``tc_xent_objf``), as a float64[1] DEVICE tensor: no host
    sync (``ChainResults.xent_objf`` reads it when asked)."""
    for t in (xent_output, xent_output_deriv):
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1 or t.dtype != torch.float32:
            raise ValueError("xent tensors must be 2-D float32 CUDA tensors with unit column stride")
    if xent_output.shape != xent_output_deriv.shape:
        raise ValueError("xent_input and its derivative must have the same shape")
    device = xent_output.device
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        ws = _workspace(device, stream, 4096)
        out = torch.empty(1, dtype=torch.float64, device=device)
        rc = lib.tc_xent_objf(_ptr(xent_output), xent_output.shape[0], xent_output.shape[1], xent_output.stride(0),
                              _ptr(xent_output_deriv), xent_output_deriv.stride(0), _ptr(out), _ptr(ws), ws.numel(),
                              device.index, C.c_void_p(stream))
        check(rc, "tc_xent_objf")
        return out


def _deriv_weights(w, rows):
    """``chain_loss``'s ``deriv_weights`` checked: None, or a 1-D real tensor of ``rows`` (S*T) entries on the CPU or a GPU.
    Raises ``ValueError`` otherwise, and for a CPU tensor under stream capture (its copy could not be captured)."""
    if w is None:
        return None
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.numel() != rows or w.is_complex() or w.dtype == torch.bool:
        raise ValueError("deriv_weights must be a 1-D real tensor of %d entries (one per frame-major row t*B + b), got %s"
                         % (rows, tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__))
    if not w.is_cuda and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise ValueError("deriv_weights must be a CUDA tensor under stream capture (a CPU tensor's copy is not captured)")
    return w


def _weights_on(w, device):
    """Checked ``deriv_weights`` as the library reads them: float32, contiguous, on ``device`` (a no-op when they are)."""
    return None if w is None else w.detach().to(device=device, dtype=torch.float32).contiguous()


# the limit of the network output (kOutputLimit in the library): exp(y) is taken at clamp(y, -30, 30), and the
# out-of-range penalty acts outside the same range
OUTPUT_LIMIT = 30.0


def _out_of_range(c):
    """``chain_loss``'s ``out_of_range_regularize`` checked: a finite real number >= 0, returned as a float.  Raises
    ``ValueError`` otherwise (before anything touches the GPU)."""
    try:
        value = float(c)
    except (TypeError, ValueError):
        raise ValueError("out_of_range_regularize must be a finite number >= 0, got %r" % (c,)) from None
    if isinstance(c, bool) or not (0.0 <= value < float("inf")) or not (2.0 * value < 3.0e38):
        raise ValueError("out_of_range_regularize must be a finite number >= 0, got %r" % (c,))
    return value


def _options(options, who="chain_loss"):
    """The keyword-only extensions that ``chain_loss`` and its siblings take through ``**options`` -- today one,
    ``out_of_range_regularize`` (default 0.0) -- checked: the penalty's factor as a float.  The pinned part of the signatures
    (the reference's parameters, then ``deriv_weights`` as the one declared keyword-only argument) stays as it is; an
    unknown keyword is the ``TypeError`` a declared signature would raise."""
    c = options.pop("out_of_range_regularize", 0.0)
    if options:
        raise TypeError("%s() got an unexpected keyword argument %r" % (who, next(iter(options))))
    return _out_of_range(c)


ON_FAILURE = ("minibatch", "sequence")


def _failure_options(options):
    """``per_sequence`` and ``on_failure`` taken out of ``**options`` and checked: ``(report, isolate)``.  ``on_failure`` is
    ``"minibatch"`` (the reference's route: one failed sequence fails them all) or ``"sequence"`` (isolation, which implies the
    report); anything else is a ``ValueError``, before any library call."""
    per_sequence = options.pop("per_sequence", False)
    on_failure = options.pop("on_failure", "minibatch")
    if not isinstance(on_failure, str) or on_failure not in ON_FAILURE:
        raise ValueError("on_failure must be 'minibatch' or 'sequence', got %r" % (on_failure,))
    if not isinstance(per_sequence, (bool, int)):
        raise ValueError("per_sequence must be a bool, got %r" % (per_sequence,))
    isolate = on_failure == "sequence"
    return bool(per_sequence) or isolate, isolate


def _xent_options(options, kaldi_way):
    """``xent_log_softmax`` taken out of ``**options`` and checked: a bool (default False).  With ``kaldi_way=False`` the
    whole objective is run again on ``xent_input``, where a log-softmax is another question: that pair is a ``ValueError``, as
    a value that is not a bool is -- before any library call."""
    flag = options.pop("xent_log_softmax", False)
    if not isinstance(flag, bool):
        raise ValueError("xent_log_softmax must be a bool, got %r" % (flag,))
    if flag and not kaldi_way:
        raise ValueError("xent_log_softmax=True needs kaldi_way=True: with kaldi_way=False the objective is run on xent_input")
    return flag


def _boost_options(options, input, supervision, xent_active, kaldi_way):
    """``boost``, ``boost_ref``, ``boost_pdf_class`` and ``boost_accuracy`` taken out of ``**options`` and checked on the host,
    before any library call: None for the call without the option (``boost == 0.0``, or neither reference given), else
    ``(boost, ref, pdf_class, accuracy)`` with exactly one of ``ref`` / ``accuracy``.  Everything else is a ``ValueError``."""
    boost = options.pop("boost", 0.0)
    ref, cls, acc = (options.pop(k, None) for k in ("boost_ref", "boost_pdf_class", "boost_accuracy"))
    try:
        b = float(boost)
    except (TypeError, ValueError):
        raise ValueError("boost must be a finite number, got %r" % (boost,)) from None
    if isinstance(boost, bool) or b != b or b in (float("inf"), float("-inf")) or abs(b) > 3.0e38:
        raise ValueError("boost must be a finite number, got %r" % (boost,))
    if ref is None and cls is None and acc is None:
        return None  # (the call without the option: nothing else is looked at)
    if isinstance(supervision, io.Supervision):
        S, T, P = supervision.n_batch, supervision.n_frame, supervision.n_pdf
    else:  # (a raw handle: its three sizes are plain accessors of the host-side structure)
        S, T, P = (lib.tc_supervision_num_sequence(supervision), lib.tc_supervision_num_frame(supervision),
                   lib.tc_supervision_num_pdf(supervision))
    ints = (torch.int32, torch.int64)

    def tensor(t, name):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a tensor, got %s" % (name, type(t).__name__))
        if t.device != input.device:
            raise ValueError("%s must be on the input's device %s, got %s" % (name, input.device, t.device))

    if ref is not None:
        tensor(ref, "boost_ref")
        if ref.dtype not in ints or tuple(ref.shape) != (S, T):
            raise ValueError("boost_ref must be an int32 or int64 (B, Tmax) = %s tensor, got %s %s" % ((S, T), ref.dtype, tuple(ref.shape)))
    if cls is not None:
        tensor(cls, "boost_pdf_class")
        if cls.dtype not in ints or tuple(cls.shape) != (P,):
            raise ValueError("boost_pdf_class must be an int32 or int64 (P,) = %s tensor, got %s %s" % ((P,), cls.dtype, tuple(cls.shape)))
        if ref is None:
            raise ValueError("boost_pdf_class goes with boost_ref (the dense boost_accuracy has no classes)")
    if acc is not None:
        tensor(acc, "boost_accuracy")
        if acc.dtype != torch.float32 or tuple(acc.shape) != (S * T, P) or acc.stride(1) != 1 or acc.stride(0) < P:
            raise ValueError("boost_accuracy must be a float32 (Tmax*B, C) = %s matrix with unit column stride, got %s %s, strides %s"
                             % ((S * T, P), acc.dtype, tuple(acc.shape), tuple(acc.stride())))
        if acc.requires_grad:
            raise ValueError("boost_accuracy is a constant: a tensor that requires grad is refused (detach it)")
    if b == 0.0 or (ref is None and acc is None):
        return None
    if ref is not None and acc is not None:
        raise ValueError("give exactly one of boost_ref and boost_accuracy")
    if xent_active and not kaldi_way:
        raise ValueError("boost needs kaldi_way=True with the xent branch: with kaldi_way=False the objective is run on xent_input")
    return b, ref, cls, acc


def _penalized(g, y, c):
    """The library's penalised gradient with torch ops in the library's order (``tc_chain_step_penalized``): ``g + t`` where
    ``p != 0`` and ``g`` itself elsewhere, ``t = fl32(2c) * p``, ``p`` the part of ``y`` beyond ``+-OUTPUT_LIMIT`` (0 for NaN and
    ``+-inf``).  Float32 throughout, one multiply and one add: bit for bit what the kernels write."""
    y = y.detach().float()
    zero = torch.zeros_like(y)
    p = torch.where(y > OUTPUT_LIMIT, y - OUTPUT_LIMIT, torch.where(y < -OUTPUT_LIMIT, y + OUTPUT_LIMIT, zero))
    p = torch.where(torch.isinf(y), zero, p)
    t = p * (2.0 * c)  # (the scalar is rounded to float32 first: fl32(2c) * p)
    return torch.where(p != 0, g.float() + t, g.float()).to(g.dtype)


def _rows_of(x):
    """Frame-major rows of an nnet output: T*B for (B, C, T), the number of rows for 2-D."""
    return x.shape[0] * x.shape[2] if x.dim() == 3 else x.shape[0]


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def to2d_hip(x):
    """(B, C, T) -> (T*B, C) in one pass (``tc_to2d``); same values as ``to2d``."""
    B, Cn, T = x.shape
    x = x.contiguous()
    out = torch.empty(T * B, Cn, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.tc_to2d(_ptr(x), B, Cn, T, _ptr(out), out.stride(0), x.device.index, _stream(x.device)), "tc_to2d")
    return out


def from2d_hip(g2d, shape, scale):
    """(T*B, C) -> scale * (B, C, T) in one pass (``tc_from2d``): inverse permutation fused with the
    negation / xent scale of the reference's backward (``functions.py:108-112``)."""
    B, Cn, T = shape
    out = torch.empty(B, Cn, T, dtype=torch.float32, device=g2d.device)
    with torch.cuda.device(g2d.device):
        check(lib.tc_from2d(_ptr(g2d), g2d.stride(0), B, Cn, T, float(scale), _ptr(out), g2d.device.index,
                            _stream(g2d.device)), "tc_from2d")
    return out


class _ChainStep(Function):
    """The whole training-side step behind ONE library call (``tc_chain_step_strided``) -- layout copies, objective, the
    reference's second call for ``kaldi_way=False``, cross-entropy objective, loss value, row weights, penalty, gradients
    in the input's own layout -- and the one autograd class of ``chain_loss``.  The reference's step is one FFI call too
    (``torchain/functions.py:82-86``).  Same values as the step composed from the library's single calls
    (``tests/composed_step.py``)."""

    @staticmethod
    def forward(ctx, input, xent_input, results, den_graph, supervision,
                l2_regularize, leaky_hmm_coefficient, xent_regularize=0.0, kaldi_way=False, deriv_weights=None,
                out_of_range_regularize=0.0, per_sequence=False, isolate=False, xent_log_softmax=False, boost=None):
        out, grad, xgrad = _run_step(input, xent_input, results, den_graph, supervision, l2_regularize,
                                     leaky_hmm_coefficient, xent_regularize, kaldi_way, want_grad=True,
                                     deriv_weights=deriv_weights, out_of_range_regularize=out_of_range_regularize,
                                     per_sequence=per_sequence, isolate=isolate, xent_log_softmax=xent_log_softmax,
                                     boost=boost)
        ctx.grads = (grad, xgrad)
        if results._defer_host_copy:
            return input.new_zeros(1)
        return out[3:4].to(input.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        return (ctx.grads[0], ctx.grads[1]) + (None,) * 13


def _run_step(input, xent_input, results, den_graph, supervision, l2_regularize, leaky_hmm_coefficient,
              xent_regularize, kaldi_way, want_grad, deriv_weights=None, out_of_range_regularize=0.0, per_sequence=False,
              isolate=False, xent_log_softmax=False, boost=None):
    """``boost`` (``_boost_options``, not None): the step through ``tc_chain_step_boosted``, which takes every other option.
    ``per_sequence`` / ``isolate`` (``_failure_options``): the same step through ``tc_chain_step_per_sequence``, which also
    fills the sequences' own values, allocated next to ``out``.  ``xent_log_softmax`` (``_xent_options``) with the xent branch
    active: that step through ``tc_chain_step_log_softmax``, whose workspace also holds the row statistics.  Otherwise:
    One ``tc_chain_step_strided``, in the layout ``classify_layout`` finds (a time-major view as the 2-D rows it is;
    gradients of channel-last views come back as views of dense tensors).  ``want_grad=False`` is the evaluation step
    (``grad == NULL``): forward recursions only, no gradient tensors -- [K] ``ComputeChainObjfAndDeriv`` with ``nnet_output_deriv == NULL``; ``deriv_weights``
    (checked by ``_deriv_weights``) are then not passed on, and ``out_of_range_regularize`` (checked by ``_out_of_range``)
    has nothing to act on."""
    device = input.device
    use_xent = xent_input is not None and xent_regularize != 0.0
    x = input.detach()
    xe = xent_input.detach() if use_xent else None
    plan = _step_plan(x, xe)  # (before any library call: what is refused has touched nothing)
    if plan is None:
        raise ValueError("input and xent_input must be CUDA tensors of one dtype (float32, bfloat16 or float16) in one layout the "
                         "step takes, with the same strides: got %s, and %s" % (_describe(x), _describe(xe)))
    kind, s0, s1 = plan
    dtype = _STEP_DTYPES[x.dtype]
    if isinstance(den_graph, io.DenominatorGraph):
        den_graph.prepare(device)
    den_ptr = den_graph.ptr if isinstance(den_graph, io.DenominatorGraph) else den_graph
    if isinstance(supervision, io.Supervision):
        sup_ptr, S, T, P = supervision.ptr, supervision.n_batch, supervision.n_frame, supervision.n_pdf
    else:
        sup_ptr = supervision
        S, T, P = (lib.tc_supervision_num_sequence(sup_ptr), lib.tc_supervision_num_frame(sup_ptr),
                   lib.tc_supervision_num_pdf(sup_ptr))
    want = (S, P, T) if input.dim() == 3 else (S * T, P)
    if tuple(input.shape) != want or (use_xent and tuple(xent_input.shape) != want):
        raise ValueError("nnet output of shape %s does not match the supervision (%s expected)" % (tuple(input.shape), want))
    if kind == "time_major":  # the 2-D layout where it lies: row t*S + s at (t*S + s) * s0
        x = x.as_strided((S * T, P), (s0, 1))
        xe = xe.as_strided((S * T, P), (s0, 1)) if xe is not None else None
    layout = {"rows": TC_LAYOUT_ROWS, "time_major": TC_LAYOUT_ROWS, "bct": TC_LAYOUT_BCT}.get(kind, TC_LAYOUT_CHANNEL_LAST)
    row_stride = s0 if layout == TC_LAYOUT_ROWS else 0
    # (gradients: contiguous in the 2-D and the (B, C, T) layout; dense (B, T, C) for a channel-last view)
    gshape = {TC_LAYOUT_ROWS: (S * T, P), TC_LAYOUT_BCT: (S, P, T), TC_LAYOUT_CHANNEL_LAST: (S, T, P)}[layout]
    grad = torch.empty(gshape, dtype=x.dtype, device=device) if want_grad else None
    xgrad = torch.empty(gshape, dtype=x.dtype, device=device) if use_xent and want_grad else None
    with torch.cuda.device(device):
        cur = torch.cuda.current_stream(device)
        log_softmax = bool(xent_log_softmax) and use_xent  # (without the xent branch the option does nothing)
        key = (S, T, layout != TC_LAYOUT_ROWS, use_xent, dtype)  # (a channel-last step has the (B, C, T) step's workspace)
        if log_softmax:
            key += ("log_softmax",)
        if boost is not None:
            key += ("boost",)
        sizes = den_graph.__dict__.setdefault("_step_bytes", {}) if isinstance(den_graph, io.DenominatorGraph) else {}
        nbytes = sizes.get(key)
        if nbytes is None:
            sizer = lib.tc_chain_step_log_softmax_workspace_bytes if log_softmax else lib.tc_chain_step_strided_workspace_bytes
            if boost is not None:
                sizer = lib.tc_chain_step_boosted_workspace_bytes
            nbytes = sizer(den_ptr, S, T, layout, int(use_xent), dtype)
            if nbytes < 0:
                check(int(nbytes), "tc_chain_step_boosted_workspace_bytes" if boost is not None else
                      "tc_chain_step_log_softmax_workspace_bytes" if log_softmax else "tc_chain_step_strided_workspace_bytes")
            sizes[key] = nbytes
        capturing = torch.cuda.is_current_stream_capturing()
        # (inside a graph capture the workspace comes from the graph's own pool and lives as long as the graph does)
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device) if capturing else _workspace(device, cur.cuda_stream, nbytes)
        # (a CPU vector is copied here; a float32 CUDA vector is read where it lies, so a replay reads its current values)
        w = _weights_on(deriv_weights, device) if want_grad else None
        out = torch.empty(6, dtype=torch.float32, device=device)  # objf, l2_term, weight | loss | xent objective (f64)
        cl = layout == TC_LAYOUT_CHANNEL_LAST
        args = (den_ptr, sup_ptr, _ptr(x), _ptr(xe), layout, row_stride, s0 if cl else 0, s1 if cl else 0, float(l2_regularize),
                float(leaky_hmm_coefficient), float(xent_regularize), int(bool(kaldi_way)), _ptr(grad), _ptr(xgrad),
                C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 12),
                C.c_void_p(out.data_ptr() + 16) if use_xent else None)
        tail = (_ptr(ws), ws.numel(), device.index, C.c_void_p(cur.cuda_stream))
        # (float32, NULL weights and no penalty: tc_chain_step itself; bfloat16 / float16 are widened on the way in and
        # their gradients rounded once on the way out)
        seq = None
        if per_sequence or isolate:
            seq = torch.empty((S, 6), dtype=torch.float64, device=device)
        keeps = ()
        if boost is not None:
            # (read where they lie; an int64 or strided reference is cast / packed by a device op in front of the call)
            b, ref, cls, acc = boost
            ref = ref.detach().to(torch.int32).contiguous() if ref is not None else None
            cls = cls.detach().to(torch.int32).contiguous() if cls is not None else None
            keeps = (ref, cls, acc)
            check(lib.tc_chain_step_boosted(*args, _ptr(w), float(out_of_range_regularize), dtype, *tail, int(bool(isolate)),
                                            _ptr(seq), int(log_softmax), b, _ptr(ref), _ptr(cls), _ptr(acc),
                                            acc.stride(0) if acc is not None else 0), "tc_chain_step_boosted")
        elif log_softmax:
            check(lib.tc_chain_step_log_softmax(*args, _ptr(w), float(out_of_range_regularize), dtype, *tail, int(bool(isolate)),
                                                _ptr(seq), 1), "tc_chain_step_log_softmax")
        elif per_sequence or isolate:
            check(lib.tc_chain_step_per_sequence(*args, _ptr(w), float(out_of_range_regularize), dtype, *tail, int(bool(isolate)),
                                                 _ptr(seq)), "tc_chain_step_per_sequence")
        else:
            check(lib.tc_chain_step_strided(*args, _ptr(w), float(out_of_range_regularize), dtype, *tail),
                  "tc_chain_step_strided")
        results._dev = out[:3]
        results._stale = True
        results._ready = None
        if capturing:
            results._graph_keeps = (ws, w) + keeps  # replays write through it; read the values after a replay with ``invalidate()``
        else:
            results._ready = torch.cuda.Event()
            results._ready.record(cur)
        results._seq_dev, results._seq_ready, results._seq_host = seq, results._ready, None
        if seq is not None:
            results._seq_weight = (supervision.weight if isinstance(supervision, io.Supervision)
                                   else float(lib.tc_supervision_weight(sup_ptr)))
        if use_xent:
            results._xent_dev = out[4:6].view(torch.float64)
            results._xent_ready = results._ready
            results._xent_scale = 1.0 / -float(xent_regularize)  # (the library's sum is of the scaled gradient, both layouts)
            results._xent_host = None
    if want_grad and kind == "time_major":  # (T*S, C) rows back in the shape of the view they answer
        grad = grad.view(T, S, P).permute(1, 2, 0)
        xgrad = xgrad.view(T, S, P).permute(1, 2, 0) if xgrad is not None else None
    elif want_grad and layout == TC_LAYOUT_CHANNEL_LAST:
        grad = grad.transpose(1, 2)
        xgrad = xgrad.transpose(1, 2) if xgrad is not None else None
    return out, grad, xgrad


_OTHER = ("other", 0, 0)


def classify_layout(shape, strides):
    """Host only: the layout of a network output of ``shape`` with element ``strides`` (sequences of ints: works for CPU
    tensors, numpy shapes, anything), as ``(kind, s0, s1)``:

    * ``("rows", row_stride, 0)``: 2-D frame-major ``(T*B, C)`` with unit column stride and ``row_stride >= C``.
    * ``("bct", 0, 0)``: contiguous ``(B, C, T)`` -- checked first among the 3-D cases, so it is always this.
    * ``("time_major", row_stride, 0)``: a ``(B, C, T)`` view with channel stride 1 whose rows ``t*B + b`` lie at
      ``(t*B + b) * row_stride``: ``(T, B, C).permute(1, 2, 0)`` and its last-dimension slices.  It is the 2-D layout.
    * ``("channel_last", batch_stride, frame_stride)``: any other ``(B, C, T)`` view with channel stride 1, element
      ``(b, c, t)`` at ``b*batch_stride + t*frame_stride + c``, whose rows do not overlap (``tc_chain_step_strided``'s
      rule): ``(B, T, C).transpose(1, 2)``, its slices along any dimension.
    * ``("other", 0, 0)``: everything else -- a channel stride that is not 1, zero or negative strides, overlapping rows
      (``expand``), other ranks, empty tensors.

    The stride of a dimension of size 1 is ignored."""
    shape, strides = tuple(int(n) for n in shape), tuple(int(n) for n in strides)
    if len(shape) != len(strides) or any(n <= 0 for n in shape):
        return _OTHER
    if len(shape) == 2:
        return ("rows", strides[0], 0) if strides[1] == 1 and strides[0] >= shape[1] else _OTHER
    if len(shape) != 3:
        return _OTHER
    B, Cn, T = shape
    sb, sc, st = strides
    if (T == 1 or st == 1) and (Cn == 1 or sc == T) and (B == 1 or sb == Cn * T):
        return ("bct", 0, 0)
    if Cn > 1 and sc != 1:
        return _OTHER
    if (B > 1 and sb < Cn) or (T > 1 and st < Cn):
        return _OTHER
    if B == 1 or T == 1:  # one run of rows: 2-D whatever the other stride says
        return ("time_major", Cn if B == T else (st if B == 1 else sb), 0)
    if st == B * sb:
        return ("time_major", sb, 0)
    if sb >= (T - 1) * st + Cn or st >= (B - 1) * sb + Cn:
        return ("channel_last", sb, st)
    return _OTHER


def _layout(x):
    return classify_layout(x.shape, x.stride())


def pair_layout(a, b=None):
    """Host only: the layout ``(kind, s0, s1)`` in which two network outputs go to the one call together, or None when they do
    not.  ``a``, ``b``: ``(shape, strides)``; ``b`` None for a step without ``xent_input``.  Together go 2-D rows with one row
    stride, two contiguous (B, C, T) tensors, and two time-major or two channel-last views of one shape with the same strides
    (a joint head split in two).  The stride of a dimension of size 1 means nothing and counts as the contiguous one."""
    def layout(shape, strides):
        dense = _contiguous_strides(shape)
        return classify_layout(shape, [d if n == 1 else s for n, s, d in zip(shape, strides, dense)])
    la = layout(*a)
    if la == _OTHER or b is None:
        return None if la == _OTHER else la
    if layout(*b) != la:
        return None
    if la[0] in ("time_major", "channel_last") and tuple(b[0]) != tuple(a[0]):
        return None
    return la


def _contiguous_strides(shape):
    strides, n = [], 1
    for size in reversed(shape):
        strides.insert(0, n)
        n *= size
    return tuple(strides)


def _dense(shape, strides, ordered=False):
    """Whether the elements fill one block of memory without gaps or overlap (then ``.float()`` keeps the strides); ``ordered``:
    in C order as well, which is ``is_contiguous()``.  The stride of a dimension of size 1 is ignored, as torch ignores it."""
    dims = [(st, n) for n, st in zip(shape, strides) if n != 1]
    want = 1
    for st, n in (reversed(dims) if ordered else sorted(dims)):
        if st != want:
            return False
        want *= n
    return all(n > 0 for n in shape)


def plan_step_inputs(a, b=None, want_grad=True):
    """Host only, a pure function of shapes, strides and dtypes: what to do with any ``(input, xent_input)`` pair so that the
    one call takes it.  ``a``, ``b``: ``(shape, strides, dtype)``, ``b`` None without ``xent_input``.  Returns ``(ops_a, ops_b,
    layout)``: per tensor the operations to apply in order -- ``"float"``, ``"contiguous"``, ``"to2d"`` -- and the layout
    (``pair_layout``) in which the pair then goes.  The rules:

    * different dtypes: the 16-bit one(s) are up-cast to float32 (correct, not the fast path).  A dtype the step does not take
      is a ``ValueError`` when a gradient is wanted and is up-cast otherwise.  (A view that is not dense is made contiguous in
      front of the cast, so that the strides behind it are known here.)
    * a pair that goes together already (``pair_layout``) stays as it is;
    * (B, C, T) with 2-D: ``to2d`` on the 3-D tensor;
    * after that, a pair that still does not go together -- 2-D rows with different row strides, channel-last views with
      different strides, a channel stride that is not 1 -- has every tensor that is not contiguous made so.

    Every pair leaves as 2-D rows with one row stride, two contiguous (B, C, T) tensors, a time-major pair or a channel-last
    pair with the same strides; what cannot (other ranks, empty tensors) is a ``ValueError``."""
    specs = [s for s in (a, b) if s is not None]
    geo = [(tuple(s[0]), tuple(s[1])) for s in specs]
    dtypes = [s[2] for s in specs]
    ops = [[] for _ in specs]
    if any(len(shape) not in (2, 3) for shape, _ in geo):
        raise ValueError("chain_loss takes (B, C, T) or (T*B, C) tensors, got shapes %s" % ([g[0] for g in geo],))
    if want_grad and any(d not in _STEP_DTYPES for d in dtypes):
        raise ValueError("chain_loss takes float32, bfloat16 or float16 tensors, got %s" % (dtypes,))

    def do(i, op):
        shape, strides = geo[i]
        if op == "to2d":
            shape = (shape[2] * shape[0], shape[1])
        geo[i] = (shape, strides if op == "float" else _contiguous_strides(shape))
        ops[i].append(op)

    for i, d in enumerate(dtypes):
        if d not in _STEP_DTYPES or (len(set(dtypes)) > 1 and d in _HALF):
            if not _dense(*geo[i]):
                do(i, "contiguous")
            do(i, "float")
    if len(geo) == 2 and len(geo[0][0]) != len(geo[1][0]):
        do(0 if len(geo[0][0]) == 3 else 1, "to2d")
    if pair_layout(*geo) is None:
        for i, g in enumerate(geo):
            if not _dense(*g, ordered=True):
                do(i, "contiguous")
    layout = pair_layout(*geo)
    if layout is None:
        raise ValueError("chain_loss cannot take tensors of shapes %s" % ([g[0] for g in geo],))
    return tuple(ops[0]), tuple(ops[1]) if b is not None else (), layout


def to2d(x):
    if x.dim() == 3:  # (B, C, T)
        n_pdf = x.shape[1]
        x = x.permute(2, 0, 1).contiguous().view(-1, n_pdf)  # (T * B, C)
    assert x.dim() == 2
    return x


_OPS = {"float": torch.Tensor.float, "contiguous": torch.Tensor.contiguous, "to2d": to2d}


def _spec(x):
    return None if x is None else (tuple(x.shape), tuple(x.stride()), x.dtype)


def _describe(x):
    return "None" if x is None else "%s %s, shape %s, strides %s" % (x.device.type, x.dtype, tuple(x.shape), tuple(x.stride()))


def _step_plan(input, xent_input):
    """The layout ``(kind, s0, s1)`` in which ``input`` and ``xent_input`` go to the one call as they are, or None when they
    do not: CUDA tensors of one dtype the step takes, in a layout they share (``pair_layout``).  What ``plan_step_inputs``
    produces, and all that ``_run_step`` accepts."""
    for t in (input, xent_input):
        if t is not None and not (t.is_cuda and t.dtype in _STEP_DTYPES and t.dtype == input.dtype):
            return None
    return pair_layout(_spec(input)[:2], _spec(xent_input)[:2] if xent_input is not None else None)


def _one_call(x):
    """One tensor the step takes in the reference's own two layouts (``rows`` or ``bct``), which is what the registered operator
    accepts: CUDA, a dtype of ``_STEP_DTYPES``, (B, C, T) contiguous or 2-D with unit column stride."""
    return x is None or (_step_view(x) and _layout(x)[0] in ("rows", "bct"))


def _step_view(x):
    """... or in any layout ``tc_chain_step_strided`` takes as it is: those two, or a channel-last view of a (B, C, T) shape."""
    return x is None or (x.is_cuda and x.dtype in _STEP_DTYPES and _layout(x) != _OTHER)


def _needs_grad(input, xent_input):
    if not torch.is_grad_enabled():
        return False
    return input.requires_grad or (xent_input is not None and xent_input.requires_grad)


def _step_inputs(input, xent_input, want_grad):
    """``plan_step_inputs`` applied: the pair as the one call takes it.  The operations are tracked by autograd when a gradient
    is wanted (the gradients flow back through them) and applied to detached tensors otherwise."""
    assert input.is_cuda and (xent_input is None or xent_input.is_cuda), "Only CUDA implementation is available"
    if not want_grad:
        input, xent_input = input.detach(), (xent_input.detach() if xent_input is not None else None)
    ops, xent_ops, _ = plan_step_inputs(_spec(input), _spec(xent_input), want_grad)
    for op in ops:
        input = _OPS[op](input)
    for op in xent_ops:
        xent_input = _OPS[op](xent_input)
    return input, xent_input


def chain_loss(input, den_graph, supervision,
               l2_regularize=0.0, leaky_hmm_coefficient=1e-5,
               xent_regularize=0.0, xent_input=None, kaldi_way=False, *, deriv_weights=None, **options):
    """``options``, keyword-only (the module docstring): ``out_of_range_regularize=0.0`` (``_options``), ``per_sequence=False``
    and ``on_failure="minibatch"`` (``_failure_options``), ``xent_log_softmax=False`` (``_xent_options``), ``boost=0.0``,
    ``boost_ref=None``, ``boost_pdf_class=None`` and ``boost_accuracy=None`` (``_boost_options``)."""
    per_sequence, isolate = _failure_options(options)
    log_softmax = _xent_options(options, kaldi_way)
    boost = _boost_options(options, input, supervision, xent_input is not None and xent_regularize != 0.0, kaldi_way)
    return _chain_loss_into(ChainResults(), input, den_graph, supervision, l2_regularize, leaky_hmm_coefficient,
                            xent_regularize, xent_input, kaldi_way, deriv_weights, _options(options), per_sequence, isolate,
                            log_softmax, boost)


# What introspection reports stays the reference's signature (torchain/functions.py:128-130), the drop-in surface callers
# compare against; ``deriv_weights`` (``chain_loss.__kwdefaults__``) and ``out_of_range_regularize`` (through ``**options``)
# are this library's keyword-only extensions.
chain_loss.__signature__ = inspect.signature(chain_loss).replace(
    parameters=[p for p in inspect.signature(chain_loss).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD])


def _chain_loss_into(results, input, den_graph, supervision, l2_regularize, leaky_hmm_coefficient, xent_regularize,
                     xent_input, kaldi_way, deriv_weights=None, out_of_range_regularize=0.0, per_sequence=False, isolate=False,
                     xent_log_softmax=False, boost=None):
    """``chain_loss`` with the ``ChainResults`` given (parallel.chain_loss_data_parallel passes one that defers the
    host copy of the three floats until after its all-reduce): check the options, plan, one call."""
    deriv_weights = _deriv_weights(deriv_weights, _rows_of(input))
    c = _out_of_range(out_of_range_regularize)
    want_grad = _needs_grad(input, xent_input)
    x, xe = _step_inputs(input, xent_input, want_grad)
    if want_grad:
        loss = _ChainStep.apply(x, xe, results, den_graph, supervision, l2_regularize, leaky_hmm_coefficient, xent_regularize,
                                kaldi_way, deriv_weights, c, per_sequence, isolate, xent_log_softmax, boost)
        return loss, results
    # Evaluation (the recipe's validation loop runs under torch.no_grad(), example/chime5/train.py:150-171): the forward
    # recursions only; deriv_weights and the penalty are checked above and not used.  The reference has no such check
    # (functions.py:74,82) and pays for a training step.
    out, _, _ = _run_step(x, xe, results, den_graph, supervision, l2_regularize, leaky_hmm_coefficient, xent_regularize,
                          kaldi_way, want_grad=False, per_sequence=per_sequence, isolate=isolate,
                          xent_log_softmax=xent_log_softmax, boost=boost)
    # (the loss of an up-cast dtype the step does not take keeps that dtype)
    like = x if input.dtype in _STEP_DTYPES else input
    return (like.new_zeros(1) if results._defer_host_copy else out[3:4].to(like.dtype)), results


_ChainLoss = _ChainStep  # (the name the reference's module exports, torchain/functions.py)


def best_path(input, supervision):
    """The frame-level pdf alignment of ``supervision`` under ``input``, in the style of ``chain_loss``: ``(pdfs, scores)``,
    int32 ``(B, Tmax)`` (``-1`` in padding frames) and float64 ``(B,)``, on the input's device
    (``io.Supervision.best_path``, ``tc_supervision_best_path``).  ``input`` is what ``chain_loss`` takes; 2-D float32 and
    dense ``(B, C, T)`` float32 / bfloat16 / float16 go to the kernel as they are, any other view through ``.contiguous()``
    -- this is not a hot path.  Autograd is not involved."""
    if not isinstance(supervision, io.Supervision):
        raise TypeError("best_path takes an io.Supervision, got %s" % type(supervision).__name__)
    with torch.no_grad():
        return supervision.best_path(input)


def den_best_path(input, den_graph, frames=None, return_states=False, max_workspace_bytes=1 << 30, workspace=None, out=None,
                  n_batch=None):
    """The single strongest path through ``den_graph`` under ``input`` -- a free decoding constrained by the phone LM alone --
    in the style of ``best_path``: ``(pdfs, scores)``, int32 ``(B, Tmax)`` (``-1`` in padding frames) and float64 ``(B,)``,
    and with ``return_states`` the FST's states, int32 ``(B, Tmax + 1)`` (``io.DenominatorGraph.best_path``,
    ``tc_den_best_path``).  ``input`` is a dense ``(B, C, T)`` float32 / bfloat16 / float16 tensor or 2-D float32 (then
    ``frames`` or ``n_batch`` tells ``B``); ``frames`` the sequences' lengths, ``Supervision.frames`` of a ragged handle as it
    is.  Autograd is not involved."""
    if not isinstance(den_graph, io.DenominatorGraph):
        raise TypeError("den_best_path takes an io.DenominatorGraph, got %s" % type(den_graph).__name__)
    with torch.no_grad():
        return den_graph.best_path(input, frames=frames, return_states=return_states, max_workspace_bytes=max_workspace_bytes,
                                   workspace=workspace, out=out, n_batch=n_batch)


class _DenExpectedAccuracy(torch.autograd.Function):
    """``den_expected_accuracy``: forward is one ``tc_den_expected_accuracy`` call, backward one
    ``tc_den_expected_accuracy_grad`` call with ``grad_output`` as the sequences' scales."""

    @staticmethod
    def forward(ctx, input, den_graph, ref_pdfs, pdf_class, frames, leaky_hmm_coefficient, n_batch, max_workspace_bytes,
                want_grad):
        st = den_graph._expected_accuracy("den_expected_accuracy", input, ref_pdfs, pdf_class, frames, leaky_hmm_coefficient,
                                          n_batch, max_workspace_bytes, want_grad)
        if want_grad:
            # (without the output itself: it points back here through its grad_fn)
            ctx.den_graph, ctx.like = den_graph, (input.dim(), input.dtype)
            ctx.st = {k: v for k, v in st.items() if k != "acc"}
        return st["acc"]

    @staticmethod
    def backward(ctx, grad_output):
        st = ctx.st
        scale = grad_output.detach().to(device=st["y2d"].device, dtype=torch.float32).contiguous()
        grad = ctx.den_graph._expected_accuracy_grad(st, scale)
        dim, dtype = ctx.like
        if dim == 3:  # (T*B, C) rows t*B + b -> (B, C, T); not a hot path
            grad = grad.view(st["T"], st["B"], -1).permute(1, 2, 0).contiguous()
        return (grad.to(dtype),) + (None,) * 8


def den_expected_accuracy(input, den_graph, ref_pdfs, pdf_class=None, frames=None, leaky_hmm_coefficient=1e-5, n_batch=None,
                          max_workspace_bytes=8 << 30):
    """The expected frame accuracy of ``den_graph``'s paths under ``input`` against the frame-level reference ``ref_pdfs``,
    float64 ``(B,)``, differentiable in ``input``: the lattice-free sMBR criterion (``io.DenominatorGraph.expected_accuracy``
    states it and the arguments; ``tc_den_expected_accuracy``, ``tc_den_expected_accuracy_grad``).  Maximise
    ``den_expected_accuracy(...).sum()``: the criterion is an accuracy, not a loss.  ``ref_pdfs`` is what ``best_path`` returns
    for the supervision, ``pdf_class`` a pdf -> phone map for an MPFE-style criterion.

    The forward pass is one denominator forward-backward and a row kernel, and nothing else runs under ``no_grad``.  The
    backward pass is one launch of the accuracy-carrying forward-backward and, unlike ``chain_loss``, honours ``grad_output``:
    sequence ``b``'s rows are ``grad_output[b] * dE_b/dinput``.  The gradient has the input's shape and dtype (computed in
    float32, rounded once); padding frames and a sequence with a NaN or an infinity in its valid frames get +0.  Both passes'
    workspaces are held against ``max_workspace_bytes`` before anything runs (``ValueError``); groups are not run."""
    if not isinstance(den_graph, io.DenominatorGraph):
        raise TypeError("den_expected_accuracy takes an io.DenominatorGraph, got %s" % type(den_graph).__name__)
    # (inside forward the grad mode is off whatever the caller's: what a backward pass will need is decided here)
    want_grad = torch.is_grad_enabled() and isinstance(input, torch.Tensor) and input.requires_grad
    return _DenExpectedAccuracy.apply(input, den_graph, ref_pdfs, pdf_class, frames, leaky_hmm_coefficient, n_batch,
                                      max_workspace_bytes, want_grad)


class _DenExpectedAccuracyDense(torch.autograd.Function):
    """``den_expected_accuracy_dense``: forward is ``tc_den_expected_accuracy_dense``; backward in ``input`` is
    ``tc_den_expected_accuracy_dense_grad`` with ``grad_output`` as the sequences' scales, backward in ``accuracy`` is
    ``grad_output`` times the denominator posteriors the forward call left."""

    @staticmethod
    def forward(ctx, input, accuracy, den_graph, frames, leaky_hmm_coefficient, n_batch, max_workspace_bytes, want_input,
                want_accuracy):
        st = den_graph._expected_accuracy_dense("den_expected_accuracy_dense", input, accuracy, frames, leaky_hmm_coefficient,
                                                n_batch, max_workspace_bytes, want_input, want_accuracy)
        ctx.want = (want_input, want_accuracy)
        if want_input or want_accuracy:
            # (without the output itself: it points back here through its grad_fn; what neither gradient reads is dropped)
            ctx.den_graph = den_graph
            ctx.like = (input.dim(), input.dtype, accuracy.dim(), accuracy.dtype)
            keep = {"frame_acc", "y2d", "a2d", "fr", "B", "T", "leaky", "group"} if want_input else {"fr", "B", "T"}
            ctx.st = {k: v for k, v in st.items() if k in keep or (k == "gamma" and want_accuracy)}
            ctx.failed = torch.isnan(st["acc"]) if want_accuracy else None
        return st["acc"]

    @staticmethod
    def backward(ctx, grad_output):
        st, (want_input, want_accuracy) = ctx.st, ctx.want
        B, T = st["B"], st["T"]
        in_dim, in_dtype, acc_dim, acc_dtype = ctx.like
        scale = grad_output.detach().to(dtype=torch.float32).contiguous()

        def shaped(g2d, dim, dtype):  # (T*B, C) rows t*B + b -> (B, C, T); not a hot path
            if dim == 3:
                g2d = g2d.view(T, B, -1).permute(1, 2, 0).contiguous()
            return g2d.to(dtype)

        grad_input = grad_accuracy = None
        if want_input and ctx.needs_input_grad[0]:
            grad_input = shaped(ctx.den_graph._expected_accuracy_dense_grad(st, scale), in_dim, in_dtype)
        if want_accuracy and ctx.needs_input_grad[1]:
            gamma = st["gamma"].view(T, B, -1)
            # +0 -- not grad_output * 0, which has grad_output's sign -- in padding rows and in every row of a failed sequence
            valid = ~ctx.failed.view(1, B)
            if st["fr"] is not None:
                valid = valid & (torch.arange(T, device=gamma.device).view(T, 1) < st["fr"].view(1, B))
            g = torch.where(valid.unsqueeze(2), gamma * scale.view(1, B, 1), gamma.new_zeros(()))
            grad_accuracy = shaped(g.view(T * B, -1), acc_dim, acc_dtype)
        return (grad_input, grad_accuracy) + (None,) * 7


def den_expected_accuracy_dense(input, den_graph, accuracy, frames=None, leaky_hmm_coefficient=1e-5, n_batch=None,
                                max_workspace_bytes=8 << 30):
    """Lattice-free sMBR against SOFT references: the expected accuracy of ``den_graph``'s paths under ``input`` where a path
    scores ``accuracy[t, pdf_t(path)]`` in frame ``t``, float64 ``(B,)``, differentiable in ``input`` and in ``accuracy``
    (``io.DenominatorGraph.expected_accuracy_dense`` states it and the arguments; ``tc_den_expected_accuracy_dense``,
    ``tc_den_expected_accuracy_dense_grad``).  Kaldi's chain-sMBR recipe is

        acc = den_expected_accuracy_dense(out, graph, num_posteriors(out, supervision))

    with the numerator's posteriors as a constant.  Maximise ``acc.sum()``: an accuracy, not a loss.

    The gradient in ``input`` is one launch of the accuracy-carrying forward-backward per group of sequences, sequence ``b``'s
    rows times ``grad_output[b]``, in the input's shape and dtype (float32 arithmetic, rounded once); it runs only when
    ``input`` requires a gradient.  The gradient in ``accuracy`` is ``grad_output[b] * gamma_den``, the denominator posteriors
    of the forward pass, in ``accuracy``'s shape and dtype; they are kept only when ``accuracy`` requires a gradient.  Padding
    rows and every row of a sequence with a NaN or an infinity in its valid frames of either argument are exactly +0 in both.
    Under ``no_grad`` only the value runs.  Beyond ``max_workspace_bytes`` consecutive groups of sequences run, with the
    single call's bits; ``ValueError`` only where one sequence alone does not fit."""
    if not isinstance(den_graph, io.DenominatorGraph):
        raise TypeError("den_expected_accuracy_dense takes an io.DenominatorGraph, got %s" % type(den_graph).__name__)
    # (inside forward the grad mode is off whatever the caller's: what a backward pass will need is decided here)
    on = torch.is_grad_enabled()
    want_input = on and isinstance(input, torch.Tensor) and input.requires_grad
    want_accuracy = on and isinstance(accuracy, torch.Tensor) and accuracy.requires_grad
    return _DenExpectedAccuracyDense.apply(input, accuracy, den_graph, frames, leaky_hmm_coefficient, n_batch,
                                           max_workspace_bytes, want_input, want_accuracy)


def den_sample_paths(input, den_graph, num_samples, frames=None, leaky_hmm_coefficient=1e-5, generator=None, uniforms=None,
                     return_states=False, max_workspace_bytes=1 << 30, workspace=None, n_batch=None):
    """``num_samples`` paths a sequence drawn from ``den_graph``'s path posterior under ``input`` -- the denominator's own
    model, leaky-HMM transitions included -- int32 ``(B, K, Tmax)`` (``-1`` in padding frames and for a failed sequence), and
    with ``return_states`` the FST's states, int32 ``(B, K, Tmax + 1, 2)`` (``io.DenominatorGraph.sample_paths`` states the
    arguments; ``tc_den_sample_paths``).  The random numbers come from ``generator`` or are given as ``uniforms``.  Autograd
    is not involved: ``sampled_risk_surrogate`` makes a gradient of the samples."""
    if not isinstance(den_graph, io.DenominatorGraph):
        raise TypeError("den_sample_paths takes an io.DenominatorGraph, got %s" % type(den_graph).__name__)
    with torch.no_grad():
        return den_graph.sample_paths(input, num_samples, frames=frames, leaky_hmm_coefficient=leaky_hmm_coefficient,
                                      generator=generator, uniforms=uniforms, return_states=return_states,
                                      max_workspace_bytes=max_workspace_bytes, workspace=workspace, n_batch=n_batch)


def _int_vector(who, name, v, n, device, dtype=torch.int32):
    """``v`` as a contiguous ``(n,)`` tensor of ``dtype`` on ``device`` (a tensor already there is not brought to the host)."""
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(v)
    if t.dim() != 1 or int(t.shape[0]) != n or t.is_floating_point() or t.is_complex():
        raise ValueError("%s: %s must be %d integers, got shape %s of %s" % (who, name, n, tuple(t.shape), t.dtype))
    return t.detach().to(device=device, dtype=dtype).contiguous()


def _path_edit(who, pdfs, token_of_pdf, refs, ref_lengths, starts, frames, want_tokens):
    if not isinstance(pdfs, torch.Tensor) or pdfs.dim() not in (2, 3) or pdfs.dtype not in (torch.int32, torch.int64):
        raise ValueError("%s: pdfs must be an int32 or int64 tensor (B, K, Tmax) or (B, Tmax)" % who)
    squeeze = pdfs.dim() == 2
    p3 = pdfs.detach().unsqueeze(1) if squeeze else pdfs.detach()
    B, K, T = (int(v) for v in p3.shape)
    if B < 1 or K < 1 or T < 1:
        raise ValueError("%s: pdfs of shape %s have an empty axis" % (who, tuple(pdfs.shape)))
    device = pdfs.device
    if p3.dtype == torch.int64:  # (a value beyond int32 stays outside 0 .. P - 1)
        p3 = p3.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    p3 = p3.contiguous()
    tok_map = token_of_pdf if isinstance(token_of_pdf, torch.Tensor) else torch.as_tensor(token_of_pdf)
    if tok_map.dim() != 1 or int(tok_map.shape[0]) < 1:
        raise ValueError("%s: token_of_pdf must be a vector of P >= 1 token ids" % who)
    P = int(tok_map.shape[0])
    tok_map = _int_vector(who, "token_of_pdf", tok_map, P, device)
    st = None
    if starts is not None:
        st = starts if isinstance(starts, torch.Tensor) else torch.as_tensor(starts)
        if st.dtype == torch.bool:
            st = st.to(torch.uint8)
        st = _int_vector(who, "starts", st, P, device, torch.uint8)
    fr = None if frames is None else _int_vector(who, "frames", frames, B, device)
    ref = ref_len = None
    max_ref = 0
    if refs is not None:
        r = refs if isinstance(refs, torch.Tensor) else torch.as_tensor(refs)
        if r.dim() != 2 or int(r.shape[0]) != B or r.is_floating_point() or r.is_complex():
            raise ValueError("%s: refs must be (%d, max_ref) integers, got shape %s of %s" % (who, B, tuple(r.shape), r.dtype))
        max_ref = int(r.shape[1])
        if ref_lengths is None:  # (the one route that looks at values on the host)
            neg = (r.detach() < 0).cpu()
            if max_ref and bool((neg[:, :-1] & ~neg[:, 1:]).any()):
                raise ValueError("%s: a reference has a token behind a negative entry; pass ref_lengths for other paddings" % who)
            ref_len = (~neg).sum(dim=1).to(device=device, dtype=torch.int32)
        else:
            ref_len = _int_vector(who, "ref_lengths", ref_lengths, B, device)
        ref = r.detach().to(device=device, dtype=torch.int32).contiguous()
    elif ref_lengths is not None:
        raise ValueError("%s: ref_lengths without refs" % who)
    if max_ref > 4096:
        raise ValueError("%s: references of up to 4096 tokens are supported, got max_ref = %d" % (who, max_ref))
    if not pdfs.is_cuda:
        raise ValueError("%s: pdfs must be on the GPU (there is no CPU path)" % who)
    dist = torch.empty((B, K), dtype=torch.int32, device=device)
    lens = torch.empty((B, K), dtype=torch.int32, device=device)
    tokens = torch.empty((B, K, T), dtype=torch.int32, device=device) if want_tokens else None
    with torch.cuda.device(device):
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        ws = None if want_tokens else torch.empty(int(lib.tc_paths_edit_distance_workspace_bytes(B, K, T)), dtype=torch.uint8,
                                                  device=device)
        check(lib.tc_paths_edit_distance(B, K, _ptr(p3), _ptr(fr), T, _ptr(tok_map), _ptr(st), P,
                                         _ptr(ref) if max_ref else None, _ptr(ref_len) if max_ref else None, max_ref,
                                         _ptr(dist), _ptr(lens), _ptr(tokens), _ptr(ws), 0 if ws is None else ws.numel(),
                                         device.index, stream), "tc_paths_edit_distance")
    if squeeze:
        dist, lens = dist[:, 0], lens[:, 0]
        tokens = None if tokens is None else tokens[:, 0]
    return dist, lens, tokens


def path_edit_distance(pdfs, token_of_pdf, refs, ref_lengths=None, starts=None, frames=None, return_tokens=False):
    """The token sequences of frame-level pdf paths and their edit distances to the references, on the device in one
    launch (``tc_paths_edit_distance``): ``(dist, lengths)``, or with ``return_tokens`` ``(dist, lengths, tokens)``.

    ``pdfs``: int32 or int64 ``(B, K, Tmax)`` -- ``den_sample_paths``' output -- or ``(B, Tmax)`` -- ``den_best_path``'s, the
    outputs then lose the ``K`` axis; on the GPU.  ``token_of_pdf``: ``P`` ints, pdf -> token id, negative for a pdf that
    emits nothing (silence).  With ``c_t = token_of_pdf[pdfs_t]``, frame ``t`` emits ``c_t`` iff ``c_t >= 0`` and

    * ``starts is None`` (collapse): ``t == 0 or c_t != c_{t-1}``, whether or not frame ``t - 1`` emitted, so ``a SIL a``
      gives ``a a`` and ``a a`` gives ``a``;
    * ``starts`` (``P`` flags): ``starts[pdfs_t]`` -- the chain topology's forward pdf of a phone, as opposed to its
      self-loop pdf; this keeps ``a a`` apart.

    ``frames``: ``B`` lengths, ``None`` for ``Tmax`` each; frames beyond a length are not read.  ``refs``: ints ``(B,
    max_ref)``, ``max_ref <= 4096``; ``ref_lengths``: ``B`` ints, or ``None`` for each row's count of leading non-negative
    entries (a non-negative entry behind a negative one is a ``ValueError``).  That count is taken on the host: pass
    ``ref_lengths`` -- and tensors on the device -- and the call makes no host synchronisation; lengths outside their range
    are then clamped, not reported.  ``dist``, int32 ``(B, K)``: the unit-cost Levenshtein distance; ``lengths``: the
    number of tokens; ``tokens``, int32 ``(B, K, Tmax)``: the tokens, then ``-1``.  A path with a pdf outside ``0 .. P - 1``
    in its frames -- ``den_sample_paths``' ``-1`` of a failed sequence -- gets ``-1`` everywhere.  Integer arithmetic: the
    results are exact.  A phone error rate of a free decoding is ``path_edit_distance(den_best_path(out, graph)[0],
    phone_of_pdf, refs)[0].sum() / ref_tokens``.  No autograd."""
    who = "path_edit_distance"
    if refs is None:
        raise ValueError("%s: refs is required (path_tokens gives the tokens alone)" % who)
    if not isinstance(return_tokens, bool):
        raise ValueError("%s: return_tokens must be a bool, got %r" % (who, return_tokens))
    dist, lens, tokens = _path_edit(who, pdfs, token_of_pdf, refs, ref_lengths, starts, frames, return_tokens)
    return (dist, lens, tokens) if return_tokens else (dist, lens)


def path_tokens(pdfs, token_of_pdf, starts=None, frames=None):
    """``(tokens, lengths)`` of frame-level pdf paths: ``path_edit_distance``'s launch without references (``max_ref = 0``),
    with its arguments and its rule."""
    dist, lens, tokens = _path_edit("path_tokens", pdfs, token_of_pdf, None, None, starts, frames, True)
    return tokens, lens


class _SampledRiskFused(Function):
    """``sampled_risk_surrogate(..., fused=True)``: the value by the torch expression, the gradient by one memset and one
    launch of ``tc_sampled_risk_grad``."""

    @staticmethod
    def forward(ctx, input, pdfs, risks, frames):
        who = "sampled_risk_surrogate"
        with torch.no_grad():
            value = sampled_risk_surrogate(input, pdfs, risks, frames)  # (and every check of the arguments)
        if not input.is_cuda:
            raise ValueError("%s: fused=True needs the input on the GPU (there is no CPU path)" % who)
        if input.dtype not in _STEP_DTYPES or (input.dim() == 2 and input.dtype != torch.float32):
            raise ValueError("%s: fused=True takes (B, C, T) float32 / bfloat16 / float16 or 2-D float32, got %s %s"
                             % (who, tuple(input.shape), input.dtype))
        B, K, T = (int(v) for v in pdfs.shape)
        device = input.device
        r = torch.as_tensor(risks).detach().to(device=device, dtype=torch.float64)
        ctx.weight = ((r - r.mean(dim=1, keepdim=True)) / (K - 1)).contiguous()
        ctx.pdfs = pdfs.detach().to(device).clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()
        ctx.frames = None if frames is None else _int_vector(who, "frames", frames, B, device)
        ctx.save_for_backward(input)
        return value

    @staticmethod
    def backward(ctx, grad_output):
        (input,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        B, K, T = (int(v) for v in ctx.pdfs.shape)
        device = input.device
        go = grad_output.detach().to(device=device, dtype=torch.float64).contiguous()
        grad = torch.empty(input.shape, dtype=input.dtype, device=device)
        if input.dim() == 3:
            P = int(input.shape[1])
            in_strides = (input.stride(0), input.stride(1), input.stride(2))
            g_strides = (grad.stride(0), grad.stride(1), grad.stride(2))
        else:
            P = int(input.shape[1])
            in_strides = (input.stride(0), input.stride(1), B * input.stride(0))
            g_strides = (grad.stride(0), grad.stride(1), B * grad.stride(0))
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            check(lib.tc_sampled_risk_grad(B, K, T, P, _ptr(ctx.pdfs), _ptr(ctx.frames), _ptr(ctx.weight), _ptr(go), _ptr(input),
                                           _STEP_DTYPES[input.dtype], in_strides[0], in_strides[1], in_strides[2], _ptr(grad),
                                           g_strides[0], g_strides[1], g_strides[2], grad.numel(), device.index, stream),
                  "tc_sampled_risk_grad")
        return grad, None, None, None


def sampled_risk_surrogate(input, pdfs, risks, frames=None, fused=False):
    """A SURROGATE whose gradient in ``input`` is the unbiased sampling estimate of ``grad E[r(path)]``, the expected risk of
    the denominator graph's paths under ``input`` -- not an estimate of ``E[r]`` itself: its value means nothing.  Float64
    ``(B,)``, plain torch, differentiable in ``input``:

        L_s = 1 / (K - 1) * sum_k (r_sk - mean_k r_sk) * sum_{t < T_s} clamp(input_s,t, +-30)[pdfs_skt]

    ``pdfs``: int ``(B, K, Tmax)``, ``K >= 2`` paths a sequence drawn by ``den_sample_paths`` from the same ``input``;
    ``risks``: ``(B, K)``, any function of each path (held constant).  Why it works: ``grad E[r] = E[(r - b) grad log
    P(path | y)]`` and ``grad log P(path | y) = onehot(pdfs of the path) - gamma_den``; with the risks centred over the
    sequence's own samples the ``gamma_den`` term cancels, and ``1 / (K - 1)`` makes up for the centring.  The clamp is the
    denominator's: an output outside +-30 gets exactly +0, as do padding rows.  A failed sequence (all ``-1``) gives 0.
    ``input`` is ``(B, C, T)`` or 2-D ``(T*B, C)`` (row ``t*B + b``); ``frames``: the sequences' lengths, ``None``: wherever
    ``pdfs >= 0``.  Training on a sequence-level risk, e.g. an edit distance to the transcript, is

        pdfs = den_sample_paths(out, graph, 8, generator=gen)
        risks, _ = path_edit_distance(pdfs, phone_of_pdf, refs, ref_lengths)   # on the device: no copy, no Python loop
        sampled_risk_surrogate(out, pdfs, risks, fused=True).sum().backward()  # minimises the expected edit distance

    ``fused=False`` (the default) leaves the gradient to autograd: a gather's backward, which scatters with atomics into a
    dense gradient.  ``fused=True`` returns the same value through an ``autograd.Function`` whose backward is one memset and
    one launch of ``tc_sampled_risk_grad``: per element the double sum over the samples, in sample order, rounded once to the
    input's dtype -- no atomics, the same bits at every call (autograd's route rounds every sample's term to the input's
    dtype and adds them in an order it does not fix).  It takes ``(B, C, T)`` float32 / bfloat16 / float16 by its strides
    and 2-D float32, on the GPU; anything else is a ``ValueError``, not another route.
    """
    if not isinstance(fused, bool):
        raise ValueError("sampled_risk_surrogate: fused must be a bool, got %r" % (fused,))
    if fused:
        return _SampledRiskFused.apply(input, pdfs, risks, frames)
    if not isinstance(input, torch.Tensor) or input.dim() not in (2, 3) or not input.is_floating_point():
        raise ValueError("sampled_risk_surrogate: input must be a floating-point (B, C, T) or (T*B, C) tensor")
    if not isinstance(pdfs, torch.Tensor) or pdfs.dim() != 3 or pdfs.dtype not in (torch.int32, torch.int64):
        raise ValueError("sampled_risk_surrogate: pdfs must be an int32 or int64 tensor (B, K, Tmax)")
    B, K, T = (int(v) for v in pdfs.shape)
    if K < 2:
        raise ValueError("sampled_risk_surrogate: centring the risks needs K >= 2 samples a sequence, got %d" % K)
    if input.dim() == 3:
        if int(input.shape[0]) != B or int(input.shape[2]) != T:
            raise ValueError("sampled_risk_surrogate: input of shape %s is not (%d, C, %d)" % (tuple(input.shape), B, T))
        rows = input.transpose(1, 2)  # (B, T, C)
    else:
        if int(input.shape[0]) != T * B:
            raise ValueError("sampled_risk_surrogate: input of shape %s is not (%d * %d, C)" % (tuple(input.shape), T, B))
        rows = input.reshape(T, B, -1).transpose(0, 1)
    P = int(rows.shape[2])
    r = torch.as_tensor(risks)
    if tuple(r.shape) != (B, K):
        raise ValueError("sampled_risk_surrogate: risks of shape %s are not (%d, %d)" % (tuple(r.shape), B, K))
    r = r.detach().to(device=input.device, dtype=torch.float64)
    pdfs = pdfs.detach().to(input.device)
    if int(pdfs.max()) >= P:
        raise ValueError("sampled_risk_surrogate: a pdf is outside 0 .. %d" % (P - 1))
    valid = pdfs >= 0
    if frames is not None:
        lengths = torch.as_tensor(frames).detach().to(device=input.device, dtype=torch.int64)
        if tuple(lengths.shape) != (B,) or int(lengths.min()) < 1 or int(lengths.max()) > T:
            raise ValueError("sampled_risk_surrogate: frames must be %d lengths in 1 .. %d" % (B, T))
        valid = valid & (torch.arange(T, device=input.device).view(1, 1, T) < lengths.view(B, 1, 1))
    index = pdfs.clamp(min=0).to(torch.int64).transpose(1, 2)  # (B, T, K)
    picked = rows.gather(2, index).clamp(-30.0, 30.0).to(torch.float64)
    picked = torch.where(valid.transpose(1, 2), picked, picked.new_zeros(()))
    weight = (r - r.mean(dim=1, keepdim=True)) / (K - 1)
    return (picked.sum(dim=1) * weight).sum(dim=1)


def num_posteriors(input, supervision, pdf_class=None):
    """The numerator's occupation posteriors of ``supervision`` under ``input``, dense float32 ``(T*B, C)``
    (``io.Supervision.posteriors``): the soft reference of ``den_expected_accuracy_dense``; with ``pdf_class`` pooled by class
    (MPFE).  A constant, as in Kaldi: no autograd."""
    if not isinstance(supervision, io.Supervision):
        raise TypeError("num_posteriors takes an io.Supervision, got %s" % type(supervision).__name__)
    with torch.no_grad():
        return supervision.posteriors(input, pdf_class=pdf_class)
