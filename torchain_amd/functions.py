"""``chain_loss`` / ``ChainResults``: the autograd wrapper of the reference
(``torchain/functions.py:9-138``) on top of the HIP C ABI.

Same names, argument meaning, defaults and quirks as the reference:

* ``ChainResults.data`` is a CPU float tensor ``[objf, l2_term, weight]``; ``loss = -objf/weight``
  (l2 not included, ``functions.py:19``).
* ``chain_loss`` accepts ``(B, C, T)`` or ``(T*B, C)`` input; 3-D input is permuted to frame-major
  rows ``t*B + b`` (``functions.py:118-125``).  For CUDA float32 3-D inputs the permutation, its inverse
  and the backward's negation / xent scale are single fused passes (``tc_to2d`` / ``tc_from2d``) with
  identical values.
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
  must be a view with the same strides (or absent); any other combination takes the routes it took before.
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


def _device_loss(results, like):
    """-objf / weight as a one-element tensor on the input's device (the reference's ``input.new([results.loss])``,
    functions.py:104) computed from the device-side results: no host round trip."""
    r = results._dev
    return (-(r[0] / r[2])).reshape(1).to(like.dtype)


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


class _ChainLoss(Function):
    """Lattice-free MMI loss; see the reference docstring ``torchain/functions.py:23-60`` for the
    meaning of every argument (identical here).  ``deriv_weights``: per-row factors of both gradients, applied in
    backward (frame-major rows, as the 2-D tensors here)."""

    @staticmethod
    def forward(ctx, input, xent_input, results, den_graph, supervision,
                l2_regularize, leaky_hmm_coefficient, xent_regularize=0.0, kaldi_way=False, deriv_weights=None,
                out_of_range_regularize=0.0):
        assert input.is_cuda, "Only CUDA implementation is available"
        # The kernels write the two matrices as backward() returns them (-deriv, -xent_regularize * xent_deriv):
        # the reference scales one and negates both in three more passes over (T*B, C) tensors.
        mmi_grad = torch.empty_like(input, memory_format=torch.contiguous_format)
        use_xent = xent_input is not None and xent_regularize != 0.0
        xent_grad = torch.empty_like(xent_input, memory_format=torch.contiguous_format) if use_xent else None
        compute_chain_objf_and_deriv(den_graph, supervision, input.detach(), results._host, mmi_grad, xent_grad,
                                     l2_regularize, leaky_hmm_coefficient, xent_regularize, as_gradients=True,
                                     holder=results)
        ctx.mmi_grad = mmi_grad
        if use_xent:
            # sum(xent_output * xent_deriv) from the scaled matrix: the scale is one factor of every term
            results._xent_dev = xent_objective(xent_input.detach(), xent_grad)
            results._xent_ready = torch.cuda.Event()
            results._xent_ready.record(torch.cuda.current_stream(xent_input.device))
            results._xent_scale = 1.0 / -float(xent_regularize)
            results._xent_host = None
            if not kaldi_way:  # the reference's second call (functions.py:96-103)
                compute_chain_objf_and_deriv(den_graph, supervision, xent_input.detach(), results._host, mmi_grad,
                                             xent_grad, l2_regularize, leaky_hmm_coefficient, xent_regularize,
                                             as_gradients=True, holder=results)
            ctx.xent_grad = xent_grad
        ctx.row_w = _weights_on(deriv_weights, input.device)
        ctx.pen = (input.detach(), float(out_of_range_regularize))  # (always the chain output, never xent_input)
        if results._defer_host_copy:
            return input.new_zeros(1)  # (filled in behind the all-reduce: parallel.chain_loss_data_parallel)
        return _device_loss(results, input)

    @staticmethod
    def backward(ctx, grad_output):
        g, xg = ctx.mmi_grad, getattr(ctx, "xent_grad", None)
        if ctx.pen[1] > 0.0:  # (in front of the weights, as tc_chain_step_penalized)
            g = _penalized(g, *ctx.pen)
        if ctx.row_w is not None:  # ([K] MulRowsVec on both derivatives)
            w = ctx.row_w.unsqueeze(1)
            g = g * w.to(g.dtype)
            xg = xg * w.to(xg.dtype) if xg is not None else None
        return (g, xg, None, None, None, None, None, None, None, None, None)


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


class _ChainLoss3d(Function):
    """``_ChainLoss`` for ``(B, C, T)`` inputs with the layout conversions fused in: the
    value and the gradients are those of ``_ChainLoss.apply(to2d(input), ...)`` followed by autograd's
    inverse permute, without the three extra passes over the activation tensor."""

    @staticmethod
    def forward(ctx, input, xent_input, results, den_graph, supervision,
                l2_regularize, leaky_hmm_coefficient, xent_regularize=0.0, kaldi_way=False, deriv_weights=None,
                out_of_range_regularize=0.0):
        assert input.is_cuda, "Only CUDA implementation is available"
        x2d = to2d_hip(input.detach())
        mmi_grad = torch.empty_like(x2d)
        use_xent = xent_input is not None and xent_regularize != 0.0
        xe2d = to2d_hip(xent_input.detach()) if use_xent else None
        xent_grad = torch.empty_like(xe2d) if use_xent else None
        compute_chain_objf_and_deriv(den_graph, supervision, x2d, results._host, mmi_grad, xent_grad,
                                     l2_regularize, leaky_hmm_coefficient, xent_regularize, holder=results)
        if use_xent:
            results._xent_dev = xent_objective(xe2d, xent_grad)
            results._xent_scale = 1.0
            results._xent_host = None
        if use_xent and not kaldi_way:  # the reference's second call (functions.py:96-103)
            compute_chain_objf_and_deriv(den_graph, supervision, xe2d, results._host, mmi_grad, xent_grad,
                                         l2_regularize, leaky_hmm_coefficient, xent_regularize, holder=results)
        ctx.mmi_grad = mmi_grad
        ctx.in_shape = tuple(input.shape)
        if use_xent:
            ctx.xent_grad = xent_grad
            ctx.xent_shape = tuple(xent_input.shape)
            ctx.xent_scale = float(xent_regularize)
        ctx.row_w = _weights_on(deriv_weights, input.device)
        ctx.pen = (input.detach(), float(out_of_range_regularize))
        if results._defer_host_copy:
            return input.new_zeros(1)
        return _device_loss(results, input)

    @staticmethod
    def backward(ctx, grad_output):
        g = from2d_hip(ctx.mmi_grad, ctx.in_shape, -1.0)
        xg = from2d_hip(ctx.xent_grad, ctx.xent_shape, -ctx.xent_scale) if hasattr(ctx, "xent_grad") else None
        if ctx.pen[1] > 0.0:
            g = _penalized(g, *ctx.pen)
        if ctx.row_w is not None:  # ([K] MulRowsVec; row t*B + b is element (b, :, t) here)
            B, _, T = ctx.in_shape
            w = ctx.row_w.view(T, B).t().unsqueeze(1)
            g = g * w
            xg = xg * w if xg is not None else None
        return (g, xg, None, None, None, None, None, None, None, None, None)


class _ChainStep(Function):
    """The whole training-side step behind ONE library call (``tc_chain_step``): what ``_ChainLoss`` / ``_ChainLoss3d``
    above do with four to six calls and as many tensor allocations -- layout copies, objective, the reference's second
    call for ``kaldi_way=False``, cross-entropy objective, loss value, gradients in the input's own layout.  The
    reference's step is one FFI call too (``torchain/functions.py:82-86``).  Same values as the classes above (tested)."""

    @staticmethod
    def forward(ctx, input, xent_input, results, den_graph, supervision,
                l2_regularize, leaky_hmm_coefficient, xent_regularize=0.0, kaldi_way=False, deriv_weights=None,
                out_of_range_regularize=0.0):
        out, grad, xgrad = _run_step(input, xent_input, results, den_graph, supervision, l2_regularize,
                                     leaky_hmm_coefficient, xent_regularize, kaldi_way, want_grad=True,
                                     deriv_weights=deriv_weights, out_of_range_regularize=out_of_range_regularize)
        ctx.grads = (grad, xgrad)
        if results._defer_host_copy:
            return input.new_zeros(1)
        return out[3:4].to(input.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        return (ctx.grads[0], ctx.grads[1], None, None, None, None, None, None, None, None, None)


def _run_step(input, xent_input, results, den_graph, supervision, l2_regularize, leaky_hmm_coefficient,
              xent_regularize, kaldi_way, want_grad, deriv_weights=None, out_of_range_regularize=0.0):
    """One ``tc_chain_step_strided``, in the layout ``classify_layout`` finds (a time-major view as the 2-D rows it is;
    gradients of channel-last views come back as views of dense tensors).  ``want_grad=False`` is the evaluation step
    (``grad == NULL``): forward recursions only, no gradient tensors -- [K] ``ComputeChainObjfAndDeriv`` with ``nnet_output_deriv == NULL``; ``deriv_weights``
    (checked by ``_deriv_weights``) are then not passed on, and ``out_of_range_regularize`` (checked by ``_out_of_range``)
    has nothing to act on."""
    device = input.device
    use_xent = xent_input is not None and xent_regularize != 0.0
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
    x = input.detach()
    xe = xent_input.detach() if use_xent else None
    dtype = _STEP_DTYPES[x.dtype]
    if xe is not None and xe.dtype != x.dtype:
        raise ValueError("input and xent_input must have the same dtype (%s, %s)" % (x.dtype, xe.dtype))
    kind, s0, s1 = _layout(x)
    if kind == "other" or (xe is not None and _layout(xe)[0] != kind):
        raise ValueError("input and xent_input must come in one layout the step takes (%s, %s)"
                         % (tuple(x.stride()), tuple(xe.stride()) if xe is not None else None))
    if kind in ("time_major", "channel_last") and xe is not None and _layout(xe) != (kind, s0, s1):
        raise ValueError("input and xent_input must be views with the same strides (%s, %s)"
                         % (tuple(x.stride()), tuple(xe.stride())))
    if kind == "time_major":  # the 2-D layout where it lies: row t*S + s at (t*S + s) * s0
        x = x.as_strided((S * T, P), (s0, 1))
        xe = xe.as_strided((S * T, P), (s0, 1)) if xe is not None else None
    layout = {"rows": TC_LAYOUT_ROWS, "time_major": TC_LAYOUT_ROWS, "bct": TC_LAYOUT_BCT}.get(kind, TC_LAYOUT_CHANNEL_LAST)
    row_stride = x.stride(0) if layout == TC_LAYOUT_ROWS else 0
    # (gradients: contiguous in the 2-D and the (B, C, T) layout; dense (B, T, C) for a channel-last view)
    gshape = {TC_LAYOUT_ROWS: (S * T, P), TC_LAYOUT_BCT: (S, P, T), TC_LAYOUT_CHANNEL_LAST: (S, T, P)}[layout]
    grad = torch.empty(gshape, dtype=x.dtype, device=device) if want_grad else None
    xgrad = torch.empty(gshape, dtype=x.dtype, device=device) if use_xent and want_grad else None
    with torch.cuda.device(device):
        cur = torch.cuda.current_stream(device)
        key = (S, T, layout != TC_LAYOUT_ROWS, use_xent, dtype)  # (a channel-last step has the (B, C, T) step's workspace)
        sizes = den_graph.__dict__.setdefault("_step_bytes", {}) if isinstance(den_graph, io.DenominatorGraph) else {}
        nbytes = sizes.get(key)
        if nbytes is None:
            nbytes = lib.tc_chain_step_strided_workspace_bytes(den_ptr, S, T, layout, int(use_xent), dtype)
            if nbytes < 0:
                check(int(nbytes), "tc_chain_step_strided_workspace_bytes")
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
        check(lib.tc_chain_step_strided(*args, _ptr(w), float(out_of_range_regularize), dtype, *tail),
              "tc_chain_step_strided")
        results._dev = out[:3]
        results._stale = True
        results._ready = None
        if capturing:
            results._graph_keeps = (ws, w)  # replays write through it; read the values after a replay with ``invalidate()``
        else:
            results._ready = torch.cuda.Event()
            results._ready.record(cur)
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


def _step_tensor(x):
    return x.is_cuda and x.dtype in _STEP_DTYPES


def _one_call(x):
    """Tensors the step takes in the reference's own two layouts (``classify_layout``: ``rows`` or ``bct``): CUDA float32
    (or bfloat16 / float16), (B, C, T) contiguous or 2-D with unit column stride.  (What the registered operator accepts.)"""
    return x is None or (_step_tensor(x) and _layout(x)[0] in ("rows", "bct"))


def _step_view(x):
    """... or in any layout ``tc_chain_step_strided`` takes as it is: those two, or a channel-last view of a (B, C, T) shape."""
    return x is None or (_step_tensor(x) and _layout(x) != _OTHER)


def _step_plan(input, xent_input):
    """The layout ``(kind, s0, s1)`` in which ``input`` and ``xent_input`` go to the one call together, or None when they
    do not: 2-D rows with one row stride, two contiguous (B, C, T) tensors, or two channel-last views of one shape with the
    same two strides (a joint head split in two)."""
    if not _step_view(input) or not _step_view(xent_input):
        return None
    a = _layout(input)
    if xent_input is None:
        return a
    if _layout(xent_input) != a:
        return None
    if a[0] in ("time_major", "channel_last") and tuple(xent_input.shape) != tuple(input.shape):
        return None
    return a


def _needs_grad(input, xent_input):
    if not torch.is_grad_enabled():
        return False
    return input.requires_grad or (xent_input is not None and xent_input.requires_grad)


def _as_step_input(x, xe=None):
    """Tensors ``tc_chain_step`` takes as they are (evaluation steps only: nothing flows back, so a copy is harmless).  A
    pair of channel-last views with the same strides stays as it is; otherwise a view is copied."""
    def one(t):
        assert t.is_cuda, "Only CUDA implementation is available"
        t = t.detach()
        return t if t.dtype in _STEP_DTYPES else t.float()
    x, xe = one(x), (one(xe) if xe is not None else None)
    if _step_plan(x, xe) is not None:
        return x, xe
    return (x if _one_call(x) else x.contiguous()), (xe if _one_call(xe) else xe.contiguous())


def _same_dtype(input, xent_input):
    """``input`` and ``xent_input`` of different dtypes: the 16-bit one(s) up-cast to float32 (tracked by autograd), which
    takes the float32 path -- correct, but with the two extra passes the 16-bit one call saves."""
    if xent_input is None or xent_input.dtype == input.dtype:
        return input, xent_input
    return (input.float() if input.dtype in _HALF else input), (xent_input.float() if xent_input.dtype in _HALF else xent_input)


def _half_one_call(input, xent_input):
    """16-bit CUDA inputs in a layout ``tc_chain_step_typed`` does not take as it is: made contiguous (tracked by autograd)
    so that the step is still one call; up-cast to float32 when even that does not fit (a 3-D input with a 2-D
    ``xent_input``).  Channel-last views that go to the one call together stay as they are."""
    if _step_plan(input, xent_input) is not None:
        return input, xent_input
    input = input if _one_call(input) else input.contiguous()
    if xent_input is not None:
        xent_input = xent_input if _one_call(xent_input) else xent_input.contiguous()
        if xent_input.dim() != input.dim():
            return input.float(), xent_input.float()
        if input.dim() == 2 and xent_input.stride(0) != input.stride(0):
            input, xent_input = input.contiguous(), xent_input.contiguous()
    return input, xent_input


def to2d(x):
    if x.dim() == 3:  # (B, C, T)
        n_pdf = x.shape[1]
        x = x.permute(2, 0, 1).contiguous().view(-1, n_pdf)  # (T * B, C)
    assert x.dim() == 2
    return x


def _fusable(x):
    return x.dim() == 3 and x.is_cuda and x.dtype == torch.float32


def chain_loss(input, den_graph, supervision,
               l2_regularize=0.0, leaky_hmm_coefficient=1e-5,
               xent_regularize=0.0, xent_input=None, kaldi_way=False, *, deriv_weights=None, **options):
    """``options``: ``out_of_range_regularize=0.0``, keyword-only (the module docstring; ``_options``)."""
    return _chain_loss_into(ChainResults(), input, den_graph, supervision, l2_regularize, leaky_hmm_coefficient,
                            xent_regularize, xent_input, kaldi_way, deriv_weights, _options(options))


# What introspection reports stays the reference's signature (torchain/functions.py:128-130), the drop-in surface callers
# compare against; ``deriv_weights`` (``chain_loss.__kwdefaults__``) and ``out_of_range_regularize`` (through ``**options``)
# are this library's keyword-only extensions.
chain_loss.__signature__ = inspect.signature(chain_loss).replace(
    parameters=[p for p in inspect.signature(chain_loss).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD])


def _chain_loss_into(results, input, den_graph, supervision, l2_regularize, leaky_hmm_coefficient, xent_regularize,
                     xent_input, kaldi_way, deriv_weights=None, out_of_range_regularize=0.0):
    """``chain_loss`` with the ``ChainResults`` given (parallel.chain_loss_data_parallel passes one that defers the
    host copy of the three floats until after its all-reduce)."""
    deriv_weights = _deriv_weights(deriv_weights, _rows_of(input))
    c = _out_of_range(out_of_range_regularize)
    input, xent_input = _same_dtype(input, xent_input)
    if not _needs_grad(input, xent_input):  # (deriv_weights and the penalty: checked above, not used without a gradient)
        # Evaluation (the recipe's validation loop runs under torch.no_grad(), example/chime5/train.py:150-171): the
        # forward recursions only.  The reference has no such check (functions.py:74,82) and pays for a training step.
        x, xe = _as_step_input(input, xent_input)
        out, _, _ = _run_step(x, xe, results, den_graph, supervision, l2_regularize, leaky_hmm_coefficient,
                              xent_regularize, kaldi_way, want_grad=False)
        return (input.new_zeros(1) if results._defer_host_copy else out[3:4].to(input.dtype)), results
    if input.is_cuda and input.dtype in _HALF:
        input, xent_input = _half_one_call(input, xent_input)
    if _step_plan(input, xent_input) is not None:
        loss = _ChainStep.apply(input, xent_input, results, den_graph, supervision,
                                l2_regularize, leaky_hmm_coefficient, xent_regularize, kaldi_way, deriv_weights, c)
        return loss, results
    if _fusable(input) and (xent_input is None or _fusable(xent_input)):
        loss = _ChainLoss3d.apply(input, xent_input, results, den_graph, supervision,
                                  l2_regularize, leaky_hmm_coefficient, xent_regularize, kaldi_way, deriv_weights, c)
        return loss, results
    input = to2d(input)
    if xent_input is not None:
        xent_input = to2d(xent_input)

    loss = _ChainLoss.apply(input, xent_input, results, den_graph, supervision,
                            l2_regularize, leaky_hmm_coefficient, xent_regularize, kaldi_way, deriv_weights, c)
    return loss, results
