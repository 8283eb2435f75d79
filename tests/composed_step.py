"""The multi-call statement of the training step: ``_ChainLoss`` (2-D) and ``_ChainLoss3d`` ((B, C, T)), the two autograd classes
``chain_loss`` used before every input went to the one library call (``functions._ChainStep``).  They compose the step from four to
six library calls -- layout copies, objective, the reference's second call, cross-entropy objective -- and apply the row weights
and the out-of-range penalty with torch ops.  Kept here, unchanged, as the independent statement the one call is compared against."""
import torch
from torch.autograd import Function

from torchain_amd.functions import (_penalized, _weights_on, compute_chain_objf_and_deriv, from2d_hip, to2d_hip,
                                    xent_objective)


def _device_loss(results, like):
    """-objf / weight as a one-element tensor on the input's device (the reference's ``input.new([results.loss])``,
    functions.py:104) computed from the device-side results: no host round trip."""
    r = results._dev
    return (-(r[0] / r[2])).reshape(1).to(like.dtype)


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


def chain_loss_composed(input, den_graph, supervision, l2_regularize=0.0, leaky_hmm_coefficient=1e-5, xent_regularize=0.0,
                        xent_input=None, kaldi_way=False, *, deriv_weights=None, out_of_range_regularize=0.0):
    """``chain_loss`` for float32 CUDA tensors through the composed classes, as it routed the pairs that did not go to the one
    call together: two (B, C, T) tensors, views included, through ``_ChainLoss3d``; anything else through ``to2d`` and
    ``_ChainLoss``."""
    from torchain_amd.functions import ChainResults, to2d
    results = ChainResults()
    args = (results, den_graph, supervision, l2_regularize, leaky_hmm_coefficient, xent_regularize, kaldi_way, deriv_weights,
            out_of_range_regularize)
    if input.dim() == 3 and (xent_input is None or xent_input.dim() == 3):
        return _ChainLoss3d.apply(input, xent_input, *args), results
    return _ChainLoss.apply(to2d(input), to2d(xent_input) if xent_input is not None else None, *args), results
