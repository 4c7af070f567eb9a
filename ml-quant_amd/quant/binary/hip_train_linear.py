"""Train-mode ``QuantLinear`` on the gfx950 kernels: the counterpart of ``quant.binary.hip_train`` for the linear layer.

The torch formulation (``QuantLinear._forward_torch``) trains through stock autograd: the clamp, the activation quantizer
(scales from detached data, signs through ``STESign``), the weight quantizer in its compute-and-cache mode and
``F.linear`` over fp32 ``x_q`` and ``w_q``.  Here the same step is one ``torch.autograd.Function`` around the C ABI, for an
input ``[N, F]`` or ``[N, *, F]`` (T = the product of the middle dimensions, M = N * T rows):

forward   the weight scales are computed from the detached weight and cached (``copy_`` into the ``v1..vk`` buffers, as
          the torch formulation does in train mode); ``lsq_pack_weight`` packs this step's sign planes;
          binary activations: ``lsq_act_quant`` on (N, T*F, 1, 1) solves the per-sample scales and packs the planes, then
          ``lsq_linear_xnor``; fp activations: ``lsq_linear_signw`` (clamp fused) -- the kernels of the inference path.
          Saved for backward: the input, the weight, both sets of scales and the weight planes -- tensors of the step, so
          a second forward of the same module before backward changes nothing backward reads.
backward  grad_bias = sum over the rows of grad_y;
          grad_xq   = grad_y . w_q: ``lsq_linear_signw_dgrad`` (liblsq_hip_linear_train.so) from the forward's own weight
                      planes, one bit per weight;
          grad_x    = ``lsq_ste_backward`` over the sample rows (N, T*F): straight-through estimator of every sign of the
                      quantizer chain + clamp mask;
          grad_wq   = grad_y^T x_q with x_q = ``lsq_quant_values`` (fp activations: the clamp's value) on ``torch.mm`` -- the
                      library route ``hip_train`` takes by default for the convolution; with ``WGRAD_KERNEL`` and binary
                      activations ``lsq_linear_signx_wgrad`` (liblsq_hip_linear_wgrad.so) from the input's sign bits
                      instead: no x_q is written;
          grad_w    = ``lsq_ste_backward`` over the weight rows.
Nothing is computed for an input that needs no gradient.  Results are those of the torch formulation within fp32
reassociation and the bf16 hi + lo split of the kernels (tests: test_gpu_linear_train.py).
The forward's weight side and activation side (forced scales, moving averages) and the module's plane workspace are
``quant.binary.hip_train_common``'s, shared with ``hip_train``; its retention policy is ``HipQuantModule._workspace``.

With ``QuantLinear.hip_train_half`` (a class attribute, False by default; it does not need ``hip_train``) a bf16 / fp16 input
takes a step of its own, ``_QuantLinearStepHalf`` -- what a layer is handed under
``torch.autocast('cuda', torch.bfloat16)``:
forward   ``lsq_act_quant_half`` on (N, T*F, 1, 1) reads the 16-bit samples as they are (the clamp bound rounded into their
          type; every scheme free-running, forced scales, both moving-average modes), then ``lsq_linear_xnor`` and one
          rounding of its fp32 result into the type; fp activations: ``lsq_linear_signw_half``;
backward  grad_x is ONE ``lsq_linear_signw_dgrad_half`` (liblsq_hip_linear_train_half.so): the 16-bit grad_y as it is against
          the forward's own weight planes, the straight-through estimator against the 16-bit x in the kernel's epilogue, a
          16-bit grad_x -- bit for bit ``lsq_ste_backward(x.float(), lsq_linear_signw_dgrad(gy.float())).to(dtype)``; grad_w
          and grad_b are computed in fp32 from one ``gy.float()`` as in the fp32 step (``x.float()``, then ``torch.mm`` or,
          with ``WGRAD_KERNEL``, ``lsq_linear_signx_wgrad`` on the two copies, then ``lsq_ste_backward``);
          with ``WGRAD_HALF_KERNEL`` and binary activations grad_w is ONE ``lsq_linear_signx_wgrad_half``
          (liblsq_hip_linear_wgrad_half.so) instead: the 16-bit grad_y and x as they are, the sign image of x, the
          straight-through estimator of the weight quantizer in the GEMM's epilogue -- bit for bit
          ``lsq_ste_backward(weight, lsq_linear_signx_wgrad(gy.float(), x.float()))`` with no fp32 copy of either operand, no
          x_q and no fp32 product in memory; grad_b on that route is ``gy.sum(dim=0, dtype=torch.float32)``.
"""

import os

import torch
from torch.autograd.function import once_differentiable

from quant.binary.hip_train_common import step_act_quant, step_planes, step_weight_planes

# True: the weight gradient of a layer with binary activations runs on lsq_linear_signx_wgrad (sign image + bf16 hi + lo
# GEMM on the matrix cores) instead of lsq_quant_values + torch.mm -- the counterpart of hip_train.WGRAD_KERNEL; DESIGN 4.13
# has the measurements.  fp activations keep torch.mm under either setting.
WGRAD_KERNEL = False

# True: in the 16-bit step (``hip_train_half``) the weight gradient of a layer with binary activations is one
# lsq_linear_signx_wgrad_half call on the 16-bit grad_y and x (the weight's straight-through estimator in its epilogue) instead
# of two fp32 copies + lsq_quant_values + torch.mm (or lsq_linear_signx_wgrad) + lsq_ste_backward -- the counterpart of
# hip_train.WGRAD_HALF_KERNEL; DESIGN 4.29 has the measurements.  Independent of WGRAD_KERNEL and ahead of it in the 16-bit
# step; fp activations and a missing library keep the routes above.
WGRAD_HALF_KERNEL = False


def _half_supported(lin, x, _hip) -> bool:
    """The 16-bit step (``hip_train_half``): autocast off or set to the input's type, at most 65535 samples (the limit of
    lsq_linear_signw_dgrad_half's epilogue), and the limits of lsq_act_quant_half + lsq_linear_xnor (binary activations) or of
    lsq_linear_signw_half (fp activations) -- independent of the eval switches ``act_half_solve`` / ``half_kernel_classes``."""
    if torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') != x.dtype:
        return False                      # (a 16-bit input under an autocast of another type: torch decides the types)
    _hip.linear_train_half_lib()          # (a missing library raises: the switch asked for the kernel)
    if x.shape[0] > _hip.LINEAR_DGRAD_HALF_MAX_SAMPLES:
        return False
    if not os.path.exists(_hip.linear_half_library_path() if lin.x_quant == 'fp' else _hip.linear_library_path()):
        return False
    if lin.x_quant != 'fp' and not os.path.exists(_hip.conv_act_half_library_path()):
        return False
    return lin._hip_supports(x, train_step=True)


def supported(lin, x: torch.Tensor) -> bool:
    """Train-mode forward + backward on the kernels: fp32 (``hip_train``) or bf16 / fp16 (``hip_train_half``) CUDA input
    ``[N, *, F]``, fp32 CUDA weight, binary weights, the limits of ``QuantLinear._hip_supports`` -- and the libraries built
    (without them an fp32 training run takes the torch formulation; the eval path, by contrast, raises)."""
    half = x.dtype in (torch.bfloat16, torch.float16) and lin.hip_train_half
    if not x.is_cuda or lin.weight.dtype != torch.float32 or not lin.weight.is_cuda:
        return False
    if not (half or x.dtype == torch.float32):
        return False
    if lin.w_quant == 'fp':
        return False
    if x.dim() < 2 or x.shape[-1] != lin.in_features or x.numel() == 0:
        return False
    from quant import _hip
    if not _hip.available():
        return False
    if half:
        return _half_supported(lin, x, _hip)
    if not os.path.exists(_hip.linear_train_library_path()):
        return False
    if not os.path.exists(_hip.linear_fp_library_path() if lin.x_quant == 'fp' else _hip.linear_library_path()):
        return False
    return lin._hip_supports(x)


class _QuantLinearStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, lin):
        from quant import _hip
        x = x.contiguous()
        n, t = lin._rows(x)
        f, o = lin.in_features, lin.out_features
        m = n * t
        alpha = lin._alpha()
        wgeom = _hip.make_geom(1, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
        wscales, wbits, wsum = step_weight_planes(lin, weight.detach().view(o, f, 1, 1), wgeom, _hip)
        b = None if bias is None else bias.detach()
        if lin.x_quant == 'fp':
            y = _hip.linear_signw(x.detach().view(m, f), alpha, wbits, wscales, b, m, f, o)
            xscales = None
        else:
            k = lin.x_approximate.n_planes
            geom = _hip.make_geom(n, t * f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
            planes = step_planes(lin, geom, k, x.device, _hip)
            xscales = step_act_quant(lin, x.detach().view(n, t * f), geom, planes, _hip)
            y = _hip.linear_xnor(planes, k, xscales, t, wbits, wsum.view(wscales.shape[0], o), wscales, b, m, f, o)
            lin.last_act_scales = xscales
        ctx.alpha, ctx.dims = alpha, (n, t, f, o)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, wscales, wbits, xscales if xscales is not None else x.new_empty(0))
        return y.view(*x.shape[:-1], o)

    @staticmethod
    @once_differentiable                       # (the straight-through kernels have no second derivative: say so instead of returning a wrong one)
    def backward(ctx, gy):
        from quant import _hip
        x, weight, wscales, wbits, xscales = ctx.saved_tensors
        xscales = xscales if xscales.numel() else None
        n, t, f, o = ctx.dims
        m, alpha = n * t, ctx.alpha
        gy2 = gy.reshape(m, o).contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        gx = gw = gb = None
        if need_b:
            gb = gy2.sum(dim=0)
        if need_x:
            gxq = _hip.linear_signw_dgrad(gy2, wbits, wscales, m, f, o)
            gx = _hip.ste_backward(x.view(n, t * f), gxq.view(n, t * f), xscales, alpha).view(x.shape)
        if need_w:
            if WGRAD_KERNEL and xscales is not None and os.path.exists(_hip.linear_wgrad_library_path()):
                gwq = _hip.linear_signx_wgrad(gy2, x.view(m, f), xscales, alpha, n, t, f, o)
            else:
                xq = _hip.quant_values(x.view(n, t * f), xscales, alpha).view(m, f)
                gwq = torch.mm(gy2.t(), xq)
            gw = _hip.ste_backward(weight.detach(), gwq, wscales, -1.0)
        return gx, gw, gb, None


class _QuantLinearStepHalf(torch.autograd.Function):
    """The step on a bf16 / fp16 input (``hip_train_half``): y and grad_x in the input's type, grad_w and grad_b in fp32."""

    @staticmethod
    def forward(ctx, x, weight, bias, lin):
        from quant import _hip
        x = x.contiguous()
        n, t = lin._rows(x)
        f, o = lin.in_features, lin.out_features
        m = n * t
        alpha = lin._alpha_in(x.dtype)                  # the bound as Tensor.clamp rounds it into the type
        wgeom = _hip.make_geom(1, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
        with torch.autocast('cuda', enabled=False):
            wscales, wbits, wsum = step_weight_planes(lin, weight.detach().view(o, f, 1, 1), wgeom, _hip)
        b = None if bias is None else bias.detach()
        if lin.x_quant == 'fp':
            y = _hip.linear_signw_half(x.detach().view(m, f), alpha, wbits, wscales, b, m, f, o)
            xscales = None
        else:
            k = lin.x_approximate.n_planes
            geom = _hip.make_geom(n, t * f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
            planes = step_planes(lin, geom, k, x.device, _hip, (x.dtype,))
            xscales = step_act_quant(lin, x.detach().view(n, t * f, 1, 1), geom, planes, _hip, alpha)
            y32 = _hip.linear_xnor(planes, k, xscales, t, wbits, wsum.view(wscales.shape[0], o), wscales, b, m, f, o)
            y = y32.to(x.dtype)                         # one rounding of the fp32 result
            lin.last_act_scales = xscales
        ctx.alpha, ctx.dims = alpha, (n, t, f, o)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, wscales, xscales if xscales is not None else wscales.new_empty(0),
                              wbits if ctx.needs_input_grad[0] else x.new_empty(0, dtype=torch.int64))
        return y.view(*x.shape[:-1], o)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        from quant import _hip
        x, weight, wscales, xscales, wbits = ctx.saved_tensors
        xscales = xscales if xscales.numel() else None
        n, t, f, o = ctx.dims
        m, alpha = n * t, ctx.alpha
        gy2 = gy.to(x.dtype).reshape(m, o).contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        gx = gw = gb = None
        if need_x:
            gx = _hip.linear_signw_dgrad_half(gy2, wbits, wscales, m, f, o, x.view(m, f), xscales, alpha, T=t).view(x.shape)
        if need_w and WGRAD_HALF_KERNEL and xscales is not None and os.path.exists(_hip.linear_wgrad_half_library_path()):
            with torch.autocast('cuda', enabled=False):
                gw = _hip.linear_signx_wgrad_half(gy2, x.view(m, f), xscales, alpha, n, t, f, o, weight.detach().contiguous(),
                                                  wscales)
                if need_b:
                    gb = gy2.sum(dim=0, dtype=torch.float32)
        elif need_w or need_b:
            with torch.autocast('cuda', enabled=False):
                gy32 = gy2.float()
                if need_b:
                    gb = gy32.sum(dim=0)
                if need_w:
                    x32 = x.float()
                    if WGRAD_KERNEL and xscales is not None and os.path.exists(_hip.linear_wgrad_library_path()):
                        gwq = _hip.linear_signx_wgrad(gy32, x32.view(m, f), xscales, alpha, n, t, f, o)
                    else:
                        xq = _hip.quant_values(x32.view(n, t * f), xscales, alpha).view(m, f)
                        gwq = torch.mm(gy32.t(), xq)
                    gw = _hip.ste_backward(weight.detach(), gwq, wscales, -1.0)
        return gx, gw, gb, None


def train_step_forward(lin, x: torch.Tensor) -> torch.Tensor:
    """``lin(x)`` in train mode through the kernels, differentiable with respect to x, weight and bias."""
    if x.dtype != torch.float32:
        return _QuantLinearStepHalf.apply(x, lin.weight, lin.bias, lin)
    return _QuantLinearStep.apply(x, lin.weight, lin.bias, lin)
