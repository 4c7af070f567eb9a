"""Train-mode ``QuantConv2d`` on the gfx950 kernels.

The reference trains through stock autograd: ``QuantConv2d.forward`` (quant/binary/binary_conv.py:161-173) composes the
clamp, the activation quantizer (scales from detached data, signs through ``STESign``, quant/binary/ste.py:21-66), the
weight quantizer in its compute-and-cache mode (quant/binary/weight_quantization.py:29-31, :53-56, :77-79, :103-105)
and ``F.conv2d``.  Here the same step is one ``torch.autograd.Function`` around the C ABI:

forward   the weight scales are computed and cached (``copy_`` into the ``v1..vk`` buffers, as the reference does);
          ``lsq_act_quant`` solves the per-sample activation scales and packs the sign planes; ``lsq_pack_weight`` +
          ``lsq_xnor_conv2d`` (binary activations) or ``lsq_signw_conv2d`` (fp activations) produce the output -- the
          kernels of the inference path.  Saved for backward: the input, both sets of scales and, for binary activations,
          this step's sign planes (a buffer of the step, not the module's: a second forward of the same module before
          backward must not change what backward reads).
backward  grad_bias = sum of grad_y;
          grad_xq   = conv_transpose2d(grad_y, w_q): one ``lsq_signw_conv2d`` per weight plane over the flipped,
                      transposed sign weights (packed once per step), the plane's per-output-channel scale folded into
                      its input-channel pre-scale, later planes accumulated through the residual epilogue; stride 2 by
                      zero insertion;
          grad_x    = ``lsq_ste_backward``: straight-through estimator of every sign of the quantizer chain + clamp mask;
          grad_wq   = correlation of x_q with grad_y: binary activations -- ``lsq_train_wgrad`` (liblsq_hip_train.so) reads
                      x_q = sum_p v_p[n] (2 bit_p - 1) from the saved sign planes and scales, a bf16 matrix-core GEMM with
                      exact +-1 signs and a three-term split of v_p grad_y; fp activations -- the clamp's
                      value (``lsq_quant_values``) and ``torch.nn.grad.conv2d_weight`` (MIOpen).  The kernel is taken when
                      ``WGRAD_KERNEL`` is True; by default (False) binary activations go the second way too;
          grad_w    = ``lsq_ste_backward`` over the weight rows.
Geometries the transposed convolution does not take (groups, dilation, strides other than 1 / 2) fall back to the torch
formulation of the module; results are those of the reference's graph within fp32 reassociation (tests: f9_train).
With ``DGRAD_KERNEL`` (False by default) grad_xq is ONE ``lsq_signw_conv2d_dgrad`` (liblsq_hip_conv_train.so) over
the forward's own weight planes, saved with the step: no residual planes, no permute / flip, no second packing and no
zero-inserted gradient; every geometry that kernel's plan accepts (groups, dilation, any stride pair, any padding) then
takes the kernels, and the weight gradient takes ``lsq_train_wgrad`` only where that kernel's stated geometry holds.
The forward's weight side and activation side (forced scales, moving averages) and the module's plane workspace are
``quant.binary.hip_train_common``'s, shared with ``hip_train_linear``; its retention policy is ``HipQuantModule._workspace``.

With ``QuantConv2d.hip_train_half`` (a class attribute, False by default) a bf16 / fp16 input takes a step of its own,
``_QuantConv2dStepHalf`` -- what a layer is handed under ``torch.autocast('cuda', torch.bfloat16)``:
forward   ``lsq_act_quant_half`` reads the 16-bit samples as they are (the clamp bound rounded into their type), then
          ``lsq_xnor_conv2d`` and one rounding of its fp32 result into the type; fp activations: ``lsq_signw_conv2d_half``;
backward  grad_x is ONE ``lsq_signw_conv2d_dgrad_half`` (liblsq_hip_conv_train_half.so): the 16-bit grad_y as it is against the
          forward's own weight planes, the straight-through estimator against the 16-bit x in the kernel's epilogue, a 16-bit
          grad_x -- bit for bit ``lsq_ste_backward(x.float(), lsq_signw_conv2d_dgrad(gy.float())).to(dtype)``.  There is no
          other route for a 16-bit input, so ``DGRAD_KERNEL`` does not matter here; grad_w and grad_b are computed in fp32
          from one ``gy.float()`` as in the fp32 step.  With ``WGRAD_HALF_KERNEL`` (False by default) and binary activations
          in lsq_train_wgrad's geometry they are ONE ``lsq_train_wgrad_half`` (liblsq_hip_train_half.so) instead:
          the 16-bit grad_y as it is against the step's own sign planes, grad_b from the same pass -- no ``gy.float()``, no
          ``x.float()``, no ``lsq_quant_values``.

With ``QuantConv2d.train_bn_fold`` (a class attribute, False by default) the train-mode ``nn.BatchNorm2d`` in front of the
convolution of an ``XnorBasicBlock`` joins the fp32 step: ``_BNQuantConv2dStep`` (liblsq_hip_bn_train.so).
forward   ``lsq_bn_train_stats`` reads x once (statistics, running buffers, scale / shift); the quantizer, or for fp
          activations ``lsq_signw_conv2d``, applies fmaf(x, scale, shift) inside its own read -- bn(x) is never written;
backward  grad_xq as above, then ONE ``lsq_bn_ste_backward``: the straight-through estimator at the recomputed bn(x) and the
          batch norm's backward (grad_x, grad_gamma, grad_beta) in two reads of x and grad_xq and one write; the MIOpen
          weight-gradient route reads ``lsq_quant_values_bn``.
"""

from typing import List, Optional

import torch
from torch.autograd.function import once_differentiable

from quant.binary.hip_module import zero_planes
from quant.binary.hip_train_common import step_act_quant, step_planes, step_weight_planes

# binary activations: the weight gradient on lsq_train_wgrad (True) or on lsq_quant_values + conv2d_weight (False).  Off by
# default: the batch-256 ResNet-18 train step measured slower with the kernel than with MIOpen (DESIGN 4.7,
# profiles/train_step.json) -- the kernel stays the default only once it makes the step faster.
WGRAD_KERNEL = False

# the input gradient on lsq_signw_conv2d_dgrad (True) or on lsq_signw_conv2d in the transposed role, one launch per weight
# plane over re-packed planes, stride 2 by zero insertion (False).  Off by default: the landing rule of WGRAD_KERNEL (DESIGN
# 4.20 holds what was measured).
DGRAD_KERNEL = False

# the 16-bit step (``hip_train_half``) with binary activations: grad_wq and grad_b from ONE lsq_train_wgrad_half
# (liblsq_hip_train_half.so) that reads the 16-bit grad_y as it is and the step's own sign planes (True), or the
# fp32 lines behind gy.float() (False).  A switch of its own, off by default: the landing rule of WGRAD_KERNEL.
WGRAD_HALF_KERNEL = False


def _wgrad_geometry(conv) -> bool:
    """The geometry lsq_train_wgrad states (include/lsq_hip_train.h): groups 1, dilation 1, one stride of 1 or 2, padding
    <= kernel - 1, kernels up to 8 x 8."""
    kh, kw = conv.kernel_size
    return (conv.groups == 1 and tuple(conv.dilation) == (1, 1) and conv.stride[0] == conv.stride[1] and conv.stride[0] in (1, 2)
            and conv.padding[0] <= kh - 1 and conv.padding[1] <= kw - 1 and max(kh, kw) <= 8)


def _half_supported(conv, x, _hip) -> bool:
    """The 16-bit step (``hip_train_half``): autocast off or set to the input's type, what the plan of
    lsq_signw_conv2d_dgrad_half accepts, and the limits of lsq_act_quant_half + lsq_xnor_conv2d (binary activations) or of
    lsq_signw_conv2d_half (fp activations) -- independent of the eval switches ``act_half`` / ``fp_half``."""
    if torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') != x.dtype:
        return False                      # (a 16-bit input under an autocast of another type: torch decides the types)
    geom = conv._geom_of(x, _hip)
    if not _hip.signw_conv2d_dgrad_half_supported(geom):      # (a missing library raises: the switch asked for the kernel)
        return False
    if x.shape[0] > _hip.CONV_DGRAD_HALF_MAX_SAMPLES or conv.out_channels > 65535:
        return False
    if getattr(conv.w_approximate, 'k', 1) > _hip.MAX_PLANES:
        return False
    if conv.x_quant == 'fp':
        return _hip.signw_conv2d_half_supported(geom)
    if getattr(conv.x_approximate, 'n_planes', 1) > _hip.MAX_PLANES or max(conv.kernel_size) > _hip.MAX_XNOR_KERNEL:
        return False
    m = x.shape[1] * x.shape[2] * x.shape[3]
    if conv.x_quant in ('ls-2', 'ls-T') and (m + conv.act_skip - 1) // conv.act_skip >= _hip.MAX_SOLVER_KEYS:
        return False
    return True


def supported(conv, x: torch.Tensor) -> bool:
    """Train-mode forward + backward on the kernels: fp32 (with ``hip_train_half``: bf16 / fp16) 4-d CUDA input, binary
    weights, plain geometry -- and the library built (without it a training run on a GPU host takes the torch formulation;
    the eval path, by contrast, raises)."""
    from quant import _hip
    if not _hip.available():
        return False
    half = x.dtype in (torch.bfloat16, torch.float16) and conv.hip_train_half
    if not (x.is_cuda and x.dim() == 4 and (x.dtype == torch.float32 or half) and conv.weight.dtype == torch.float32):
        return False
    if conv.w_quant == 'fp' or conv.padding_mode != 'zeros' or isinstance(conv.padding, str):
        return False
    if half:
        return _half_supported(conv, x, _hip)
    if DGRAD_KERNEL:
        # what the plan of lsq_signw_conv2d_dgrad accepts (a missing library raises: the switch asked for the kernel)
        if not _hip.signw_conv2d_dgrad_supported(conv._geom_of(x, _hip)):
            return False
    else:
        if conv.groups != 1 or tuple(conv.dilation) != (1, 1) or conv.stride[0] != conv.stride[1] or conv.stride[0] not in (1, 2):
            return False
        kh, kw = conv.kernel_size
        if conv.padding[0] > kh - 1 or conv.padding[1] > kw - 1:
            return False
    if x.shape[0] > 65535 or conv.out_channels > 65535:
        return False
    return conv._hip_supports(x)


def _weight_residual_planes(weight: torch.Tensor, plane_scales: torch.Tensor) -> List[torch.Tensor]:
    """r_q = w - sum_{p<q} u_p sign(r_p): the tensors whose signs are the weight planes (one per plane scale)."""
    out, resid = [], weight
    for q in range(plane_scales.shape[0]):
        out.append(resid)
        if q + 1 < plane_scales.shape[0]:
            sign = torch.where(resid < 0, -torch.ones_like(resid), torch.ones_like(resid))
            resid = resid - plane_scales[q].view(-1, 1, 1, 1) * sign
    return out


_CONSTANTS = {}


def _constants(c: int, o: int, device):
    """(ones [1, c], zeros [o]) on ``device``: read-only operands of the input-gradient convolutions, made once."""
    key = (c, o, device)
    t = _CONSTANTS.get(key)
    if t is None:
        t = _CONSTANTS[key] = (torch.ones((1, c), dtype=torch.float32, device=device),
                               torch.zeros((o,), dtype=torch.float32, device=device))
    return t


def _grad_xq(conv, geom, x, weight, wscales, wbits, gy, _hip):
    """conv_transpose2d(gy, w_q), the gradient with respect to the quantizer's value, [N, C, H, W] fp32: ONE
    lsq_signw_conv2d_dgrad over the step's saved weight planes ``wbits`` where the forward kept them (``DGRAD_KERNEL``), else
    stride-1 sign-weight convolutions of the (zero-inserted) gradient, one per weight plane."""
    if wbits.numel():
        return _hip.signw_conv2d_dgrad(gy, wbits, wscales, geom)
    n, c, h, w = x.shape
    o = conv.out_channels
    kh, kw = conv.kernel_size
    s = conv.stride[0]
    ph, pw = conv.padding
    if s == 1:
        gin = gy
    else:
        hu, wu = h + 2 * ph - kh + 1, w + 2 * pw - kw + 1          # rows / columns a stride-1 pass would produce
        gin = gy.new_zeros((n, o, hu, wu))
        gin[:, :, ::s, ::s][:, :, :gy.shape[2], :gy.shape[3]] = gy
    tgeom = _hip.make_geom(n, o, gin.shape[2], gin.shape[3], c, kh, kw, (1, 1), (kh - 1 - ph, kw - 1 - pw), (1, 1), 1)
    assert _hip.out_hw(tgeom) == (h, w), (_hip.out_hw(tgeom), h, w)
    ones, zeros = _constants(c, o, x.device)
    gxq = None
    for r, u in zip(_weight_residual_planes(weight.detach(), wscales), wscales):
        wt = r.permute(1, 0, 2, 3).flip(2, 3).contiguous()              # [C, O, KH, KW], taps mirrored
        tbits, _ = _hip.pack_weight(wt, tgeom, ones)
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
        _hip.signw_conv2d(gin, -1.0, tbits, ones, None, tgeom, out, pre=(u.contiguous(), zeros), res_post=gxq)
        gxq = out
    return gxq


class _QuantConv2dStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, conv):
        from quant import _hip
        x = x.contiguous()
        n, c, h, w = x.shape
        kh, kw = conv.kernel_size
        alpha = conv._alpha()
        geom = _hip.make_geom(n, c, h, w, conv.out_channels, kh, kw, conv.stride, conv.padding, conv.dilation, conv.groups)
        ho, wo = _hip.out_hw(geom)
        wscales, wbits, wsum = step_weight_planes(conv, weight.detach(), geom, _hip)
        y = torch.empty((n, conv.out_channels, ho, wo), dtype=torch.float32, device=x.device)
        b = None if bias is None else bias.detach()
        keep_planes = False
        if conv.x_quant == 'fp':
            _hip.signw_conv2d(x.detach(), alpha, wbits, wscales, b, geom, y)
            xscales = None
        else:
            k = conv.x_approximate.n_planes
            keep_planes = WGRAD_KERNEL and ctx.needs_input_grad[1] and _wgrad_geometry(conv)
            if keep_planes:
                # backward reads these planes: a buffer of this step (zero halo), saved with it
                planes = zero_planes(geom, k, x.device, _hip)
            else:
                planes = step_planes(conv, geom, k, x.device, _hip, (geom.pad_h, geom.pad_w))
            xscales = step_act_quant(conv, x.detach(), geom, planes, _hip)
            _hip.xnor_conv2d(planes, k, xscales, wbits, wsum, wscales, b, geom, y)
            conv.last_act_scales = xscales
        ctx.conv, ctx.geom, ctx.alpha = conv, geom, alpha
        ctx.has_bias = bias is not None
        saved_planes = planes if (xscales is not None and keep_planes) else None
        # lsq_signw_conv2d_dgrad reads this step's weight planes (a tensor of the step: a second forward packs its own)
        saved_wbits = wbits if (DGRAD_KERNEL and ctx.needs_input_grad[0]) else None
        ctx.save_for_backward(x, weight, wscales, xscales if xscales is not None else x.new_empty(0),
                              saved_planes if saved_planes is not None else x.new_empty(0, dtype=torch.int64),
                              saved_wbits if saved_wbits is not None else x.new_empty(0, dtype=torch.int64))
        return y

    @staticmethod
    @once_differentiable                       # (the straight-through kernels have no second derivative: say so instead of returning a wrong one)
    def backward(ctx, gy):
        from quant import _hip
        conv, geom, alpha = ctx.conv, ctx.geom, ctx.alpha
        x, weight, wscales, xscales, planes, wbits = ctx.saved_tensors
        xscales = xscales if xscales.numel() else None
        gy = gy.contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        gx = gw = gb = None
        if need_b:
            gb = gy.sum(dim=(0, 2, 3))
        if need_x:
            gx = _hip.ste_backward(x, _grad_xq(conv, geom, x, weight, wscales, wbits, gy, _hip), xscales, alpha)
        if need_w:
            if planes.numel():
                gwq = _hip.wgrad(planes, xscales.shape[0], xscales, gy, geom)
            else:
                xq = _hip.quant_values(x, xscales, alpha)
                gwq = torch.nn.grad.conv2d_weight(xq, weight.shape, gy, conv.stride, conv.padding, conv.dilation, conv.groups)
            gw = _hip.ste_backward(weight.detach(), gwq, wscales, -1.0)
        return gx, gw, gb, None


class _QuantConv2dStepHalf(torch.autograd.Function):
    """The step on a bf16 / fp16 input (``hip_train_half``): y and grad_x in the input's type, grad_w and grad_b in fp32."""

    @staticmethod
    def forward(ctx, x, weight, bias, conv):
        from quant import _hip
        x = x.contiguous()
        n, c, h, w = x.shape
        alpha = conv._alpha_in(x.dtype)                 # the bound as Tensor.clamp rounds it into the type
        geom = conv._geom_of(x, _hip)
        with torch.autocast('cuda', enabled=False):
            wscales, wbits, wsum = step_weight_planes(conv, weight.detach(), geom, _hip)
        b = None if bias is None else bias.detach()
        keep_planes = False
        if conv.x_quant == 'fp':
            y = _hip.signw_conv2d_half(x.detach(), alpha, wbits, wscales, b, geom)
            xscales = None
        else:
            k = conv.x_approximate.n_planes
            keep_planes = (WGRAD_KERNEL or WGRAD_HALF_KERNEL) and ctx.needs_input_grad[1] and _wgrad_geometry(conv)
            if keep_planes:
                planes = zero_planes(geom, k, x.device, _hip)
            else:
                planes = step_planes(conv, geom, k, x.device, _hip, (geom.pad_h, geom.pad_w, x.dtype))
            xscales = step_act_quant(conv, x.detach(), geom, planes, _hip, alpha)
            if conv.xnor_half:                          # the rounding in the convolution's epilogue: the same bits
                y = _hip.xnor_conv2d_half(planes, k, xscales, wbits, wsum, wscales, b, geom, x.dtype)
            else:
                y32 = torch.empty((n, conv.out_channels) + tuple(_hip.out_hw(geom)), dtype=torch.float32, device=x.device)
                _hip.xnor_conv2d(planes, k, xscales, wbits, wsum, wscales, b, geom, y32)
                y = y32.to(x.dtype)                     # one rounding of the fp32 result
            conv.last_act_scales = xscales
        ctx.conv, ctx.geom, ctx.alpha = conv, geom, alpha
        ctx.has_bias = bias is not None
        ctx.wgrad_half = bool(WGRAD_HALF_KERNEL and keep_planes)      # (the switch as the forward saw it: it kept the planes)
        empty = x.new_empty(0, dtype=torch.int64)
        ctx.save_for_backward(x, weight, wscales, xscales if xscales is not None else wscales.new_empty(0),
                              planes if keep_planes else empty, wbits if ctx.needs_input_grad[0] else empty)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        from quant import _hip
        conv, geom, alpha = ctx.conv, ctx.geom, ctx.alpha
        x, weight, wscales, xscales, planes, wbits = ctx.saved_tensors
        xscales = xscales if xscales.numel() else None
        gy = gy.to(x.dtype).contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        gx = gw = gb = None
        if need_x:
            gx = _hip.signw_conv2d_dgrad_half(gy, wbits, wscales, geom, x, xscales, alpha)
        if need_w and ctx.wgrad_half:
            # grad_wq, and grad_b with it, from the 16-bit grad_y as it is: no gy.float(), no x.float(), no lsq_quant_values
            with torch.autocast('cuda', enabled=False):
                gwq, gb = _hip.wgrad_half(planes, xscales.shape[0], xscales, gy, geom, bias=need_b)
                gw = _hip.ste_backward(weight.detach(), gwq, wscales, -1.0)
        elif need_w or need_b:
            with torch.autocast('cuda', enabled=False):
                gy32 = gy.float()
                if need_b:
                    gb = gy32.sum(dim=(0, 2, 3))
                if need_w:
                    if planes.numel():
                        gwq = _hip.wgrad(planes, xscales.shape[0], xscales, gy32, geom)
                    else:
                        xq = _hip.quant_values(x.float(), xscales, alpha)
                        gwq = torch.nn.grad.conv2d_weight(xq, weight.shape, gy32, conv.stride, conv.padding, conv.dilation,
                                                          conv.groups)
                    gw = _hip.ste_backward(weight.detach(), gwq, wscales, -1.0)
        return gx, gw, gb, None


class _BNQuantConv2dStep(torch.autograd.Function):
    """``conv(bn(x))`` for a train-mode ``nn.BatchNorm2d`` and fp32 ``x`` (``QuantConv2d.train_bn_fold``): the
    normalised tensor is never written.  Forward: lsq_bn_train_stats reads x once and gives (scale, shift), which the
    quantizer (or, for fp activations, the sign-weight convolution) applies inside its own read.  Backward: grad_xq by the
    routes of ``_QuantConv2dStep``, then ONE lsq_bn_ste_backward for the straight-through estimator and the batch norm
    together.  Saved: x, the five [C] vectors of the statistics, the weight and the scales -- no tensor of x's shape but x."""

    @staticmethod
    def forward(ctx, x, gamma, beta, weight, bias, conv, bn):
        from quant import _hip
        x = x.contiguous()
        n, c, h, w = x.shape
        kh, kw = conv.kernel_size
        alpha = conv._alpha()
        geom = _hip.make_geom(n, c, h, w, conv.out_channels, kh, kw, conv.stride, conv.padding, conv.dilation, conv.groups)
        ho, wo = _hip.out_hw(geom)
        # the batch norm's train-mode bookkeeping (torch.nn.modules.batchnorm._BatchNorm.forward), then its statistics
        count = 1
        running = bn.track_running_stats and bn.running_mean is not None
        if running and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
            if bn.momentum is None:
                count = int(bn.num_batches_tracked)
        stats = _hip.bn_train_stats(x.detach(), None if gamma is None else gamma.detach(), None if beta is None else beta.detach(),
                                    bn.eps, bn.momentum, bn.running_mean if running else None,
                                    bn.running_var if running else None, count)
        mean, var, invstd, scale, shift = stats
        wscales, wbits, wsum = step_weight_planes(conv, weight.detach(), geom, _hip)
        y = torch.empty((n, conv.out_channels, ho, wo), dtype=torch.float32, device=x.device)
        b = None if bias is None else bias.detach()
        keep_planes = False
        if conv.x_quant == 'fp':
            _hip.signw_conv2d(x.detach(), alpha, wbits, wscales, b, geom, y, pre=(scale, shift))
            xscales = None
        else:
            k = conv.x_approximate.n_planes
            keep_planes = WGRAD_KERNEL and ctx.needs_input_grad[3] and _wgrad_geometry(conv)
            if keep_planes:
                planes = zero_planes(geom, k, x.device, _hip)
            else:
                planes = step_planes(conv, geom, k, x.device, _hip, (geom.pad_h, geom.pad_w))
            xscales = step_act_quant(conv, x.detach(), geom, planes, _hip, pre=(scale, shift))
            _hip.xnor_conv2d(planes, k, xscales, wbits, wsum, wscales, b, geom, y)
            conv.last_act_scales = xscales
        ctx.conv, ctx.geom, ctx.alpha = conv, geom, alpha
        ctx.has_bias, ctx.affine = bias is not None, (gamma is not None, beta is not None)
        empty = x.new_empty(0, dtype=torch.int64)
        ctx.save_for_backward(x, mean, var, invstd, scale, shift, weight, wscales,
                              xscales if xscales is not None else x.new_empty(0), planes if keep_planes else empty,
                              wbits if (DGRAD_KERNEL and any(ctx.needs_input_grad[:3])) else empty)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        from quant import _hip
        conv, geom, alpha = ctx.conv, ctx.geom, ctx.alpha
        x, mean, var, invstd, scale, shift, weight, wscales, xscales, planes, wbits = ctx.saved_tensors
        xscales = xscales if xscales.numel() else None
        gy = gy.contiguous()
        need = ctx.needs_input_grad
        need_w, need_b = need[3], ctx.has_bias and need[4]
        gx = ggamma = gbeta = gw = gb = None
        if need_b:
            gb = gy.sum(dim=(0, 2, 3))
        if need[0] or (ctx.affine[0] and need[1]) or (ctx.affine[1] and need[2]):
            gq = _grad_xq(conv, geom, x, weight, wscales, wbits, gy, _hip)
            gx, ggamma, gbeta = _hip.bn_ste_backward(x, gq, scale, shift, mean, invstd, xscales, alpha)
        if need_w:
            if planes.numel():
                gwq = _hip.wgrad(planes, xscales.shape[0], xscales, gy, geom)
            else:
                xq = _hip.quant_values_bn(x, scale, shift, xscales, alpha)
                gwq = torch.nn.grad.conv2d_weight(xq, weight.shape, gy, conv.stride, conv.padding, conv.dilation, conv.groups)
            gw = _hip.ste_backward(weight.detach(), gwq, wscales, -1.0)
        return (gx if need[0] else None, ggamma if (ctx.affine[0] and need[1]) else None,
                gbeta if (ctx.affine[1] and need[2]) else None, gw, gb, None, None)


def bn_fold_supported(conv, bn, x: torch.Tensor) -> bool:
    """Whether ``conv(bn(x))`` takes ``train_step_forward_bn``: the class switch ``train_bn_fold`` (and ``hip_train``), both
    modules training, ``bn`` a plain ``nn.BatchNorm2d`` (not a subclass: SyncBatchNorm's statistics are not one device's), a 4-d
    fp32 ``x`` that ``supported`` accepts with at least two values per channel (below that torch raises) and at most 65535
    channels, fp32 batch-norm parameters and buffers.  Anything else keeps ``conv(bn(x))``."""
    if not (conv.train_bn_fold and conv.hip_train and conv.training and bn.training and type(bn) is torch.nn.BatchNorm2d):
        return False
    if not (x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] == bn.num_features and x.shape[1] <= 65535
            and x.shape[0] * x.shape[2] * x.shape[3] >= 2):
        return False
    if any(t is not None and (t.dtype != torch.float32 or t.device != x.device)
           for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
        return False
    if torch.is_autocast_enabled('cuda'):
        return False                      # (under autocast torch decides the batch norm's types)
    return supported(conv, x)


def train_step_forward_bn(conv, bn, x: torch.Tensor) -> torch.Tensor:
    """``conv(bn(x))`` in train mode through the kernels with the batch norm folded into them (``bn_fold_supported`` holds):
    differentiable with respect to x, the batch norm's weight and bias and the convolution's; updates ``bn``'s buffers."""
    return _BNQuantConv2dStep.apply(x, bn.weight, bn.bias, conv.weight, conv.bias, conv, bn)


def train_step_forward(conv, x: torch.Tensor) -> torch.Tensor:
    """``conv(x)`` in train mode through the kernels, differentiable with respect to x, weight and bias."""
    if x.dtype != torch.float32:
        return _QuantConv2dStepHalf.apply(x, conv.weight, conv.bias, conv)
    return _QuantConv2dStep.apply(x, conv.weight, conv.bias, conv)
