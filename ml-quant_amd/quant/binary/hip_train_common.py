"""What the train steps of ``QuantConv2d`` (``hip_train``) and ``QuantLinear`` (``hip_train_linear``) do alike: the weight
side and the activation side of the forward.  Each takes the module (a ``HipQuantModule``) and the binding ``_hip`` as
parameters; geometry, ``supported()``, the input-gradient and weight-gradient routes differ and stay with the steps.
"""

import torch

from quant.binary.activation_quantization import MovingAverageMode
from quant.binary.hip_module import zero_planes


def step_weight_planes(mod, weight4: torch.Tensor, geom, _hip):
    """(wscales [planes, O], wbits, wsum) of this step for the detached weight ``weight4`` [O, C, KH, KW]: the scales are
    computed from it and cached in the module's buffers (train mode, weight_quantization.py:29-31), then the planes packed."""
    with torch.no_grad():
        mod.w_approximate(weight4)
        wscales = mod.w_approximate.plane_scales().to(torch.float32).contiguous()
    wbits, wsum = _hip.pack_weight(weight4, geom, wscales)
    return wscales, wbits, wsum


def step_planes(mod, geom, k: int, device, _hip, extra: tuple = ()) -> torch.Tensor:
    """The module's activation-plane workspace for train steps, one per input shape and launch stream as in eval mode -- for
    steps whose backward reads the saved scales, not the planes."""
    return mod._workspace('train_planes', (geom.key()[:4],) + extra + (k, device, _hip.stream_ptr(device)),
                          lambda: zero_planes(geom, k, device, _hip))


def step_act_quant(mod, x: torch.Tensor, geom, planes: torch.Tensor, _hip, alpha=None, pre=None) -> torch.Tensor:
    """lsq_act_quant (a bf16 / fp16 ``x``: lsq_act_quant_half) of the samples ``x`` of ``geom`` into ``planes``; returns the
    step's scales [planes, N] (a tensor of the step, saved for backward).  Moving averages (activation_quantization.py:72-88)
    are tracked from the batch's mean scales; 'train_and_eval' quantizes again with the tracked values.  ``alpha``: the clamp
    bound where it is not ``_alpha()`` (rounded into a 16-bit type).  ``pre`` = (scale [C], shift [C]), fp32 ``x`` only: the
    quantizer reads fmaf(x, scale[c], shift[c]) (a batch norm folded into its read), in both launches."""
    xq = mod.x_approximate
    k, n, alpha = xq.n_planes, geom.N, (mod._alpha() if alpha is None else alpha)
    act_quant = _hip.act_quant if x.dtype == torch.float32 else _hip.act_quant_half
    fold = {} if pre is None else {'pre': pre}
    xscales = torch.empty((k, n), dtype=torch.float32, device=x.device)
    forced = xq._forced_scales
    forced = None if forced is None else xq.plane_scales(forced).to(device=x.device, dtype=torch.float32).contiguous()
    act_quant(x, geom, xq.hip_scheme, k, mod.act_skip, alpha, planes, xscales, forced, **fold)
    if forced is None and xq.moving_average_mode != MovingAverageMode.off:
        with torch.no_grad():
            tracked = xq.moving_avg_module(xscales[:xq.num_scaling_factors].mean(1))
        if xq.moving_average_mode == MovingAverageMode.train_and_eval:
            forced = xq.plane_scales(tracked.view(-1, 1).expand(-1, n)).to(torch.float32).contiguous()
            act_quant(x, geom, xq.hip_scheme, k, mod.act_skip, alpha, planes, xscales, forced, **fold)
    return xscales
