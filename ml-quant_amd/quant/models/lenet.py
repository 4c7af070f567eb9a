"""LeNet-5 with a quantized second convolution.

Same constructor, sub-module names and forward as the reference's ``quant/models/lenet.py``
(:21-94): first and last layers full precision, ``conv2`` a 5x5 ``QuantConv2d`` over 20
input channels (not a multiple of 64, no padding) fed by a non-affine batch norm.
One optional keyword of this project's own, ``fc1_quant``, makes ``fc1`` a ``QuantLinear``.
"""

from typing import Callable, Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from quant import _hip
from quant.binary.binary_conv import QuantConv2d
from quant.binary.binary_linear import QuantLinear
from quant.models import resnet


class QLeNet5(nn.Module):
    """conv5-relu-bn-pool, bn-quantconv5-relu-pool, fc-relu-fc, log-softmax."""

    def __init__(self, loss_fn: Callable[..., torch.Tensor], conv1_filters: int = 20, conv2_filters: int = 50,
                 output_classes: int = 10, x_quant: str = 'fp', w_quant: str = 'fp',
                 clamp: Optional[Dict] = None, moving_average_mode: str = 'off',
                 moving_average_momentum: float = 0.99, fc1_quant: Optional[Dict] = None) -> None:
        """``fc1_quant``: None (``fc1`` full precision, as in the reference), or ``{'x_quant', 'w_quant'[, 'clamp']}`` for a
        binary ``fc1`` (``QuantLinear``, 800 -> 500 with the default sizes; moving-average settings as ``conv2``'s)."""
        super().__init__()
        setattr(self, 'loss_fn', loss_fn)
        self.conv1_filters, self.conv2_filters = conv1_filters, conv2_filters
        self.output_classes = output_classes
        self.x_quant, self.w_quant = x_quant, w_quant

        self.conv1 = nn.Conv2d(1, conv1_filters, 5, stride=1)
        self.bn_conv1 = nn.BatchNorm2d(conv1_filters, eps=1e-4, momentum=0.1, affine=False)
        self.conv2 = QuantConv2d(x_quant, w_quant, conv1_filters, conv2_filters, 5, clamp,
                                 moving_average_mode, moving_average_momentum, stride=1)
        self.bn_conv2 = nn.BatchNorm2d(conv1_filters, eps=1e-4, momentum=0.1, affine=False)
        hidden = conv2_filters * output_classes
        if fc1_quant is None:
            self.fc1 = nn.Linear(conv2_filters * 4 * 4, hidden)
        else:
            self.fc1 = QuantLinear(fc1_quant['x_quant'], fc1_quant['w_quant'], conv2_filters * 4 * 4, hidden,
                                   fc1_quant.get('clamp'), moving_average_mode, moving_average_momentum)
        self.fc2 = nn.Linear(hidden, output_classes)

    def _bn_conv1_affine(self):
        """(scale, shift) of the eval-mode ``bn_conv1``: ``1 / sqrt(var + eps)`` and ``-mean / sqrt(var + eps)``, times
        / plus its weight and bias where it has them; cached against the buffers' versions (as resnet._folded_conv_bn)."""
        bn = self.bn_conv1
        tensors = [bn.running_mean, bn.running_var] + ([bn.weight, bn.bias] if bn.affine else [])
        stamp = tuple((t._version, t.data_ptr()) for t in tensors)
        hit = self.__dict__.get('_front_affine')
        if hit is None or hit[0] != stamp:
            with torch.no_grad():
                scale = torch.rsqrt(bn.running_var + bn.eps)
                if bn.affine:
                    scale = scale * bn.weight
                shift = -bn.running_mean * scale
                if bn.affine:
                    shift = shift + bn.bias
            hit = self.__dict__['_front_affine'] = (stamp, scale.float().contiguous(), shift.float().contiguous())
        return hit[1], hit[2]

    def set_input_norm(self, mean, std) -> None:
        """Accept uint8 inputs [N, 1, H, W]: the forward is then the one on ``x.float().div(255).sub(mean).div(std)``.
        Non-persistent buffers: ``state_dict`` keys stay the reference's."""
        resnet._set_input_norm(self, mean, std, self.conv1.in_channels)

    def _front_u8(self, x: torch.Tensor) -> torch.Tensor:
        """``_front`` on a uint8 input; with ``resnet.STEM_U8``, in eval mode on the GPU, ONE kernel (lsq_stem_conv_u8: the
        normalisation inside, the batch norm as its per-channel affine behind the ReLU, pool 2)."""
        bn, conv = self.bn_conv1, self.conv1
        resnet._input_norm(self)
        if (resnet.STEM_U8 and not self.training and not bn.training and bn.track_running_stats
                and bn.running_mean is not None and x.is_cuda):
            gl = resnet._stem_u8_geom(conv, x)
            if gl is not None and _hip.stem_conv_u8_supported(gl[0], 2, gl[1]):
                return _hip.stem_conv_u8(x, conv.weight.detach(), None if conv.bias is None else conv.bias.detach(),
                                         *resnet._u8_affine(self), conv.stride, conv.padding, True, self._bn_conv1_affine(), 2)
        return self._front(resnet._normalise_u8(self, x))

    def _front(self, x: torch.Tensor) -> torch.Tensor:
        """``max_pool2d(bn_conv1(relu(conv1(x))), 2, 2)``; with ``resnet.STEM_GENERAL``, in eval mode on a contiguous fp32
        GPU input, as ONE kernel (lsq_stem_conv_gen: the batch norm is its per-channel affine behind the ReLU).  A uint8 input
        (after ``set_input_norm``) goes through ``_front_u8``."""
        if x.dtype == torch.uint8:
            return self._front_u8(x)
        bn, conv = self.bn_conv1, self.conv1
        if (resnet.STEM_GENERAL and not self.training and not bn.training and bn.track_running_stats
                and bn.running_mean is not None and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                and x.is_contiguous() and not (torch.is_grad_enabled() and x.requires_grad)):
            geom = resnet._stem_gen_geom(conv, x)
            if geom is not None and _hip.stem_conv_gen_supported(geom, 2):
                return _hip.stem_conv_gen(x, conv.weight.detach(), None if conv.bias is None else conv.bias.detach(),
                                          conv.stride, conv.padding, True, self._bn_conv1_affine(), 2)
        return F.max_pool2d(bn(F.relu(conv(x))), kernel_size=2, stride=2)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self._front(x)
        # bn -> quantized conv -> relu: one fused call (on the HIP path the batch norm is folded into the
        # quantizer's read and the ReLU into the conv epilogue; elsewhere it is the plain composition)
        # (the 2 x 2 pool is asked of the same call: with ``QuantConv2d.xnor_narrow`` it runs inside the convolution's launch)
        x = self.conv2.fused_forward(x, self.bn_conv2, relu=True, pool=2)
        x = F.relu(self.fc1(x.reshape(-1, self.conv2_filters * 4 * 4)))
        return F.log_softmax(self.fc2(x), dim=1)
