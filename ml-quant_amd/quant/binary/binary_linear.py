"""``QuantLinear``: fully connected layer of scaled-binary-quantized activations and weights.

The linear counterpart of ``QuantConv2d``: the same schemes (fp | ls-1 | ls-2 | ls-T | gf-k), constructor arguments
(``x_quant, w_quant, in_features, out_features, clamp, moving_average_mode, moving_average_momentum`` then ``bias``),
attributes (``x_approximate``, ``w_approximate``, ``clamping_fn``, ``quantized_parameters``), quantizer buffer names and
``ValueError``s; construction, the factories, cache invalidation, workspace retention and the eval-side activation
quantization are ``quant.binary.hip_module.HipQuantModule``'s, shared with ``QuantConv2d``.

Semantics are those of the quantizer modules: an activation row is one SAMPLE, ``x.view(N, -1)`` in x's own element
order, quantized on the 4-D view ``(N, T*F, 1, 1)`` (T = the product of the dimensions between the batch and the
features); a weight row is one output feature, quantized on ``(O, F, 1, 1)``.  Input ``[N, F]`` or ``[N, *, F]``,
output ``[N, O]`` or ``[N, *, O]``.

Dispatch of ``forward``:
  * CUDA fp32 tensor, ``eval()`` mode, no gradient wanted for the input, binary schemes on both sides, T == 1 or
    F % 64 == 0 -> lsq_act_quant on (N, T*F, 1, 1), weight sign planes packed once per ``eval()`` session, then the fp4
    matrix-core GEMM lsq_linear_xnor (liblsq_hip_linear.so).  No fallback on this branch: a failed launch raises.
  * the same conditions with ``fp`` activations and binary weights (any T and F) -> the weight sign planes packed once per
    ``eval()`` session, then lsq_linear_signw (liblsq_hip_linear_fp.so): the clamp fused, the fp32 rows split into bf16
    hi + lo on the bf16 matrix cores.  No fallback on this branch either.
  * the same conditions with ``fp`` activations, binary fp32 weights and a bf16 / fp16 input, autocast off or set to the
    input's own type -> the same packed planes, then lsq_linear_signw_half (liblsq_hip_linear_half.so): the 16-bit rows
    read as they are, one MFMA per k-step, the output in the input's type (the fp32 result rounded once).  On a shape
    class of ``half_kernel_classes``' complement the rows go through ``x.float()`` -> lsq_linear_signw -> ``.to(dtype)``
    instead.  No fallback on this branch either.
  * the conditions of the first branch with a bf16 / fp16 input, fp32 weights, autocast off or set to the input's own type,
    and activations that need no scale solve -- ``ls-1``, ``gf-k``, or any scheme whose scales are given
    (``x_approximate.eval_scales``: a moving average, ``_forced_scales``) -> lsq_linear_act_quant_half
    (liblsq_hip_linear_act_half.so) reads the 16-bit rows as they are (the clamp bound rounded into their type), then
    lsq_linear_xnor as above; the output is its fp32 result rounded once into the input's type.  With
    ``act_half_kernel = False`` the rows go through ``x.float()`` -> lsq_act_quant instead: the same bits.  No
    fallback on this branch either.
  * the conditions of the branch above with free-running ``ls-2`` / ``ls-T`` activations and ``act_half_solve`` set (class
    attribute, False by default: nothing is measured yet) -> lsq_linear_act_quant_solve_half
    (liblsq_hip_linear_act_solve.so): the v1 solve on a table of one count per 15-bit magnitude, v2 and both planes in one
    launch, then lsq_linear_xnor; v1 and the planes are those of lsq_act_quant on ``x.float()``, which is the route
    ``act_half_kernel = False`` takes.  No fallback on this branch either.
  * CUDA fp32 tensor in ``train()`` mode with ``hip_train`` set (class attribute, False by default), binary weights and
    the same limits -> the kernels of the inference path for the forward and ``quant.binary.hip_train_linear`` for the
    backward (lsq_linear_signw_dgrad of liblsq_hip_linear_train.so, straight-through estimator), one
    ``torch.autograd.Function`` per call.
  * CUDA bf16 / fp16 tensor in ``train()`` mode with ``hip_train_half`` set (class attribute, False by default; ``hip_train``
    is not needed), binary fp32 weights, autocast off or set to the input's own type, at most 65535 samples and the same
    limits (the ``act_half_solve`` gate is an eval switch and does not apply) -> ``hip_train_linear._QuantLinearStepHalf``:
    lsq_act_quant_half on (N, T*F, 1, 1) + lsq_linear_xnor, or lsq_linear_signw_half, for the forward (y in the input's
    type), ONE lsq_linear_signw_dgrad_half (liblsq_hip_linear_train_half.so) for grad_x in the input's type, grad_w and
    grad_b in fp32.  A missing library raises: the switch asked for the kernel.
  * anything else (CPU, training without ``hip_train`` / a 16-bit input without ``hip_train_half``, ``fp`` weights, 16-bit weights, a 16-bit input with free-running
    ``ls-2`` / ``ls-T`` activations without ``act_half_solve`` or under an autocast of another type, F % 64 != 0 with T > 1 for binary activations, beyond the kernels'
    limits) -> the torch formulation ``F.linear(x_approximate(clamp(x)), w_approximate(w), bias)`` on
    the same 4-D views.
"""

from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from quant.binary.hip_module import HipQuantModule


class QuantLinear(HipQuantModule, nn.Linear):
    """``Linear(x_quant(clamp(x)), w_quant(w))`` with schemes fp | ls-1 | ls-2 | ls-T | gf-k."""

    def __init__(self, x_quant: str, w_quant: str, in_features: int, out_features: int, clamp: Optional[Dict] = None,
                 moving_average_mode: str = 'off', moving_average_momentum: float = 0.99, bias: bool = True) -> None:
        super().__init__(x_quant, w_quant, clamp, moving_average_mode, moving_average_momentum,
                         in_features, out_features, bias=bias)

    # ------------------------------------------------------------------ forward
    #: train-mode CUDA tensors through the kernels (quant.binary.hip_train_linear).  False: the torch formulation, the
    #: default until the measured train step says otherwise
    hip_train = False

    #: shape classes of lsq_linear_signw's tile rule ('split': fewer than 256 tiles of 64 x 64 in M x O, 'big': at least 256
    #: tiles of 128 x 128, 'small': between them) on which a bf16 / fp16 input takes lsq_linear_signw_half -- those where it
    #: is measured faster than x.float() -> lsq_linear_signw -> .to(dtype), the route the other classes take
    half_kernel_classes = frozenset(('split', 'small', 'big'))

    #: a bf16 / fp16 input with binary activations is quantized by lsq_linear_act_quant_half (True) or, for the comparison
    #: of DESIGN 4.16, by lsq_act_quant on x.float() (False): the same planes, scales and output bits
    act_half_kernel = True

    #: a bf16 / fp16 input with FREE-RUNNING ls-2 / ls-T activations takes lsq_linear_act_quant_solve_half (with
    #: act_half_kernel = False: lsq_act_quant on x.float(), the same v1 and planes).  False: the torch formulation, the
    #: default until the kernel is measured against the cast route
    act_half_solve = False

    #: a bf16 / fp16 train-mode CUDA tensor -- what the layer is handed under torch.autocast('cuda', torch.bfloat16) -- through
    #: the kernels: ``hip_train_linear._QuantLinearStepHalf`` on lsq_linear_signw_dgrad_half.  A switch of its own (it does not
    #: need ``hip_train``, which alone governs fp32 inputs).  False: the torch formulation
    hip_train_half = False

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._wants_hip(x):
            return self._forward_hip(x)
        if self.training and x.is_cuda and (self.hip_train or self.hip_train_half):
            from quant.binary import hip_train_linear
            # (fp32 inputs are hip_train's alone; supported() asks hip_train_half for a 16-bit one)
            if (self.hip_train or x.dtype != torch.float32) and hip_train_linear.supported(self, x):
                return hip_train_linear.train_step_forward(self, x)
        return self._forward_torch(x)

    def _rows(self, x: torch.Tensor):
        """(N, T): samples and rows per sample of an input [N, *, F]."""
        if x.dim() < 2 or x.shape[-1] != self.in_features:
            raise ValueError(f'QuantLinear expects [N, *, {self.in_features}], got {list(x.shape)}')
        n = x.shape[0]
        t = 1
        for s in x.shape[1:-1]:
            t *= s
        return n, t

    def _forward_torch(self, x: torch.Tensor) -> torch.Tensor:
        n, t = self._rows(x)
        f, o = self.in_features, self.out_features
        x_q = self.x_approximate(self.clamping_fn(x.reshape(n, t * f, 1, 1))).reshape(x.shape)
        w_q = self.w_approximate(self.weight.view(o, f, 1, 1)).view(o, f)
        return F.linear(x_q, w_q, self.bias)

    def _wants_hip(self, x: torch.Tensor) -> bool:
        if not x.is_cuda or self.training:
            return False
        if torch.is_grad_enabled() and x.requires_grad:
            return False
        if self.w_quant == 'fp':
            return False
        if x.dim() < 2 or x.shape[-1] != self.in_features or x.numel() == 0:
            return False
        if x.dtype != torch.float32 and torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') != x.dtype:
            return False                  # (a 16-bit input under an autocast of another type: torch decides the types)
        return self._hip_supports(x)

    def _hip_supports(self, x: torch.Tensor, train_step: bool = False) -> bool:
        """The limits of lsq_act_quant / lsq_linear_act_quant_half / lsq_linear_act_quant_solve_half and lsq_linear_xnor (binary activations, fp32 / bf16 and
        fp16) or of lsq_linear_signw / lsq_linear_signw_half (fp activations, fp32 / bf16 and fp16); anything outside them
        takes the torch formulation.  ``train_step``: the eval switch ``act_half_solve`` does not apply (the 16-bit train step
        solves free-running ls-2 / ls-T on lsq_act_quant_half)."""
        from quant import _hip
        if self.weight.dtype != torch.float32:
            return False
        if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            return False
        if self.x_quant == 'fp':
            n, t = self._rows(x)
            return (getattr(self.w_approximate, 'k', 1) <= _hip.MAX_PLANES and self.in_features < _hip.LINEAR_MAX_FEATURES
                    and self.out_features < _hip.LINEAR_MAX_OUTPUTS and n * t < 1 << 31)
        if getattr(self.w_approximate, 'k', 1) > _hip.MAX_PLANES or self.x_approximate.n_planes > _hip.MAX_PLANES:
            return False
        n, t = self._rows(x)
        f, row = self.in_features, t * self.in_features
        if t > 1 and f % 64:
            return False                  # the rows of a sample must start on whole plane words
        if f >= _hip.LINEAR_MAX_FEATURES or self.out_features >= _hip.LINEAR_MAX_OUTPUTS or row >= 1 << 31 or n * t >= 1 << 31:
            return False
        if self.x_quant in ('ls-2', 'ls-T') and (row + self.act_skip - 1) // self.act_skip >= _hip.MAX_SOLVER_KEYS:
            return False
        if (not train_step and x.dtype != torch.float32 and self.x_quant in ('ls-2', 'ls-T') and not self.act_half_solve
                and self.x_approximate.eval_scales(n) is None):
            return False                  # (the free-running 16-bit scale solve is off by default: DESIGN 4.17)
        return True

    # ------------------------------------------------------------------ HIP path
    def _packed_weights(self, _hip):
        """Weight sign planes of (O, F, 1, 1), packed once per eval session (re-packed when the weight or a scale changes)."""
        wq = self.w_approximate
        bufs = wq.cached_scales()
        w = self._parameters['weight']
        stamp = (w._version, w.data_ptr()) + tuple((b._version, b.data_ptr()) for b in bufs)
        hit = self._hip_cache.get('w')
        if hit is None or hit[0] != stamp:
            o, f = self.out_features, self.in_features
            geom = _hip.make_geom(1, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
            scales = wq.plane_scales().to(torch.float32).contiguous()
            wbits, wsum = _hip.pack_weight(self.weight.detach().view(o, f, 1, 1), geom, scales)
            hit = (stamp, wbits, wsum.view(scales.shape[0], o), scales)
            self._hip_cache['w'] = hit
        return hit[1], hit[2], hit[3]

    @staticmethod
    def _tile_class(m: int, o: int) -> str:
        """The kernel lsq_linear_signw and lsq_linear_signw_half run for m rows and o outputs (their tile rule)."""
        if ((m + 63) // 64) * ((o + 63) // 64) < 256:
            return 'split'
        return 'big' if ((m + 127) // 128) * ((o + 127) // 128) >= 256 else 'small'

    def _forward_hip(self, x: torch.Tensor) -> torch.Tensor:
        from quant import _hip
        x = x.detach()
        n, t = self._rows(x)
        f, o = self.in_features, self.out_features
        wbits, wsum, wscales = self._packed_weights(_hip)
        bias = None if self.bias is None else self.bias.detach()
        if self.x_quant == 'fp':
            # (the kernel reads whole rows: a strided input -- h[:, 0], a slice of a wider tensor -- is copied first)
            rows = x.reshape(n * t, f).contiguous()
            if x.dtype == torch.float32:
                y = _hip.linear_signw(rows, self._alpha(), wbits, wscales, bias, n * t, f, o)
            elif self._tile_class(n * t, o) in self.half_kernel_classes:
                y = _hip.linear_signw_half(rows, self._alpha(), wbits, wscales, bias, n * t, f, o)
            else:
                # the clamp bound as Tensor.clamp would round it into x's type (negative: none)
                y = _hip.linear_signw(rows.float(), self._alpha_in(x.dtype), wbits, wscales, bias, n * t, f, o).to(x.dtype)
            return y.view(*x.shape[:-1], o)
        geom = _hip.make_geom(n, t * f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
        k = self.x_approximate.n_planes
        if x.dtype == torch.float32:
            planes, scales = self._act_planes(x.reshape(n, t * f), geom, k, _hip)
        else:
            # 16-bit rows: the bound as Tensor.clamp would round it into x's type; planes and scales in a workspace of their
            # own per type; the cast route of DESIGN 4.16 feeds the same rows to lsq_act_quant as fp32
            rows = x.reshape(n, t * f).contiguous()
            planes, scales = self._act_planes(rows if self.act_half_kernel else rows.float(), geom, k, _hip, extra=(x.dtype,),
                                              alpha=self._alpha_in(x.dtype))
        y = _hip.linear_xnor(planes, k, scales, t, wbits, wsum, wscales, bias, n * t, f, o)
        self.last_act_scales = scales
        return (y if x.dtype == torch.float32 else y.to(x.dtype)).view(*x.shape[:-1], o)
