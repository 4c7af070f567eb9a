"""``HipQuantModule``: what ``QuantConv2d`` and ``QuantLinear`` share, as a mixin in front of ``nn.Conv2d`` / ``nn.Linear``.

One copy of each policy the two modules (and their train steps, ``quant.binary.hip_train*``) follow:
  * construction: scheme attributes, the quantizer / clamp factories of the reference's ``QuantConv2d`` (static methods,
    reachable on both classes), ``quantized_parameters`` and the derived-state dict ``_hip_cache``;
  * invalidation: ``train(True)``, ``load_state_dict``, ``_apply`` (``.to()``, ``.double()``) and data-parallel replication
    empty ``_hip_cache``, cooperatively through ``super()``;
  * retention: ``_workspace(kind, key, make)`` -- one workspace per (shape, stream), the newest few of a kind kept;
  * the eval-side activation quantization ``_act_planes``.
``_hip_cache`` is a plain dict: ``'w'`` = packed weights, ``'bn'`` = a folded batch norm, tuples ``(kind, ...)`` = workspaces
and memos (``quant.common.graph_replay`` keeps every value alive for a captured graph's lifetime).
"""

import re
from collections import defaultdict
from functools import partial
from typing import Any, Callable, Dict, List, Optional

import torch
import torch.nn as nn

import quant.binary.activation_quantization as activation_quantization
import quant.binary.quantization as quantization
import quant.binary.weight_quantization as weight_quantization

_SCHEME_RE = re.compile(r'fp|ls-1|ls-2|ls-T|gf-\d+')


def zero_planes(geom, k: int, device, _hip) -> torch.Tensor:
    """A new buffer for ``k`` activation sign planes of ``geom``: halo words must be zero, the kernels only ever write the
    interior."""
    return torch.zeros((k * _hip.act_plane_words(geom),), dtype=torch.int64, device=device)


class HipQuantModule:
    """Schemes fp | ls-1 | ls-2 | ls-T | gf-k on both sides of an ``nn.Conv2d`` / ``nn.Linear`` (next in the MRO)."""

    #: sub-sampling stride of the activation v1 search (quantizer_ls_2 / ls_ternary default)
    act_skip = 3

    def __init__(self, x_quant: str, w_quant: str, clamp: Optional[Dict], moving_average_mode: str,
                 moving_average_momentum: float, *args: Any, **kwargs: Any) -> None:
        super().__init__(*args, **kwargs)             # nn.Conv2d / nn.Linear: weight [out, ...] and bias
        self.x_quant, self.w_quant = x_quant, w_quant
        self.x_approximate = self._get_x_quantizer(x_quant, moving_average_mode, moving_average_momentum)
        self.w_approximate = self._get_w_quantizer(w_quant, self.weight.shape[0])
        self.clamp_config = dict(clamp) if clamp is not None else {'kind': 'identity'}
        self.clamping_fn = self._get_clamper(**self.clamp_config)

        self.quantized_parameters: Dict[str, List[torch.Tensor]] = defaultdict(list)
        if self.bias is not None:
            self.quantized_parameters['fp'].append(self.bias)
        self.quantized_parameters[w_quant].append(self.weight)

        self._hip_cache: Dict[Any, Any] = {}          # packed weights, workspaces (never in state_dict)

    # ------------------------------------------------------------------ factories
    @staticmethod
    def _validate_scheme(scheme: str) -> None:
        if not isinstance(scheme, str) or not _SCHEME_RE.fullmatch(scheme):
            raise ValueError(f'Scheme {scheme} is invalid. Please see docs for valid schemes.')

    @staticmethod
    def _get_x_quantizer(scheme: str, moving_average_mode: str = 'off',
                         moving_average_momentum: float = 0.99) -> nn.Module:
        HipQuantModule._validate_scheme(scheme)
        if scheme == 'fp':
            return quantization.QuantizerFP()
        if scheme.startswith('gf-'):
            return activation_quantization.ActivationQuantizerGF(
                int(scheme[3:]), moving_average_mode, moving_average_momentum)
        cls = {'ls-1': activation_quantization.ActivationQuantizerLS1,
               'ls-2': activation_quantization.ActivationQuantizerLS2,
               'ls-T': activation_quantization.ActivationQuantizerLST}[scheme]
        return cls(moving_average_mode, moving_average_momentum)

    @staticmethod
    def _get_w_quantizer(scheme: str, size: int) -> nn.Module:
        HipQuantModule._validate_scheme(scheme)
        if scheme == 'fp':
            return quantization.QuantizerFP()
        if scheme.startswith('gf-'):
            return weight_quantization.WeightQuantizerGF(size, int(scheme[3:]))
        cls = {'ls-1': weight_quantization.WeightQuantizerLS1,
               'ls-2': weight_quantization.WeightQuantizerLS2,
               'ls-T': weight_quantization.WeightQuantizerLST}[scheme]
        return cls(size)

    @staticmethod
    def _get_clamper(kind: str, alpha: float = 2) -> Callable[[torch.Tensor], torch.Tensor]:
        if kind == 'identity':
            return quantization.clamp_identity
        if kind == 'symmetric':
            return partial(quantization.clamp_symmetric, alpha=alpha)
        raise ValueError(f'{kind} is not a valid clamping function.')

    def _alpha(self) -> float:
        """The symmetric clamp bound, or -1 for the identity."""
        if self.clamp_config.get('kind') == 'symmetric':
            return float(self.clamp_config.get('alpha', 2))
        return -1.0

    def _alpha_in(self, dtype: torch.dtype) -> float:
        """``_alpha()`` as ``Tensor.clamp`` rounds it into a tensor of ``dtype`` (bf16: 1.3 -> 1.296875); -1 stays -1."""
        alpha = self._alpha()
        return float(torch.tensor(alpha, dtype=dtype)) if alpha >= 0 else alpha

    # ------------------------------------------------------------------ invalidation of the derived state
    def _replicate_for_data_parallel(self):
        replica = super()._replicate_for_data_parallel()
        replica._hip_cache = {}           # packed weights / workspaces live on the replica's own device
        return replica

    def train(self, mode: bool = True):
        if mode:
            self._hip_cache.clear()       # weights (and cached scales) may change
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self._hip_cache.clear()
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._hip_cache.clear()
        return super()._apply(fn, *args, **kwargs)

    # ------------------------------------------------------------------ workspaces
    def _workspace(self, kind: str, key: tuple, make: Callable[[], Any]):
        """The workspace ``_hip_cache[(kind,) + key]``, made by ``make()`` on a miss.  A key names one input shape and one
        launch stream (two streams through one module must not share planes and scales); serving with many batch sizes
        must not grow without bound, so a miss first drops all but the three newest entries of ``kind``."""
        key = (kind, *key)
        ws = self._hip_cache.get(key)
        if ws is None:
            ws = make()
            stale = [kk for kk in self._hip_cache if isinstance(kk, tuple) and kk[0] == kind]
            for kk in stale[:max(0, len(stale) - 3)]:
                del self._hip_cache[kk]
            self._hip_cache[key] = ws
        return ws

    def _act_planes(self, x, geom, k, _hip, extra: tuple = (), pre=None, alpha: Optional[float] = None):
        """Quantize ``x`` (the samples of ``geom``) with lsq_act_quant -- a bf16 / fp16 4-D convolution input: with
        lsq_act_quant_half (lsq_act_quant_bn_half where ``pre`` is given); bf16 / fp16 rows [N, L] of a geometry (N, L, 1, 1): with lsq_linear_act_quant_half, or
        lsq_linear_act_quant_solve_half where ls-2 / ls-T have no given scales -- into this module's plane workspace of kind
        ``'act'``; returns (planes, scales).
        ``extra``: what the caller's plane layout depends on beyond ``geom``'s N, C, H, W; ``pre``: a folded batch norm for the
        read; ``alpha``: the clamp bound where it is not ``_alpha()`` (rounded into a 16-bit type)."""
        shape, device = geom.key()[:4], x.device
        n = shape[0]
        planes, scales = self._workspace(
            'act', (shape, *extra, k, device, _hip.stream_ptr(device)),
            lambda: (zero_planes(geom, k, device, _hip), torch.empty((k, n), dtype=torch.float32, device=device)))
        xq = self._modules['x_approximate']     # (read straight from the module's dict: nn.Module.__getattr__ costs a microsecond per launch)
        forced = xq.eval_scales(n)
        if forced is not None:
            forced = forced.to(device=device, dtype=torch.float32).contiguous()
        alpha = self._alpha() if alpha is None else alpha
        if x.dtype == torch.float32:
            _hip.act_quant(x, geom, xq.hip_scheme, k, self.act_skip, alpha, planes, scales, forced, pre)
        elif x.dim() == 4 and pre is not None:  # the same with the eval batch norm in front folded into the read
            _hip.act_quant_bn_half(x, geom, xq.hip_scheme, k, self.act_skip, alpha, planes, scales, forced, pre)
        elif x.dim() == 4:                      # a convolution's 16-bit NCHW input: the convolution's plane layout
            _hip.act_quant_half(x, geom, xq.hip_scheme, k, self.act_skip, alpha, planes, scales, forced)
        elif forced is None and xq.hip_scheme in (_hip.SCHEME_LS2, _hip.SCHEME_LST):
            _hip.linear_act_quant_solve_half(x, xq.hip_scheme, self.act_skip, alpha, planes, scales)
        else:
            _hip.linear_act_quant_half(x, xq.hip_scheme, k, alpha, planes, scales, forced)
        return planes, scales
