"""Inputs and CPU references of the lsq_act_quant_bn_half tests (tests/test_conv_act_bn_half_host.py,
tests/test_gpu_conv_act_bn_half.py): the geometries, batches, clamp bounds, chain and packer are
``conv_act_half_cases``'s; this file adds the per-channel (scale, shift) sets of the folded batch norm and ``folded``, the
torch statement of the tensor the kernel quantizes without writing it."""

import functools

import torch

import detgen
from conv_act_half_cases import (BOUNDS, DTYPES, GEOMS, KERNEL, OUT_CHANNELS, SKIPS, batch, batch_size, chain,  # noqa: F401
                                 clamped32, oracle_rows, pack, plane_shape, rounded)

FOLD_BOUNDS = (-1, 2.0, 0.5)      # none, and two that both types hold (2.0 clamps little, 0.5 about two thirds of a sample)
SETS = ('mixed', 'identity', 'edges', 'overflow')
# the scale that takes x ~ N(0, 1.2) into the subnormal range of the type (bf16: of fp32 as well -- fp32 denormals count)
TINY = {'bf16': 2.0 ** -131, 'fp16': 2.0 ** -19}      # (|x - x0| < 16 stays below the smallest normal, 2^-126 / 2^-14)
OVERFLOW = 6e4                    # fp16: |x| > 1.1 gives |x s| > 65520, which rounds to inf


@functools.lru_cache(maxsize=None)
def params(gi: int, dt: str, which: str):
    """(scale [C], shift [C]) fp32 on the CPU for geometry gi; nothing writes into them.
      mixed     scales of both signs in +-[0.25, 2], shifts in [-1, 1]
      identity  (1, 0)
      edges     mixed, with channel 0 of scale 0 (a constant channel: t = shift) and, where C > 1, channel 1 scaled into the
                type's subnormal range with shift = -(x[0, 1, 0, 0] s): that element cancels to zero, the channel's others
                land on subnormals of the type around it
      overflow  fp16 only: mixed, with the last channel of scale 6e4 -- t overflows to +-inf there (for a clamp bound >= 0)"""
    c = GEOMS[gi][0]
    if which == 'identity':
        return torch.ones(c), torch.zeros(c)
    mag = detgen.uniform(f'convactbnhalf.s.{gi}', (c,), 0.25, 2.0, seed=gi)
    sign = torch.where(detgen.uniform(f'convactbnhalf.sign.{gi}', (c,), seed=gi) < 0.5, -1.0, 1.0)
    if c > 1:
        sign[:2] = torch.tensor([1.0, -1.0])          # (both signs whatever the draw)
    scale, shift = mag * sign, detgen.uniform(f'convactbnhalf.b.{gi}', (c,), -1.0, 1.0, seed=gi)
    if which == 'edges':
        scale[0] = 0.0
        if c > 1:
            scale[1] = TINY[dt]
            shift[1] = -(batch(gi, dt)[0, 1, 0, 0].float() * scale[1])
    elif which == 'overflow':
        assert dt == 'fp16'
        scale[-1] = OVERFLOW
    else:
        assert which == 'mixed', which
    return scale.contiguous(), shift.contiguous()


def folded(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """The contract's t of include/lsq_hip_conv_act_bn_half.h: two fp32 operations, one rounding into x's type."""
    return (x.float() * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).to(x.dtype)


@functools.lru_cache(maxsize=None)
def folded_batch(gi: int, dt: str, which: str, n: int = 0) -> torch.Tensor:
    """folded(batch(gi, dt, n), *params(gi, dt, which)) on the CPU: computed once, shared, left unchanged."""
    return folded(batch(gi, dt, n), *params(gi, dt, which))
