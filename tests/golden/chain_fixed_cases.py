"""Cases, inputs and the CPU model of the lsq_xnor_conv2d_chain_fixed tests (tests/test_chain_fixed_host.py,
tests/test_gpu_chain_fixed.py): the next layer's quantizer with GIVEN per-sample scales in the producing convolution's epilogue
(include/lsq_hip_conv_chain.h; csrc/lsq_xnor_mfma.hip, NQF).

The model restates the epilogue's arithmetic on a given fp32 ``y [N,O,Ho,Wo]`` and is exact:
  * ``c = fp32(fp64(y) * fp64(s) + fp64(t))`` with a folded batch norm (the product of two fp32 numbers is exact in fp64: one
    rounding of the sum, as fmaf), else ``c = y``; then the clamp in fp32 (none with a negative alpha);
  * plane p: ``bit_p = (c - result_p) >= 0`` (-0.0 gives 1), ``result_0 = 0``, ``result_{p+1} = result_p + (bit_p ? v_p : -v_p)``
    in torch fp32 -- the result chain of lsq_act_quant's sweeps (csrc/lsq_act_quant.hip, chain_eval; quantizer_gf's ``approx``).
    For p <= 1 ``c - result_p`` is the residual itself; from p = 2 on the residual ``(c -+ v_0) -+ v_1`` rounds differently from
    ``c - (+-v_0 +- v_1)``, and it is the latter that decides the bit in lsq_act_quant and here;
  * words packed like ``chain_cases.model_words``.
Every decision is a comparison of fp32 values: the planes are required bit-equal, no element exempt."""

import collections
import functools
import math

import numpy as np
import torch

import chain_cases as CC
import detgen

SCHEMES = {'ls-1': (1, 1), 'ls-2': (2, 2), 'ls-T': (3, 2), 'gf': (4, None)}       # name -> (LSQ_SCHEME_*, planes)

# id, N, C, O, H, W, stride, pad, kx (producer planes), consumer scheme, k, the consumer's padding, alpha (< 0: identity),
# folded batch norm, act (none | prelu), res_post, weight planes
FCase = collections.namedtuple('FCase', 'id N C O H W stride pad kx scheme k next_pad alpha affine act res_post wplanes')
CASES = (
    FCase('two_samples', 2, 64, 64, 5, 5, 1, 1, 1, 'ls-2', 2, (1, 1), 2.0, False, 'none', False, 1),
    FCase('bn_prelu_res', 2, 64, 64, 5, 5, 1, 1, 1, 'ls-2', 2, (1, 1), 2.0, True, 'prelu', True, 2),
    FCase('kx2_s2_lsT', 1, 128, 128, 9, 9, 2, 1, 2, 'ls-T', 2, (0, 0), 2.0, False, 'none', False, 1),
    FCase('g4', 1, 256, 64, 4, 4, 1, 1, 1, 'ls-2', 2, (1, 1), 2.0, False, 'none', False, 1),
    FCase('g8', 1, 512, 64, 4, 4, 1, 1, 2, 'ls-2', 2, (1, 1), 2.0, True, 'none', False, 1),
    FCase('k1', 2, 64, 64, 5, 5, 1, 1, 1, 'ls-1', 1, (1, 1), 2.0, False, 'none', False, 1),
    FCase('k3', 2, 64, 64, 5, 5, 1, 1, 2, 'gf', 3, (1, 1), 2.0, False, 'none', False, 1),
    FCase('k8', 2, 64, 64, 5, 5, 1, 1, 2, 'gf', 8, (2, 1), 2.0, True, 'none', False, 1),
    FCase('identity', 2, 64, 64, 5, 5, 1, 1, 1, 'ls-2', 2, (1, 1), -1.0, False, 'none', False, 1),
    FCase('anchor', 2, 64, 64, 5, 5, 1, 1, 1, 'gf', 3, (1, 1), 2.0, False, 'none', False, 1),
    FCase('two_tiles_per_wave', 16, 64, 64, 56, 56, 1, 1, 1, 'ls-2', 2, (1, 1), 2.0, False, 'none', False, 1),
)
BY_ID = {c.id: c for c in CASES}


def out_hw(c: FCase):
    return (c.H + 2 * c.pad - 3) // c.stride + 1, (c.W + 2 * c.pad - 3) // c.stride + 1


def _duck(c: FCase):
    """``c`` with the attribute names chain_cases.epilogue64 reads."""
    ho, wo = out_hw(c)
    return collections.namedtuple('Duck', 'N O Ho Wo act')(c.N, c.O, ho, wo, c.act)


@functools.lru_cache(maxsize=None)
def inputs(cid: str) -> dict:
    """CPU tensors of a case (nothing writes into them): x, xs [kx, N] (the producer's own given scales), w, wscales
    [wplanes, O], bias, slope, res_post, s, t, and the consumer's scales [k, N] -- different from sample to sample.  The value
    in front of the consumer's clamp gets a standard deviation of about 0.8 |alpha|."""
    c = BY_ID[cid]
    tag = f'chain_fixed.{cid}'
    g = torch.Generator().manual_seed(sum(map(ord, cid)))
    ho, wo = out_hw(c)
    target = 0.8 * abs(c.alpha)
    sigma = 1.0 if c.affine else target
    conv_std = sigma * math.sqrt(1.0 - (0.16 if c.res_post else 0.0))
    x = detgen.normal(tag + '.x', (c.N, c.C, c.H, c.W), scale=1.0)
    xs = torch.stack([(0.8 * 0.5 ** p) * (1.0 + 0.1 * torch.rand((c.N,), generator=g)) for p in range(c.kx)]).contiguous()
    gain = math.sqrt(sum(4.0 ** -q for q in range(c.wplanes)) * sum(0.64 * 4.0 ** -p for p in range(c.kx)))
    ws0 = detgen.uniform(tag + '.ws', (c.O,), 0.8, 1.2) * (conv_std / (math.sqrt(c.C * 7.0) * gain))
    d = {'x': x, 'xs': xs, 'w': (detgen.normal(tag + '.w', (c.O, c.C, 3, 3), scale=1.2) * ws0.view(-1, 1, 1, 1)).contiguous(),
         'wscales': torch.stack([ws0 * 0.5 ** q for q in range(c.wplanes)]).contiguous(),
         'bias': detgen.normal(tag + '.bias', (c.O,), scale=0.1 * sigma), 'slope': None, 'res_pre': None, 'res_post': None,
         's': None, 't': None}
    if c.act == 'prelu':
        d['slope'] = torch.tensor([0.25])
    if c.res_post:
        d['res_post'] = detgen.normal(tag + '.res_post', (c.N, c.O, ho, wo), scale=0.4 * sigma)
    if c.affine:
        s = detgen.uniform(tag + '.s', (c.O,), 0.8, 1.2) * (1.5 * target)       # (a good part of the values beyond the clamp)
        s[1::3] *= -1.0
        d['s'], d['t'] = s.contiguous(), detgen.normal(tag + '.t', (c.O,), scale=0.1 * target)
    first = target * 0.8 * (1.0 + 0.25 * torch.arange(c.N, dtype=torch.float32) + 0.05 * torch.rand((c.N,), generator=g))
    d['scales'] = torch.stack([first * 0.5 ** p for p in range(c.k)]).contiguous()
    return d


def input_signs(x: torch.Tensor, xs: torch.Tensor):
    """The producer's own input planes for given scales ``xs`` [kx, N] (kx <= 2, clamp ALPHA_IN): +-1 tensors in fp64."""
    xc = x.clamp(-CC.ALPHA_IN, CC.ALPHA_IN)
    b0 = torch.where(xc >= 0, 1.0, -1.0)
    out = [b0.double()]
    if xs.shape[0] == 2:
        out.append(torch.where(xc - xs[0].view(-1, 1, 1, 1) * b0 >= 0, 1.0, -1.0).double())
    return out


@functools.lru_cache(maxsize=None)
def reference(cid: str) -> torch.Tensor:
    """y of the case in fp64 on the CPU (computed once, shared, left unchanged)."""
    c, d = BY_ID[cid], inputs(cid)
    acc = 0
    for xb, xsp in zip(input_signs(d['x'], d['xs']), d['xs']):
        for u, sq in zip(d['wscales'], CC.weight_signs(d['w'], d['wscales'])):
            ints = torch.nn.functional.conv2d(xb, sq, None, c.stride, c.pad)
            acc = acc + ints * u.double().view(1, -1, 1, 1) * xsp.double().view(-1, 1, 1, 1)
    return CC.epilogue64(_duck(c), d, acc)


def pre_quant(y, s, t, alpha: float) -> torch.Tensor:
    """fp32 [N,O,Ho,Wo]: the value the planes are cut from."""
    c = torch.as_tensor(y, dtype=torch.float32)
    if s is not None:
        c = (c.double() * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1)).float()
    if alpha > 0:
        a = float(np.float32(alpha))
        c = c.clamp(-a, a)
    return c


def model_bits(y, s, t, alpha: float, scales: torch.Tensor):
    """[k] bool arrays [N,O,Ho,Wo]: the planes the epilogue writes for fp32 y and scales [k, N]."""
    c = pre_quant(y, s, t, alpha)
    result, out = torch.zeros_like(c), []
    for v in scales.float():
        bit = (c - result) >= 0
        out.append(bit.numpy())
        vv = v.view(-1, 1, 1, 1).expand_as(c)
        result = result + torch.where(bit, vv, -vv)
    return out


def model_words(y, s, t, alpha: float, scales: torch.Tensor, next_pad) -> np.ndarray:
    """uint64 [k, N, O/64, Ho + 2 ph, Wo + 2 pw]: the consumer's planes, halo zero."""
    return np.stack([CC.model_words(b, next_pad) for b in model_bits(y, s, t, alpha, scales)])


def anchor_scales(c: torch.Tensor, scales: torch.Tensor):
    """``scales`` [3, N] with sample 0's v_1 = |c[e]| and v_2 chosen so that element f's residual in front of plane 3 is
    exactly zero: (scales, e, f), e and f index sample 0 of ``c`` [N,O,Ho,Wo] flat.  |c[f]| is within a factor of two of v_1, so
    c[f] -+ v_1 is exact (Sterbenz) and +-v_1 + (c[f] -+ v_1) gives c[f] back."""
    flat = c[0].reshape(-1)
    mags = flat.abs()
    e = int(torch.argsort(mags)[mags.numel() // 2])                     # a median magnitude: not clamped, not tiny
    v1 = mags[e]
    ok = (mags > 0.55 * v1) & (mags < 1.9 * v1) & (mags != v1)
    f = int(torch.nonzero(ok)[0])
    r1 = flat[f] - torch.where(flat[f] >= 0, v1, -v1)
    out = scales.clone()
    out[0, 0], out[1, 0] = v1, r1.abs()
    return out, e, f
