"""tests/golden/chain_fixed_cases.py on the host (no GPU): the case table is self-consistent, the CPU model's planes are the
signs of quant.binary's torch quantizers with the same given scales, and ``NextFixed`` mirrors ``lsq_next_fixed``."""

import ctypes
import os
import re

import pytest
import torch

import chain_fixed_cases as FC
from quant import _sublibs
from quant.binary import quantization

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_case_table_is_self_consistent():
    assert len(FC.BY_ID) == len(FC.CASES)
    for c in FC.CASES:
        ho, wo = FC.out_hw(c)
        d = FC.inputs(c.id)
        assert c.C in (64, 128, 256, 512) and c.O % 64 == 0 and c.kx in (1, 2) and 1 <= c.k <= 8
        assert FC.SCHEMES[c.scheme][1] in (None, c.k)
        assert d['xs'].shape == (c.kx, c.N) and d['scales'].shape == (c.k, c.N) and d['wscales'].shape == (c.wplanes, c.O)
        assert (d['s'] is not None) == c.affine and (d['res_post'] is not None) == c.res_post
        assert bool((d['scales'] > 0).all()) and (c.N == 1 or bool((d['scales'][:, 0] != d['scales'][:, 1]).all()))
        if d['res_post'] is not None:
            assert d['res_post'].shape == (c.N, c.O, ho, wo)
    two = FC.BY_ID['two_samples']
    assert 32 % (FC.out_hw(two)[0] * FC.out_hw(two)[1]) != 0 and FC.out_hw(two)[0] * FC.out_hw(two)[1] < 32     # a tile spans both samples
    big = FC.BY_ID['two_tiles_per_wave']
    assert (big.N * 56 * 56 + 31) // 32 > 128 * 12                      # more tiles than the grid has waves per out-channel tile


@pytest.mark.parametrize('scheme,k', [('ls-1', 1), ('ls-2', 2), ('ls-T', 2), ('gf', 3), ('gf', 8)])
def test_the_model_gives_the_torch_quantizers_signs(scheme, k):
    g = torch.Generator().manual_seed(k)
    x = (torch.randn((3, 64, 4, 5), generator=g) * 1.6).clamp(-2, 2)
    x[0, 0, 0, :2] = torch.tensor([0.0, -0.0])
    first = torch.tensor([1.1, 0.9, 1.3])
    scales = torch.stack([first * 0.5 ** (0 if scheme == 'ls-T' else p) for p in range(k)])
    bits = [torch.from_numpy(b) for b in FC.model_bits(x, None, None, 2.0, scales)]
    rebuilt = sum(v.view(-1, 1, 1, 1) * torch.where(b, 1.0, -1.0) for v, b in zip(scales, bits))
    if scheme == 'ls-1':
        xq = quantization.quantizer_ls_1(x, scales[0])[1]
    elif scheme == 'ls-2':
        xq = quantization.quantizer_ls_2(x, scales[0], scales[1])[2]
    elif scheme == 'ls-T':
        xq = quantization.quantizer_ls_ternary(x, scales[0])[1]
    else:
        xq = quantization.quantizer_gf(x, k, list(scales))[1].reshape(x.shape)
    # halving (or, ternary, equal) scales: the quantized value names its signs, so equal values are equal planes
    assert torch.allclose(xq, rebuilt, rtol=0, atol=1e-6)
    assert bool(bits[0][0, 0, 0, 0]) and bool(bits[0][0, 0, 0, 1])       # +-0: sign +1


def test_next_fixed_mirrors_the_header():
    with open(os.path.join(ROOT, 'include', 'lsq_hip_conv_chain.h')) as f:
        body = re.search(r'typedef struct lsq_next_fixed \{(.*?)\} lsq_next_fixed;', re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S),
                         flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        ctype, names = re.fullmatch(r'(.*?)\s*(\w+(?:\s*,\s*\w+)*)', decl, flags=re.S).groups()
        for name in re.split(r'\s*,\s*', names):
            fields.append((name, ctypes.c_void_p if '*' in ctype else {'int32_t': ctypes.c_int32, 'float': ctypes.c_float}[ctype]))
    assert fields == list(_sublibs.NextFixed._fields_)
    assert ctypes.sizeof(_sublibs.NextFixed) == 56
