"""lsq_train_wgrad (fp32 grad_y) on the mechanism cases of tests/golden/train_wgrad_half_cases.py, and against
lsq_train_wgrad_half on the same operands.  The two kernels take the tiles, the K split, the reduce kernel and the host rules from one
header (csrc/train/lsq_wgrad_core.h) and keep the same sign-word steps in line, each in its own text: the first test runs the fp32
kernel through the shapes that so far only the 16-bit one saw (8 x 8 taps in eight tap tiles, eight planes, Ho Wo = 1, samples of
49 and 81 positions), the others fail when a shared piece is specialised wrongly for one side or a step is changed in one file
alone."""

import pytest
import torch

import detgen
import train_wgrad_half_cases as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _hip():
    from quant import _hip
    return _hip


def _geom(c):
    return _hip().make_geom(c.N, c.C, c.H, c.W, c.O, c.k[0], c.k[1], (c.stride, c.stride), c.pad, (1, 1), 1)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_OPERANDS = {}


def _operands(c):
    """Planes and scales of a case from lsq_act_quant, and x_q in fp64: computed once, left unchanged."""
    if c.id not in _OPERANDS:
        hip = _hip()
        geom = _geom(c)
        code, k = T.SCHEMES[c.scheme]
        x = detgen.normal(f'wgc.x.{c.id}', (c.N, c.C, c.H, c.W), scale=1.3)
        planes = torch.zeros((k * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
        scales = torch.empty((k, c.N), dtype=torch.float32, device=DEV)
        hip.act_quant(x.to(DEV), geom, code, k, 3, 2.0, planes, scales)
        torch.cuda.synchronize()
        _OPERANDS[c.id] = dict(geom=geom, k=k, planes=planes, scales=scales, xq=T.xq64(T.unpack_planes(planes, k, c), scales))
    return _OPERANDS[c.id]


@pytest.mark.parametrize('c', T.MECHANISMS, ids=lambda c: c.id)
def test_the_fp32_kernel_equals_the_fp64_closed_form_on_the_mechanism_cases(c):
    """fp32 grad_y that bf16 does not hold (the mid and lo terms carry weight); the bound of tests/test_gpu_wgrad.py per element,
    and an exact 0 where sum |gy| |x_q| is 0."""
    hip = _hip()
    ops = _operands(c)
    gy = detgen.normal(f'wgc.gy.{c.id}', (c.N, c.O) + T.out_hw(c)) * 0.25
    assert gy.dtype == torch.float32 and float((gy.to(torch.bfloat16).float() != gy).float().mean()) > 0.9
    ref = T.closed_form(c, ops['xq'], gy)
    g = hip.wgrad(ops['planes'], ops['k'], ops['scales'], gy.to(DEV), ops['geom'])
    torch.cuda.synchronize()
    assert g.dtype == torch.float32 and tuple(g.shape) == (c.O, c.C) + c.k
    err = (g.cpu().double() - ref['g']).abs()
    ratio = float((err / (T.BOUND * ref['mag'] + 1e-30)).max())
    print(f'\nwgrad-cases fp32 {c.id}: {ratio:.4f} of the bound')
    assert bool((err <= T.BOUND * ref['mag'] + 1e-30).all()), (c.id, ratio)
    assert bool((g.cpu()[ref['mag'] == 0] == 0).all()), (c.id, 'exact zeros')


@pytest.mark.parametrize('c', T.MECHANISMS, ids=lambda c: c.id)
@pytest.mark.parametrize('dtype', T.DTYPES, ids=lambda t: T.DTYPE_NAMES[t])
def test_the_two_kernels_agree_on_a_16_bit_gradient(c, dtype):
    """The same planes, scales and (16-bit) grad_y: each kernel is within BOUND * sum |gy| |x_q| of the same fp64 value, so they
    are within twice that of each other -- and both are 0 where that magnitude is 0."""
    hip = _hip()
    ops = _operands(c)
    gy = (detgen.normal(f'wgc.gy16.{c.id}', (c.N, c.O) + T.out_hw(c)) * 0.25).to(dtype)
    mag = T.closed_form(c, ops['xq'], gy.float())['mag']
    g32 = hip.wgrad(ops['planes'], ops['k'], ops['scales'], gy.float().to(DEV), ops['geom'])
    g16, _ = hip.wgrad_half(ops['planes'], ops['k'], ops['scales'], gy.to(DEV), ops['geom'])
    torch.cuda.synchronize()
    diff = (g32.cpu().double() - g16.cpu().double()).abs()
    ratio = float((diff / (2 * T.BOUND * mag + 1e-30)).max())
    print(f'\nwgrad-cases fp32 vs {T.DTYPE_NAMES[dtype]} {c.id}: {ratio:.4f} of twice the bound')
    assert bool((diff <= 2 * T.BOUND * mag + 1e-30).all()), (c.id, ratio)
    zero = mag == 0
    assert bool((g32.cpu()[zero] == 0).all()) and bool((g16.cpu()[zero] == 0).all())


@pytest.mark.parametrize('c', T.ANCHORS, ids=lambda c: c.id)
@pytest.mark.parametrize('dtype', T.DTYPES, ids=lambda t: T.DTYPE_NAMES[t])
def test_the_two_kernels_are_bit_equal_on_integer_operands(c, dtype):
    """gy = m / 8 with m in [-8, 8], scales powers of two that differ per sample and plane, random bits: scale * gy is one bf16
    term, every partial sum of either kernel an integer multiple of 2^-7 below 2^24 -- both are exact, hence bit-equal."""
    hip = _hip()
    k = T.kx_of(c)
    gen = torch.Generator().manual_seed(len(c.id) + 17 * c.C + c.O)
    bits = torch.randint(0, 2, (k, c.N, c.C, c.H, c.W), generator=gen)
    gy = torch.randint(-8, 9, (c.N, c.O) + T.out_hw(c), generator=gen).float() / 8
    scales = torch.tensor([[2.0 ** -((n + 2 * p) % 5) for n in range(c.N)] for p in range(k)])
    ref = T.closed_form(c, T.xq64(bits, scales), gy)
    assert float(ref['mag'].max()) * 128 < 2 ** 24 and torch.equal(gy.to(dtype).float(), gy)
    planes = T.pack_planes(bits, c.pad).to(DEV)
    g32 = hip.wgrad(planes, k, scales.to(DEV), gy.to(DEV), _geom(c))
    g16, _ = hip.wgrad_half(planes, k, scales.to(DEV), gy.to(dtype).to(DEV), _geom(c))
    torch.cuda.synchronize()
    assert _bits_equal(g32, g16), int((g32 != g16).sum())
    assert torch.equal(g32.cpu().double(), ref['g'])
