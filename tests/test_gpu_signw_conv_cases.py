"""lsq_signw_conv2d's general kernels (no prepared weights) on every geometry of tests/golden/conv_half_cases.py with genuinely
fp32 activations.  The fp32 and the 16-bit convolution are one set of kernels (csrc/lsq_signw_conv_core.h) and the table is
the thorough one: together its cases reach all ten kinds of kernel (patch: unit / strided x narrow / wide x up to nine / more
taps; tiled: narrow / wide).  The inputs are not representable in bf16, so the lo plane of the hi + lo split carries weight.

Reference: the fp64 sum written out tap by tap (conv_half_cases.im2col64).  Bound: TOL of tests/test_gpu_planes.py, the 1e-4
of max |y64| that DESIGN 4.4 states for this kernel.  Every test prints the figure it asserts on (pytest -s shows them)."""

import functools

import pytest
import torch

import conv_half_cases as C
import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4
IDS = [c.id for c in C.CASES]
PRE_IDS = ('p1_wide', 's2_narrow')      # a unit-stride and a strided patch case: the two sizes of the folded-batch-norm table


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    """(x fp32, pre-scale, pre-shift) of a case on the CPU, made once."""
    c = C.BY_ID[cid]
    x = detgen.normal(f'signwcases.x.{cid}', (c.N, c.C, c.H, c.W), scale=1.2)
    lo = x - x.bfloat16().float()
    assert x.dtype == torch.float32 and (lo != 0).float().mean() > 0.9          # bf16 does not hold these values
    return x, detgen.uniform(f'signwcases.s.{cid}', (c.C,), 0.5, 1.5), detgen.normal(f'signwcases.t.{cid}', (c.C,), scale=0.3)


@functools.lru_cache(maxsize=None)
def _reference(cid, pre):
    """fp64: the clamped (and, with ``pre``, first scaled and shifted) activations against the quantised weights."""
    c = C.BY_ID[cid]
    x, s, t = _inputs(cid)
    w, _, sc, b = C.weights(cid)
    wq = P.quantize_weight(w, c.ws, sc)
    v = x.double()
    if pre:
        v = v * s.double()[None, :, None, None] + t.double()[None, :, None, None]
    a = C.ALPHAS[c.alpha]
    if a >= 0:
        a32 = float(torch.tensor(a, dtype=torch.float32))                       # the bound as the kernel receives it
        v = v.clamp(-a32, a32)
    return torch.from_numpy(C.im2col64(v.numpy(), wq.double().numpy(), None if b is None else b.double().numpy(), c))


def _check(cid, pre):
    from quant import _hip as hip
    c = C.BY_ID[cid]
    x, s, t = _inputs(cid)
    w, wsc, _, b = C.weights(cid)
    g = hip.make_geom(c.N, c.C, c.H, c.W, c.O, c.KH, c.KW, c.stride, c.pad, c.dil, c.groups)
    wbits, _ = hip.pack_weight(w.to(DEV), g, wsc.to(DEV))
    y64 = _reference(cid, pre)
    y = torch.full(tuple(y64.shape), float('nan'), device=DEV)
    hip.signw_conv2d(x.to(DEV), C.ALPHAS[c.alpha], wbits, wsc.to(DEV), None if b is None else b.to(DEV), g, y,
                     pre=(s.to(DEV), t.to(DEV)) if pre else None)
    err = (y.cpu().double() - y64).abs().max().item()
    scale = y64.abs().max().item()
    print(f'signw fp32 {cid} plan={c.plan} pre={pre} alpha={C.ALPHAS[c.alpha]}: max err / max|y64| = {err / scale:.3e}')
    assert err <= TOL * scale, (cid, err / scale)            # (a NaN left in y fails the comparison)


@pytest.mark.parametrize('cid', IDS)
def test_general_kernels_against_fp64(cid):
    """Every case of the table: where fp32_patch holds the patch kernel of the case's plan, else the tiled one.
    Measured on an MI355X: the worst case is 3.3e-06 of max |y64| (out1x1, the narrow tiled kernel)."""
    assert C.fp32_patch(C.BY_ID[cid]) == bool(C.BY_ID[cid].plan & C.PATCH)
    _check(cid, False)


@pytest.mark.parametrize('cid', PRE_IDS)
def test_general_kernels_with_a_folded_batch_norm(cid):
    c = C.BY_ID[cid]
    assert c.plan & C.PATCH and (c.stride == (1, 1)) == (cid == PRE_IDS[0])
    _check(cid, True)
