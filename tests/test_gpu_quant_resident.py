"""The row-resident form of the single-launch ls-2 / ls-T quantizer (csrc/lsq_act_fused.hip, Impl::run_resident: one read of
the row, its clamped values in registers) against the exact oracle and against the two-read kernel (lsq_debug_fused_mode 16),
on the shapes of tests/golden/resident_shapes.py: the three ResNet-18 row shapes below 56 x 56 -- 7 x 7 x 512 and
14 x 14 x 256 take the resident form, 28 x 28 x 128 keeps the two-read kernel -- and two shorter rows of the same H W on the
other side of the selection.  N = 3: an odd row count, and the last row's tail."""

import functools

import numpy as np
import pytest
import torch

import resident_shapes as RS
from oracle import lsq_exact as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TWO_READ, FALL_BACK = 16, 8                  # lsq_debug_fused_mode bits


def _hip():
    from quant import _hip
    return _hip


def _quantize(x, alpha, ternary, pre=None, mode=0):
    """(planes, scales, chosen sorted positions) of one lsq_act_quant launch."""
    hip = _hip()
    n, c, h, w = x.shape
    geom = hip.make_geom(n, c, h, w, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    planes = torch.zeros((2 * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    scales = torch.empty((2, n), dtype=torch.float32, device=DEV)
    with hip.debug_switches(fused_mode=mode), hip.solver_trace(n, DEV) as trace:
        hip.act_quant(x.to(DEV), geom, hip.SCHEME_LST if ternary else hip.SCHEME_LS2, 2, 3, alpha, planes, scales, None, pre)
        torch.cuda.synchronize()
        pos = trace.cpu().clone()
    return planes.cpu(), scales.cpu(), pos


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(x, folded batch norm scale, shift) of a case: computed once, shared by the tests, never written to."""
    rs = np.random.RandomState(sum(shape))
    n, c, h, w = shape
    x = torch.from_numpy((rs.standard_normal(shape) * 1.3).astype(np.float32))
    sc = torch.from_numpy((0.5 + rs.random_sample(c)).astype(np.float32))
    sh = torch.from_numpy((0.3 * rs.standard_normal(c)).astype(np.float32))
    return x, sc, sh


def _exact_v1(x, sc, sh, alpha, ternary):
    if sc is not None:                       # the kernel's read is ONE fma per element: fp64 product and sum, one rounding
        x = (x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).float()
    return E.solve_rows(x.clamp(-alpha, alpha).reshape(x.shape[0], -1).numpy(), ternary, 3)


@pytest.mark.parametrize('alpha', [2.0, 3.0])
@pytest.mark.parametrize('ternary', [False, True], ids=['ls-2', 'ls-T'])
@pytest.mark.parametrize('shape', RS.CASES, ids=['x'.join(map(str, s)) for s in RS.CASES])
def test_resident_form_equals_the_oracle_and_the_two_read_kernel(shape, ternary, alpha):
    """With and without the folded batch norm: v1 bit-equal to oracle/lsq_exact.solve_rows; planes, v1, v2 and the chosen
    candidate position (lsq_debug_solver_trace) equal to the two-read kernel's; a second launch gives the same bits."""
    x, sc, sh = _inputs(shape)
    for bn in (False, True):
        pre = (sc.to(DEV), sh.to(DEV)) if bn else None
        got_p, got_s, got_pos = _quantize(x, alpha, ternary, pre)
        ref_p, ref_s, ref_pos = _quantize(x, alpha, ternary, pre, mode=TWO_READ)
        exact = _exact_v1(x, sc if bn else None, sh if bn else None, alpha, ternary)
        assert np.array_equal(got_s[0].numpy(), exact), (shape, bn, got_s[0], exact)
        assert torch.equal(got_s, ref_s), (shape, bn, got_s, ref_s)
        assert torch.equal(got_p, ref_p), (shape, bn)
        assert torch.equal(got_pos, ref_pos) and (got_pos >= 0).all(), (shape, bn, got_pos, ref_pos)
        again_p, again_s, again_pos = _quantize(x, alpha, ternary, pre)
        assert torch.equal(again_s, got_s) and torch.equal(again_p, got_p) and torch.equal(again_pos, got_pos), (shape, bn)


def _hard_rows(shape):
    """The rows of test_solver_hard_rows at a case's row length (clamp 3): one value everywhere; a narrow band (one fine bin
    of the window holds thousands of keys that are not a run: the fixed tables refuse it); values far below the clamp (the
    candidates lie below the window); the zeros of a ReLU; and a Gaussian row as the neighbour that does not fall back."""
    rs = np.random.RandomState(7 + shape[1])
    _, c, h, w = shape
    m = c * h * w
    rows = np.stack([np.full(m, 1.75), 1.0 + 1e-4 * rs.standard_normal(m), 1e-5 * rs.standard_normal(m),
                     np.maximum(rs.standard_normal(m), 0), 1.3 * rs.standard_normal(m)]).astype(np.float32)
    return torch.from_numpy(rows.reshape(5, c, h, w))


@pytest.mark.parametrize('ternary', [False, True], ids=['ls-2', 'ls-T'])
@pytest.mark.parametrize('shape', RS.CASES[:3], ids=['x'.join(map(str, s)) for s in RS.CASES[:3]])
def test_hard_rows_through_the_fall_back(shape, ternary):
    """Rows the windowed tables cannot take leave the resident form for the round-2 solve (the narrow and the far-below-the-clamp
    rows by construction; lsq_debug_fused_mode 8 sends every row there): the exact oracle's v1, and the bits of the two-read
    kernel, whichever way a row goes -- and the neighbours of a row that falls back are untouched by it."""
    x = _hard_rows(shape)
    exact = E.solve_rows(x.clamp(-3, 3).reshape(x.shape[0], -1).numpy(), ternary, 3)
    ref_p, ref_s, ref_pos = _quantize(x, 3.0, ternary, mode=TWO_READ)
    assert np.array_equal(ref_s[0].numpy(), exact), (shape, ref_s[0], exact)
    for mode in (0, FALL_BACK):
        got_p, got_s, got_pos = _quantize(x, 3.0, ternary, mode=mode)
        assert torch.equal(got_s, ref_s), (shape, mode, got_s, ref_s)
        assert torch.equal(got_p, ref_p), (shape, mode)
        assert torch.equal(got_pos, ref_pos), (shape, mode, got_pos, ref_pos)
