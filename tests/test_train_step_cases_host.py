"""tests/golden/train_step_cases.py on the host (no GPU): the fp64 reference of QuantConv2d's train step against fp32 autograd
through the torch formulation of the module (the graph the f9_train fixture pins to the reference), for every case of the
table, and the conditions the table itself must meet.  This is what makes ``step64`` trustworthy before a kernel enters
(tests/test_gpu_train_geometries.py)."""

import pytest
import torch

import train_step_cases as T

TOL = 1e-5            # fp32 reassociation only: DESIGN 4.7's figure for this step against the reference fixture


def _rel(a, b64):
    return float((a.detach().double() - b64).abs().max() / b64.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('case', T.CASES, ids=lambda c: c.id)
def test_step64_equals_fp32_autograd_through_the_torch_formulation(case):
    d = T.inputs(case.id)
    conv = T.make_module(case)
    x = d['x'].clone().requires_grad_()
    y = conv(x)
    assert type(y.grad_fn).__name__ != '_QuantConv2dStepBackward'
    assert tuple(y.shape) == tuple(d['gy'].shape)
    y.backward(d['gy'])
    wscales = list(conv.w_approximate.plane_scales())                       # cached by the step (train mode)
    assert len(wscales) == T.planes(case.ws) and float(wscales[0].abs().min()) > 0
    xscales = T.act_scales_cpu(case, d['x'])                                # what the quantizer used: scales come from detached data
    assert len(xscales) == T.planes(case.xs)
    ref = T.step64(d['x'], d['w'], d['b'], d['gy'], xscales, wscales, T.alpha_of(case.clamp), case.stride, (case.pad_h, case.pad_w))
    got = {'y': y, 'gx': x.grad, 'gw': conv.weight.grad}
    if case.bias:
        got['gb'] = conv.bias.grad
    for name, t in got.items():
        assert t.shape == ref[name].shape, name
        err = _rel(t, ref[name])
        assert err <= TOL, (case.id, name, err)
    # the magnitudes of the GPU test's bounds: m is the estimator as a multiplier, and a closed mask or an unread position
    # leaves a bound of exactly 0
    assert torch.equal(ref['m_x'] * ref['gxq'], ref['gx']) or _rel(ref['m_x'] * ref['gxq'], ref['gx']) <= 1e-14
    assert _rel(ref['m_w'] * ref['gwq'], ref['gw']) <= 1e-14
    assert bool((ref['gxq'].abs() <= ref['mag_x'] * (1 + 1e-12)).all()) and bool((ref['gwq'].abs() <= ref['mag_w'] * (1 + 1e-12)).all())
    ur, uc = T.unread(case)
    if ur:
        assert float(ref['mag_x'][:, :, case.H - ur:, :].abs().max()) == 0.0 and float(x.grad[:, :, case.H - ur:, :].abs().max()) == 0.0
    if uc:
        assert float(ref['mag_x'][:, :, :, case.W - uc:].abs().max()) == 0.0 and float(x.grad[:, :, :, case.W - uc:].abs().max()) == 0.0


def _accepted(c) -> bool:
    """The geometry clauses of ``hip_train.supported`` and the limits of the kernels behind it (include/lsq_hip_train.h,
    ``QuantConv2d._hip_supports``), restated: groups 1 and dilation 1 (the table has neither), one stride of 1 or 2, padding
    at most k - 1 per axis, N and O up to 65535, binary weights of 1 .. 8 planes; binary activations: at most 8 planes, kernels
    up to 8 x 8, fewer than 2^22 sub-sampled keys per row for the ls-2 / ls-T solve."""
    ho, wo = T.out_hw(c)
    ok = c.stride in (1, 2) and 0 <= c.pad_h <= c.KH - 1 and 0 <= c.pad_w <= c.KW - 1 and ho >= 1 and wo >= 1
    ok = ok and 1 <= c.N <= 65535 and 1 <= c.O <= 65535 and c.ws != 'fp' and 1 <= T.planes(c.ws) <= 8
    if c.xs != 'fp':
        ok = ok and T.planes(c.xs) <= 8 and max(c.KH, c.KW) <= 8
        if c.xs in ('ls-2', 'ls-T'):
            ok = ok and (c.C * c.H * c.W + 2) // 3 < (1 << 22)
    return ok


def test_the_table_is_what_the_gpu_tests_need():
    ids = [c.id for c in T.CASES]
    assert len(set(ids)) == len(ids)
    assert 16 <= len(ids) <= 20
    present = set()
    for c in T.CASES:
        assert _accepted(c), c.id
        assert c.O * c.C * c.KH * c.KW <= 100_000 and c.H * c.W <= 1040 and c.N <= 3, c.id       # tiny inputs
        present |= T.kinds(c)
    assert set(T.REQUIRED_KINDS) <= present, set(T.REQUIRED_KINDS) - present
    # schemes: every activation scheme over every weight scheme family, the bare transposed convolutions, bias on about half
    assert {c.xs for c in T.CASES} == {'fp', 'ls-1', 'ls-2', 'ls-T', 'gf-2'}
    assert {c.ws for c in T.CASES} == {'ls-1', 'ls-2', 'ls-T', 'gf-3'}
    assert any(c.xs == 'fp' and c.clamp['kind'] == 'symmetric' for c in T.CASES)
    assert 0.4 <= sum(c.bias for c in T.CASES) / len(ids) <= 0.6
    # every kernel of the transposed role: patch narrow / wide, few / many taps, tiled narrow / wide
    reached = {T.transposed_kernel(c) for c in T.CASES}
    assert {('patch', False, False), ('patch', True, False), ('patch', False, True), ('patch', True, True)} <= reached
    assert {(k, w) for k, w, _ in reached} >= {('tiled', False), ('tiled', True)}


def test_the_inputs_hold_the_edge_values():
    """+-0, the clamp bound itself, |d| = 1 of the first sign everywhere, and of the second sign in sample 0 of at least one
    case with two or more activation planes (exactly, with the scales of the torch formulation)."""
    hit_second = 0
    for c in T.CASES:
        x = T.inputs(c.id)['x']
        alpha = T.alpha_of(c.clamp)
        assert bool((x == 0).any()) and bool(((x == 0) & torch.signbit(x)).any()), c.id
        assert bool((x.abs() == 1).any()), c.id
        if alpha >= 0:
            assert bool((x == alpha).any()) and bool((x == -alpha).any()), c.id
        if T.planes(c.xs) >= 2:
            v1 = T.act_scales_cpu(c, x)[0][0]
            xc = x[0].clamp(-alpha, alpha)
            d2 = xc - v1 * torch.where(xc >= 0, 1.0, -1.0)
            hit_second += int(bool((d2.abs() == 1).any()))
    assert hit_second >= 1


def test_chain64_decides_in_fp32_and_computes_in_fp64():
    """The same decisions as ``chain`` (its value rounds to chain's within an ulp of the largest partial sum), a gradient that
    is the multiplier m applied to g, and an edge |d| = 1 that is open."""
    x = torch.tensor([[0.0, -0.0, 1.0, -1.0, 1.75, 2.0, -2.0, 2.5, 0.3]], dtype=torch.float32)
    scales = [torch.tensor([0.75]), torch.tensor([0.4])]
    v32, g32 = T.chain(x, scales, 2.0)
    v64, g64 = T.chain64(x, scales, 2.0)
    assert torch.allclose(v64.float(), v32, rtol=0, atol=1e-6)
    g = torch.arange(1.0, 10.0).view(1, -1)
    assert torch.allclose(g64(g.double()).float(), g32(g), rtol=1e-6, atol=0)
    m = g64(torch.ones(1, 9, dtype=torch.float64))
    assert float(m[0, 7]) == 0.0                                              # outside the clamp
    assert float(m[0, 2]) == pytest.approx(0.4 + 0.6 * 0.75)                  # x = 1: |d_1| = 1 exactly (open), |d_2| = 0.25
    assert float(m[0, 4]) == pytest.approx(0.4)                               # x = 1.75: |d_1| > 1 (closed), d_2 = 1 exactly (open)
    assert float(m[0, 5]) == 0.0                                              # x = 2 (on the clamp: inside), |d_1| = 2, |d_2| = 1.25
