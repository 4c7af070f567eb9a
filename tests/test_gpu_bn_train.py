"""The kernels of liblsq_hip_bn_train.so (include/lsq_hip_bn_train.h) against their contracts, on the cases of
tests/golden/bn_train_cases.py: the statistics against torch in fp64, the fold against the quantizer's own, the quantized
values and the backward against the unfused kernels and fp64 closed forms, run-to-run bit equality and the refusals.

Bounds (u = 2^-53, m = N H W): a mean or a sum is one fp32 rounding of its fp64 value plus the fp64 summation term, m u times
the mean (the sum) of the terms' magnitudes -- the header derives it; grad_x is nine fp32 roundings of the magnitudes of its
three terms (eight in the kernel's expression, counted in the header, plus one).  None of them is a measured figure."""

import numpy as np
import pytest
import torch

import bn_train_cases as B
import detgen

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U24, U53 = 2.0 ** -24, 2.0 ** -53
GRAD_X_ROUNDINGS = 9
SCHEME_K = {'ls-1': 1, 'ls-2': 2, 'ls-T': 2, 'gf-3': 3, 'fp': 0}
CASE_PARAMS = [pytest.param(c, id=c.id) for c in B.CASES]


def _hip():
    from quant import _hip
    return _hip


def _scheme_id(scheme):
    hip = _hip()
    return {'ls-1': hip.SCHEME_LS1, 'ls-2': hip.SCHEME_LS2, 'ls-T': hip.SCHEME_LST, 'gf-3': hip.SCHEME_GF}[scheme]


# ------------------------------------------------------------------------------------------------------------- inputs
def _place(case, flat_cpu):
    """``flat_cpu`` [N C H W] on the device as the case's x: contiguous, ``offset`` floats behind a 16-byte boundary."""
    n = flat_cpu.numel()
    big = torch.zeros((n + 8,), dtype=torch.float32, device=DEV)
    assert big.data_ptr() % 16 == 0
    x = big[case.offset:case.offset + n].view(case.N, case.C, case.H, case.W)
    x.copy_(flat_cpu.view(x.shape))
    assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == (case.offset == 0)
    return x


def _fold(case):
    """(scale, shift) [C] of powers of two and quarters, so that fmaf(x, scale, shift) is exact on dyadic x; with gamma = 1
    and beta = 0 they are the batch norm of mean = -shift / scale and invstd = scale."""
    c = torch.arange(case.C)
    scale = torch.tensor([0.5, 2.0, 1.0, 0.25])[c % 4]
    shift = torch.tensor([0.5, -0.25, 0.0, 1.0, -1.5])[c % 5]
    return scale, shift


def _plane_scales(case, k, dyadic=True):
    """[k, N] plane scales: v_i[n] = 2^-i (1 + (n % 2) / 4), or generic positive values."""
    if k == 0:
        return None
    if dyadic:
        n = torch.arange(case.N, dtype=torch.float32)
        return torch.stack([2.0 ** -i * (1.0 + (n % 2) * 0.25) for i in range(k)])
    return detgen.uniform(f'bnt.{case.id}.v', (k, case.N), 0.2, 1.1)


def _x_for_fold(case, k):
    """x whose folded value fmaf(x, scale, shift) is exactly +0, +-alpha, +-1 (the first sign's estimator edge) and, with two
    planes or more, v_1 + 1 in sample 0 (the second sign's edge under the dyadic plane scales), among generic values; channel 0
    is constant.  Built from the targets: x = (target - shift) / scale is exact for power-of-two scales."""
    scale, shift = _fold(case)
    x = detgen.normal(f'bnt.{case.id}.x', (case.N, case.C, case.H, case.W), scale=1.2)
    x += (torch.arange(case.C, dtype=torch.float32) % 3 - 1).view(1, -1, 1, 1) * 0.5
    sc, sh = scale.view(1, -1, 1, 1).expand_as(x).reshape(-1), shift.view(1, -1, 1, 1).expand_as(x).reshape(-1)
    flat = x.view(-1)
    targets = [(0, 7, 0.0), (2, 11, 1.0), (4, 13, -1.0)]
    if case.alpha >= 0:
        targets += [(1, 5, case.alpha), (3, 9, -case.alpha)]
    if k >= 2:
        targets.append((6, 17, 2.0))                    # v_1[0] = 1 in sample 0: d_2 = 2 - 1 = 1
    placed = torch.full_like(flat, float('nan'))
    for start, step, target in targets:
        idx = torch.arange(start, flat.numel(), step)
        if target == 2.0:
            idx = idx[idx < flat.numel() // case.N]
        flat[idx] = (target - sh[idx]) / sc[idx]
        placed[idx] = target
    x[:, 0] = 0.75
    placed.view(x.shape)[:, 0] = float('nan')
    y = _fold64(flat, sc, sh)
    at = ~placed.isnan()
    assert bool((y[at] == placed[at].double()).all())                 # the fold lands on the targets exactly
    for _, _, target in targets:
        assert int((placed == target).sum()) > 0 or flat.numel() < 40, (case.id, target)
    return x.view(-1)


def _fold64(x, scale, shift):
    """fmaf(x, scale, shift) for power-of-two scales, in fp64 (the product is exact, the sum is below 53 bits here)."""
    return x.double() * scale.double() + shift.double()


def _x_for_stats(case):
    """Generic x with a channel-dependent offset and spread; channel 0 constant (var = 0)."""
    x = detgen.normal(f'bnt.{case.id}.xs', (case.N, case.C, case.H, case.W), scale=1.0)
    c = torch.arange(case.C, dtype=torch.float32).view(1, -1, 1, 1)
    x = x * (0.25 + (c % 5) * 0.5) + (c % 7 - 3.0) * 0.75
    x[:, 0] = 0.75
    return x.reshape(-1)


def _affine(case):
    if not case.affine:
        return None, None
    return (detgen.uniform(f'bnt.{case.id}.gamma', (case.C,), 0.5, 1.5).to(DEV),
            detgen.normal(f'bnt.{case.id}.beta', (case.C,), scale=0.3).to(DEV))


def _running(case):
    return (detgen.normal(f'bnt.{case.id}.rm', (case.C,), scale=0.2).to(DEV),
            detgen.uniform(f'bnt.{case.id}.rv', (case.C,), 0.5, 1.5).to(DEV))


def _within(got, ref64, bound, what):
    err = (got.detach().cpu().double() - ref64).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f'{what}: max err / bound = {worst:.4f}')
    assert bool((err <= bound).all()), (what, worst)


def _one_ulp(got, ref64, what):
    """|got - ref| <= the spacing of fp32 at ref (one ulp)."""
    ref = ref64.numpy()
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(got.detach().cpu().double().numpy() - ref)
    print(f'{what}: max err / ulp = {float((err / ulp).max()):.4f}')
    assert (err <= ulp).all(), what


# --------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize('case', CASE_PARAMS)
def test_statistics_against_fp64(case):
    hip = _hip()
    x = _place(case, _x_for_stats(case))
    gamma, beta = _affine(case)
    count = 3
    runs = []
    for _ in range(2):
        rm, rv = _running(case)
        runs.append(hip.bn_train_stats(x, gamma, beta, 1e-5, case.momentum, rm, rv, count) + (rm, rv))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    mean, var, invstd, scale, shift, rm, rv = runs[0]

    x64 = x.cpu().double()
    m = case.N * case.H * case.W
    mean64, var64 = x64.mean((0, 2, 3)), x64.var((0, 2, 3), unbiased=False)
    b_mean = U24 * mean64.abs() + m * U53 * x64.abs().mean((0, 2, 3))
    b_var = U24 * var64 + m * U53 * (x64 * x64).mean((0, 2, 3))
    _within(mean, mean64, b_mean, f'{case.id} mean')
    _within(var, var64, b_var, f'{case.id} var')
    assert float(var[0]) == 0.0 and float(mean[0]) == 0.75           # the constant channel
    assert bool((var >= 0).all())

    # the affine map: the fp64 formulas on the mean and var that were written
    mk, vk = mean.cpu().double(), var.cpu().double()
    g64 = torch.ones(case.C, dtype=torch.float64) if gamma is None else gamma.cpu().double()
    b64 = torch.zeros(case.C, dtype=torch.float64) if beta is None else beta.cpu().double()
    inv64 = 1.0 / torch.sqrt(vk + float(np.float32(1e-5)))
    _one_ulp(invstd, inv64, f'{case.id} invstd')
    _one_ulp(scale, g64 * inv64, f'{case.id} scale')
    _one_ulp(shift, b64 - mk * (g64 * inv64), f'{case.id} shift')

    # the running statistics: torch's batch norm in fp64 on the same data and buffers
    rm0, rv0 = _running(case)
    rm64, rv64 = rm0.cpu().double(), rv0.cpu().double()
    factor = 1.0 / count if case.momentum is None else case.momentum
    torch.nn.functional.batch_norm(x64, rm64, rv64, g64, b64, True, factor, 1e-5)
    _within(rm, rm64, U24 * rm64.abs() + factor * b_mean, f'{case.id} running_mean')
    _within(rv, rv64, U24 * rv64.abs() + factor * b_var * m / (m - 1), f'{case.id} running_var')


def test_the_slab_case_has_several_slabs():
    case = B.BY_ID['slabs']
    assert _hip().bn_train_slabs(case.N, case.C, case.H, case.W) >= 3
    assert all(_hip().bn_train_slabs(c.N, c.C, c.H, c.W) >= 1 for c in B.CASES)


def test_statistics_without_running_buffers():
    case = B.BY_ID['run30']
    x = _place(case, _x_for_stats(case))
    rm, rv = _running(case)
    with_buffers = _hip().bn_train_stats(x, None, None, 1e-5, 0.1, rm, rv)
    without = _hip().bn_train_stats(x, None, None, 1e-5, 0.1)
    for a, b in zip(with_buffers, without):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------------- fold
@pytest.mark.parametrize('forced', [False, True], ids=['free', 'forced'])
@pytest.mark.parametrize('scheme', ['ls-1', 'ls-2', 'ls-T', 'gf-3'])
@pytest.mark.parametrize('case', CASE_PARAMS)
def test_bn_apply_is_the_quantizers_fold(case, scheme, forced):
    """lsq_act_quant behind pre = (scale, shift) and lsq_act_quant of lsq_bn_apply's tensor: the same planes and scales."""
    from quant.binary.hip_module import zero_planes
    hip = _hip()
    k = SCHEME_K[scheme]
    x = _place(case, _x_for_fold(case, k))
    scale, shift = (t.to(DEV) for t in _fold(case))
    y = hip.bn_apply(x, scale, shift)
    want = _fold64(x.cpu(), scale.cpu().view(1, -1, 1, 1), shift.cpu().view(1, -1, 1, 1)).float()    # one rounding, as fmaf
    assert torch.equal(y.cpu(), want)
    assert int((y == 0).sum()) > 0 and int((y == 1).sum()) > 0 and int((y == -1).sum()) > 0 or x.numel() < 40
    geom = hip.make_geom(case.N, case.C, case.H, case.W, 8, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    scales_in = _plane_scales(case, k).to(DEV).contiguous() if forced else None
    got = []
    for operand, pre in ((x, (scale, shift)), (y, None)):
        planes = zero_planes(geom, k, DEV, hip)
        scales = torch.empty((k, case.N), dtype=torch.float32, device=DEV)
        hip.act_quant(operand, geom, _scheme_id(scheme), k, 3, case.alpha, planes, scales, scales_in, pre=pre)
        got.append((planes, scales))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    # (a row of three values sub-sampled by 3 can solve to v_1 = 0: the scales are checked for being scales, not for size)
    assert int((got[0][0] != 0).sum()) > 0 and bool((got[0][1] >= 0).all()) and bool(torch.isfinite(got[0][1]).all())


@pytest.mark.parametrize('dyadic', [True, False], ids=['dyadic', 'generic'])
@pytest.mark.parametrize('case', CASE_PARAMS)
def test_quant_values_bn_equals_the_unfused_pair(case, dyadic):
    hip = _hip()
    k = SCHEME_K[case.scheme]
    x = _place(case, _x_for_fold(case, k) if dyadic else _x_for_stats(case))
    if dyadic:
        scale, shift = (t.to(DEV) for t in _fold(case))
    else:
        scale, shift = hip.bn_train_stats(x, *_affine(case), 1e-5, 0.1)[3:]
    v = _plane_scales(case, k, dyadic)
    v = None if v is None else v.to(DEV)
    got = hip.quant_values_bn(x, scale, shift, v, case.alpha)
    want = hip.quant_values(hip.bn_apply(x, scale, shift), v, case.alpha)
    assert torch.equal(got, want)
    assert float(got.abs().sum()) > 0


# ----------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize('dyadic', [True, False], ids=['dyadic', 'stats'])
@pytest.mark.parametrize('case', CASE_PARAMS)
def test_backward_against_fp64(case, dyadic):
    """grad_beta, grad_gamma: fp64 sums of the unfused kernels' g and g x^.  grad_x: the closed form in fp64 on that g and the
    sums the kernel wrote.  Channel 1 gets a zero gradient: its grad_x must be exactly 0."""
    hip = _hip()
    k = SCHEME_K[case.scheme]
    m = case.N * case.H * case.W
    x = _place(case, _x_for_fold(case, k) if dyadic else _x_for_stats(case))
    if dyadic:
        scale, shift = (t.to(DEV) for t in _fold(case))
        mean, invstd = (-shift / scale).contiguous(), scale.clone()
    else:
        mean, _, invstd, scale, shift = hip.bn_train_stats(x, *_affine(case), 1e-5, 0.1)
    v = _plane_scales(case, k, dyadic)
    v = None if v is None else v.to(DEV)
    gq_cpu = detgen.normal(f'bnt.{case.id}.gq', (case.N, case.C, case.H, case.W))
    gq_cpu[:, 1] = 0.0
    gq = _place(case, gq_cpu.view(-1))

    runs = [hip.bn_ste_backward(x, gq, scale, shift, mean, invstd, v, case.alpha) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    gx, ggamma, gbeta = runs[0]

    g = hip.ste_backward(hip.bn_apply(x, scale, shift), gq.contiguous(), v, case.alpha).cpu().double()
    assert float(g.abs().sum()) > 0
    per_c = lambda t: t.view(1, -1, 1, 1)                                              # noqa: E731
    xh = (x.cpu().double() - per_c(mean.cpu().double())) * per_c(invstd.cpu().double())
    sum_g, sum_gx = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
    _within(gbeta, sum_g, U24 * sum_g.abs() + m * U53 * g.abs().sum((0, 2, 3)), f'{case.id} grad_beta')
    _within(ggamma, sum_gx, U24 * sum_gx.abs() + m * U53 * (g * xh).abs().sum((0, 2, 3)), f'{case.id} grad_gamma')

    a, b = per_c(gbeta.cpu().double()) / m, per_c(ggamma.cpu().double()) / m
    s64 = per_c(scale.cpu().double())
    want = s64 * (g - a - xh * b)
    bound = GRAD_X_ROUNDINGS * U24 * s64.abs() * (g.abs() + a.abs() + xh.abs() * b.abs())
    _within(gx, want, bound, f'{case.id} grad_x')
    nothing = (g == 0) & (a == 0) & (xh * b == 0)
    assert bool(nothing[:, 1].all()) and bool((gx.cpu()[nothing] == 0).all())


# ----------------------------------------------------------------------------------------------------------- refusals
def test_argument_errors_come_back_without_a_launch():
    hip = _hip()
    lib = hip.bn_train_lib()
    n, c, h, w = 2, 4, 4, 4
    x = torch.ones((n, c, h, w), device=DEV)
    vec = [torch.full((c,), 7.0, device=DEV) for _ in range(8)]
    out = torch.full((n, c, h, w), 7.0, device=DEV)
    ws = torch.zeros((4096,), dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()                                                          # noqa: E731
    E_NULL, E_SHAPE, E_SCHEME, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -3, -5, -6

    def stats(xp=p(x), n=n, c=c, h=h, w=w, mean=p(vec[0]), wsp=p(ws), wsb=ws.numel(), rm=None, rv=None, mom=0.1, count=1):
        return lib.lsq_bn_train_stats(xp, n, c, h, w, None, None, 1e-5, mom, count, rm, rv, mean, p(vec[1]), p(vec[2]), p(vec[3]),
                                      p(vec[4]), wsp, wsb, None)

    assert stats(xp=None) == E_NULL and stats(mean=None) == E_NULL and stats(rm=p(vec[5])) == E_NULL
    assert stats(n=0) == E_SHAPE and stats(w=-1) == E_SHAPE and stats(n=1, h=1, w=1) == E_SHAPE
    assert stats(rm=p(vec[5]), rv=p(vec[6]), mom=-1.0, count=0) == E_SHAPE
    assert stats(n=65536) == E_UNSUPPORTED and stats(c=65536) == E_UNSUPPORTED and stats(xp=p(x) + 2) == E_UNSUPPORTED
    assert stats(wsp=None) == E_WORKSPACE and stats(wsb=8) == E_WORKSPACE and stats(wsp=p(ws) + 8) == E_WORKSPACE

    def apply(xp=p(x), n=n, s=p(vec[0]), y=p(out)):
        return lib.lsq_bn_apply(xp, n, c, h, w, s, p(vec[1]), y, None)

    assert apply(xp=None) == E_NULL and apply(s=None) == E_NULL and apply(y=None) == E_NULL
    assert apply(n=0) == E_SHAPE and apply(n=65536) == E_UNSUPPORTED and apply(y=p(out) + 1) == E_UNSUPPORTED

    def values(k=1, v=p(vec[2]), n=n, xq=p(out)):
        return lib.lsq_quant_values_bn(p(x), n, c, h, w, p(vec[0]), p(vec[1]), k, v, 2.0, xq, None)

    assert values(v=None) == E_NULL and values(xq=None) == E_NULL and values(n=0) == E_SHAPE
    assert values(k=-1) == E_SCHEME and values(k=hip.MAX_PLANES + 1) == E_SCHEME and values(n=65536) == E_UNSUPPORTED

    def backward(gq=p(x), k=1, v=p(vec[2]), n=n, gx=p(out), gg=p(vec[5]), wsp=p(ws), wsb=ws.numel()):
        return lib.lsq_bn_ste_backward(p(x), gq, n, c, h, w, p(vec[0]), p(vec[1]), p(vec[3]), p(vec[4]), k, v, 2.0, gx, gg,
                                       p(vec[6]), wsp, wsb, None)

    assert backward(gq=None) == E_NULL and backward(v=None) == E_NULL and backward(gg=None) == E_NULL
    assert backward(n=0) == E_SHAPE and backward(k=9) == E_SCHEME and backward(n=65536) == E_UNSUPPORTED
    assert backward(gx=p(out) + 2) == E_UNSUPPORTED
    assert backward(wsp=None) == E_WORKSPACE and backward(wsb=16) == E_WORKSPACE and backward(wsp=p(ws) + 4) == E_WORKSPACE
    assert lib.lsq_bn_train_workspace_bytes(0, c, h, w) == 0 and lib.lsq_bn_ste_backward_workspace_bytes(n, c, 0, w) == 0
    assert lib.lsq_bn_ste_backward_workspace_bytes(n, c, h, w) > lib.lsq_bn_train_workspace_bytes(n, c, h, w) > 0

    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and all(bool((t == 7.0).all()) for t in vec) and bool((ws == 0).all())
    assert stats() == 0                                                                # the accepted call, last
    torch.cuda.synchronize()
    assert float(vec[0][0]) == 1.0 and float(vec[1][0]) == 0.0


def test_the_bindings_refuse_what_the_library_would():
    hip = _hip()
    x = torch.ones((2, 4, 4, 4), device=DEV)
    s = torch.ones((4,), device=DEV)
    with pytest.raises(TypeError):
        hip.bn_apply(x.half(), s, s)
    with pytest.raises(ValueError, match='contiguous'):
        hip.bn_apply(x.permute(0, 1, 3, 2)[:, :, :, ::2], s, s)
    with pytest.raises(ValueError, match='C = 4'):
        hip.bn_apply(x, s[:3].contiguous(), s)
    with pytest.raises(ValueError, match='more than 1 value'):
        hip.bn_train_stats(x[:1, :, :1, :1].contiguous(), None, None, 1e-5, 0.1)
    with pytest.raises(ValueError, match='shape of x'):
        hip.bn_ste_backward(x, x[:1].contiguous(), s, s, s, s, None, 2.0)
    with pytest.raises(ValueError, match='plane scales'):
        hip.quant_values_bn(x, s, s, torch.ones((2, 3), device=DEV), 2.0)
