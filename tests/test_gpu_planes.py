"""The binary kernels at every bit-plane count up to LSQ_MAX_PLANES = 8 (include/lsq_hip.h) on each side.

Before these tests, no GPU test went past two or three planes, and the code that only runs deeper went untested: the greedy
chain of lsq_act_quant past plane 2, odd activation plane counts (the last launch of a convolution or linear call is a
one-plane accumulating launch that carries the epilogue), plane offsets that are only nonzero from the third plane on,
and calls of up to 32 accumulating launches.

References: bits -- the fp32 chains of the oracle (planes_ref, P.quant_gf), bit for bit; free-running scales -- mean |residual|
in fp64 of the fp32 residual chain run with the GPU's own earlier scales, rtol 1e-6; outputs -- an fp64 convolution / matmul
of the oracle's x_q and w_q, |y - ref| <= TOL * max|ref|.  Every tolerance check also shows that it can see the deepest plane
on either side (`_assert_sees_deepest_planes`).
"""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detgen
from oracle import ref_port as P
from test_gpu_linear import _popcount_route
from test_gpu_parity import pack_ref, planes_ref, run_act_quant

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOL = 1e-4
GF = 4                 # LSQ_SCHEME_GF
MAXP = 8               # LSQ_MAX_PLANES
CLAMP = {'kind': 'symmetric', 'alpha': 2}

# (kx, kw): every kx with kw = 1, every kw with kx = 1, and mixed depths
GRID = [(k, 1) for k in range(1, MAXP + 1)] + [(1, k) for k in range(2, MAXP + 1)] + [(3, 3), (5, 2), (2, 7), (7, 4), (8, 8)]


def _hip():
    from quant import _hip
    return _hip


def rel_err(y, ref):
    return float((y.double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max())


def _assert_sees_deepest_planes(y, ref, ref_no_x, ref_no_w, what):
    """y within TOL of ref, and ref without the deepest activation plane / without the deepest weight plane at least
    10 x TOL away from y: the tolerance can see the last plane on either side."""
    assert rel_err(y, ref) <= TOL, (what, rel_err(y, ref))
    for name, other in (('x', ref_no_x), ('w', ref_no_w)):
        d = float((y.double().cpu() - other.double().cpu()).abs().max() / ref.double().abs().max())
        assert d >= 10 * TOL, (what, 'deepest plane of', name, 'is invisible', d)


# ================================================================================================ 1. lsq_act_quant, GF, k = 1 .. 8
QSHAPES = [  # (shape, groups, pad, alpha, sweep workspace)
    ((2, 64, 8, 8), 1, (1, 1), 2.0, True),        # run<4>, rows shared by several workgroups
    ((1, 64, 6, 7), 1, (0, 0), 2.0, True),        # run<2> (H*W = 42), batch 1, no padding
    ((2, 64, 7, 7), 1, (2, 2), 2.0, False),       # run<1> (H*W = 49), one workgroup per row, pad 2
    ((2, 100, 8, 8), 1, (1, 1), -1.0, True),      # channel tail (64 + 36), no clamp
    ((1, 96, 6, 7), 2, (2, 1), 3.0, False),       # groups = 2 (48 channels each), run<2>
    ((2, 130, 5, 9), 1, (1, 2), -1.0, True),      # odd image, run<1>, a tail of 2 channels, no clamp
    ((2, 64, 28, 28), 1, (1, 1), 2.0, False),     # run<4>, one workgroup per row
]


def _act_input(case):
    shape = QSHAPES[case][0]
    x = detgen.normal(f'planes.q.x{case}', shape, scale=1.3)
    x.view(-1)[::17] = 0.0
    x.view(-1)[5::29] = -0.0
    return x


def _quant(x, k, alpha, groups, pad, workspace=True, forced=None):
    """lsq_act_quant(GF, k) -> (planes uint64 [k, N, Gt, Hp, Wp], scales [k, N]); workspace=False: no sweep workspace."""
    if workspace or forced is not None:
        return run_act_quant(x, GF, k, alpha, groups, pad, forced=forced)
    hip = _hip()
    n, c, h, w = x.shape
    geom = hip.make_geom(n, c, h, w, 64, 3, 3, (1, 1), pad, (1, 1), groups)
    planes = torch.zeros((k * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    scales = torch.empty((k, n), dtype=torch.float32, device=DEV)
    xd = x.to(DEV).contiguous()
    code = hip.lib().lsq_act_quant(xd.data_ptr(), ctypes.byref(geom), GF, k, 3, float(alpha), None, None, None,
                                   planes.data_ptr(), scales.data_ptr(), None, 0, hip.stream_ptr(xd.device))
    assert code == 0, code
    torch.cuda.synchronize()
    gt = groups * ((c // groups + 63) // 64)
    return planes.cpu().numpy().view(np.uint64).reshape(k, n, gt, h + 2 * pad[0], w + 2 * pad[1]), scales.cpu()


def _clamped(x, alpha):
    return x.clamp(-alpha, alpha) if alpha > 0 else x


@pytest.mark.parametrize('k', range(1, MAXP + 1))
@pytest.mark.parametrize('case', range(len(QSHAPES)))
def test_gf_quantizer_free_running(case, k):
    """Scale q = mean |residual_q| (fp64, residual chain in fp32 with the GPU's own v_1 .. v_(q-1)), rtol 1e-6; planes
    = the oracle's result chain with the GPU's scales, bit for bit, halo words zero."""
    shape, groups, pad, alpha, ws = QSHAPES[case]
    x = _act_input(case)
    planes, scales = _quant(x, k, alpha, groups, pad, workspace=ws)
    xc = _clamped(x, alpha)
    resid = xc.reshape(shape[0], -1).clone()
    for q in range(k):
        want = resid.double().abs().mean(dim=1)
        assert torch.allclose(scales[q].double(), want, rtol=1e-6, atol=0), (case, k, q, scales[q], want)
        resid = resid - scales[q].view(-1, 1) * P.pm1(resid)
    for q, b in enumerate(planes_ref(xc, list(scales))):
        assert np.array_equal(planes[q], pack_ref(b, groups, pad)), (case, k, q)


@pytest.mark.parametrize('case', range(len(QSHAPES)))
def test_gf_quantizer_given_scales(case):
    """The moving-average eval path (scales given) for k = 3 .. 8: planes = planes_ref(x, forced), scales = forced."""
    shape, groups, pad, alpha, _ = QSHAPES[case]
    x = _act_input(case)
    xc = _clamped(x, alpha)
    for k in range(3, MAXP + 1):
        forced = torch.stack([detgen.uniform(f'planes.q.f{case}.{i}', (shape[0],), 0.9 / 2 ** i, 1.4 / 2 ** i) for i in range(k)])
        planes, scales = _quant(x, k, alpha, groups, pad, forced=forced)
        assert torch.equal(scales, forced), (case, k)
        for q, b in enumerate(planes_ref(xc, list(forced))):
            assert np.array_equal(planes[q], pack_ref(b, groups, pad)), (case, k, q)


@pytest.mark.parametrize('shape,alpha', [((2, 64, 8, 8), 2.0), ((2, 70, 7, 7), -1.0)])
def test_gf_quantizer_exact_ties_at_depth(shape, alpha):
    """Inputs on multiples of 2^-6 and given scales 1, 1/2, ..., 1/128: x - result == 0 happens at planes q >= 3, where
    sign(+0) = +1 must hold (ste.py:16-18)."""
    rs = np.random.RandomState(61)
    x = torch.from_numpy((rs.randint(-128, 129, size=shape) / 64.0).astype(np.float32))
    n = shape[0]
    forced = torch.stack([torch.full((n,), 2.0 ** -i) for i in range(MAXP)])
    planes, scales = _quant(x, MAXP, alpha, 1, (1, 1), forced=forced)
    assert torch.equal(scales, forced)
    xc = _clamped(x, alpha)
    result, ties = torch.zeros_like(xc), 0
    for q, b in enumerate(planes_ref(xc, list(forced))):
        tie = (xc - result) == 0
        if q >= 3:
            ties += int(tie.sum())
            assert bool(b[tie].all())
        assert np.array_equal(planes[q], pack_ref(b, 1, (1, 1))), q
        result = result + forced[q].view(-1, 1, 1, 1) * P.pm1(xc - result)
    assert ties > 100, ties


# ================================================================================================ 2. lsq_pack_weight, k = 1 .. 8
PACK_CASES = [  # (O, C, KH, KW, groups)
    (40, 64, 1, 1, 1),         # 1x1
    (24, 70, 3, 3, 1),         # channel tail, 24 out-channels (not a multiple of 16)
    (36, 32, 5, 5, 2),         # 5x5, groups = 2, 18 out-channels per group
    (20, 130, 3, 3, 2),        # groups = 2 with a tail of 1 channel per group, 10 out-channels per group
    (48, 128, 3, 3, 1),
]


def _wbits_ref(bits, groups):
    """bool [O, cg, KH, KW] -> uint64 [taps, Gg, groups * og_pad] in the layout of include/lsq_hip.h."""
    o, cg, kh, kw = bits.shape
    taps, gg, og = kh * kw, (cg + 63) // 64, o // groups
    og_pad = (og + 15) // 16 * 16
    b = bits.reshape(o, cg, taps).astype(np.uint64)
    out = np.zeros((taps, gg, groups * og_pad), dtype=np.uint64)
    for grp in range(groups):
        for j in range(gg):
            nb = min(64, cg - 64 * j)
            chunk = b[grp * og:(grp + 1) * og, 64 * j:64 * j + nb, :] << np.arange(nb, dtype=np.uint64).reshape(1, nb, 1)
            out[:, j, grp * og_pad:grp * og_pad + og] = chunk.sum(axis=1, dtype=np.uint64).T     # (distinct bits: sum = or)
    return out


@pytest.mark.parametrize('k', range(1, MAXP + 1))
@pytest.mark.parametrize('case', range(len(PACK_CASES)))
def test_pack_weight_every_depth(case, k):
    """Unpacked bits = planes_ref(w, scales) bit for bit, padded out-channel slots zero, wsum[q][o][tap] = sum of the +-1."""
    hip = _hip()
    o, c, kh, kw, groups = PACK_CASES[case]
    cg = c // groups
    w = detgen.normal(f'planes.pack.w{case}', (o, cg, kh, kw), scale=0.5)
    w.view(-1)[::29] = 0.0
    scales = torch.stack(P.weight_scales(w, f'gf-{k}'))
    geom = hip.make_geom(2, c, 6, 6, o, kh, kw, (1, 1), (kh // 2, kw // 2), (1, 1), groups)
    wbits, wsum = hip.pack_weight(w.to(DEV), geom, scales.to(DEV))
    torch.cuda.synchronize()
    taps, gg, og_pad = kh * kw, (cg + 63) // 64, (o // groups + 15) // 16 * 16
    got = wbits.cpu().numpy().view(np.uint64).reshape(k, taps, gg, groups * og_pad)
    sums = wsum.cpu().to(torch.int64)
    for q, b in enumerate(planes_ref(w, list(scales))):
        b = b.numpy()
        assert np.array_equal(got[q], _wbits_ref(b, groups)), (case, k, q)
        want = torch.from_numpy((2 * b.astype(np.int64) - 1).reshape(o, cg, taps).sum(axis=1))
        assert torch.equal(sums[q], want), (case, k, q)


# ================================================================================================ 3. lsq_xnor_conv2d, (kx, kw) grid
def _conv_case(tag, n, c, h, w, o, kh, kw_, stride, pad, dil, groups, kx, kw, forced=None, wsc=None, bias=True):
    """GF(kx) activation planes of x (free-running, or the scales `forced`) and GF(kw) weight planes (the oracle's scales,
    or `wsc`)."""
    hip = _hip()
    geom = hip.make_geom(n, c, h, w, o, kh, kw_, stride, pad, dil, groups)
    x = detgen.uniform(tag + '.x', (n, c, h, w), -2.2, 2.2)
    planes = torch.zeros((kx * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xs = torch.empty((kx, n), dtype=torch.float32, device=DEV)
    hip.act_quant(x.to(DEV), geom, GF, kx, 3, 2.0, planes, xs, None if forced is None else forced.to(DEV).contiguous())
    wt = detgen.uniform(tag + '.w', (o, c // groups, kh, kw_), -0.5, 0.5)
    if wsc is None:
        wsc = torch.stack(P.weight_scales(wt, f'gf-{kw}'))
    wsc = wsc.to(DEV).contiguous()
    wbits, wsum = hip.pack_weight(wt.to(DEV), geom, wsc)
    b = detgen.normal(tag + '.b', (o,), scale=0.2).to(DEV) if bias else None
    ho, wo = hip.out_hw(geom)
    return dict(geom=geom, x=x, planes=planes, xs=xs, wt=wt, wsc=wsc, wbits=wbits, wsum=wsum, b=b, kx=kx, kw=kw,
                stride=stride, pad=pad, dil=dil, groups=groups, yshape=(n, o, ho, wo))


def _conv_ref(cs, drop_x=False, drop_w=False, epi=None):
    """fp64 convolution of the oracle's x_q (GF chain with the call's activation scales) and w_q, bias and epilogue; drop_x /
    drop_w: the deepest activation / weight plane's scale set to 0."""
    xs = [v.clone() for v in cs['xs'].cpu()]
    ws = [v.clone() for v in cs['wsc'].cpu()]
    if drop_x:
        xs[-1].zero_()
    if drop_w:
        ws[-1].zero_()
    xq = P.quant_gf(cs['x'].clamp(-2, 2), cs['kx'], xs)[1]
    wq = P.quantize_weight(cs['wt'], f"gf-{cs['kw']}", ws)
    b = None if cs['b'] is None else cs['b'].cpu().double()
    y = F.conv2d(xq.double(), wq.double(), b, cs['stride'], cs['pad'], cs['dil'], cs['groups'])
    if epi:
        if epi.get('res_pre') is not None:
            y = y + epi['res_pre'].cpu().double()
        if epi.get('relu'):
            y = y.clamp_min(0)
        if epi.get('prelu') is not None:
            y = torch.where(y > 0, y, y * epi['prelu'].cpu().double().view(1, -1, 1, 1))
        if epi.get('res_post') is not None:
            y = y + epi['res_post'].cpu().double()
    return y


def _conv_run(cs, epi=None):
    hip = _hip()
    y = torch.full(cs['yshape'], float('nan'), device=DEV)
    hip.xnor_conv2d(cs['planes'], cs['kx'], cs['xs'], cs['wbits'], cs['wsum'], cs['wsc'], cs['b'], cs['geom'], y, **(epi or {}))
    torch.cuda.synchronize()
    return y


MFMA_GEOS = [  # (n, h, w, o, stride, pad, dil): 3x3, dilation_w = 1, O % 32 == 0 -- the matrix-core kernel's geometries
    (2, 9, 11, 32, (1, 1), (1, 1), (1, 1)),
    (2, 12, 10, 64, (2, 1), (1, 2), (2, 1)),
    (1, 7, 7, 96, (2, 2), (1, 1), (1, 1)),
    (3, 6, 5, 32, (1, 1), (0, 0), (1, 1)),
]


@pytest.mark.parametrize('kx,kw', GRID)
def test_xnor_conv_matrix_core_geometry(kx, kw):
    """3x3 over 64 / 128 / 256 / 512 channels: popcount, fp4 and int8 matrix-core kernels agree bit for bit, plain and with
    every epilogue (an odd kx puts the epilogue into a one-plane accumulating launch); each within TOL of fp64."""
    hip = _hip()
    i = GRID.index((kx, kw))
    c = (64, 128, 256, 512)[i % 4]
    n, h, w, o, stride, pad, dil = MFMA_GEOS[i % len(MFMA_GEOS)]
    tag = f'planes.xm.{kx}.{kw}'
    cs = _conv_case(tag, n, c, h, w, o, 3, 3, stride, pad, dil, 1, kx, kw)
    res = detgen.normal(tag + '.r1', cs['yshape'], scale=2.0).to(DEV)
    res2 = detgen.normal(tag + '.r2', cs['yshape'], scale=2.0).to(DEV)
    slope = detgen.uniform(tag + '.sl', (o,), 0.1, 0.4).to(DEV)
    epis = [{}, dict(res_pre=res, relu=True), dict(prelu=slope), dict(res_post=res2), dict(res_pre=res, res_post=res2, relu=True)]
    outs = []
    for impl in (True, False, 2):             # popcount, fp4 matrix cores (the default), int8 matrix cores
        with hip.debug_switches(xnor_popcount=impl):
            outs.append([_conv_run(cs, e) for e in epis])
    for impl in (1, 2):
        for e, u, v in zip(epis, outs[0], outs[impl]):
            assert torch.equal(u, v), (kx, kw, c, impl, sorted(e), float((u - v).abs().max()))
    for e, y in zip(epis, outs[0]):
        assert rel_err(y, _conv_ref(cs, epi=e)) <= TOL, (kx, kw, c, sorted(e), rel_err(y, _conv_ref(cs, epi=e)))
    _assert_sees_deepest_planes(outs[0][0], _conv_ref(cs), _conv_ref(cs, drop_x=True), _conv_ref(cs, drop_w=True), (kx, kw, c))


OTHER_GEOS = [  # (n, c, h, w, o, kh, kw, stride, pad, dil, groups): outside the matrix-core kernel
    (2, 96, 9, 8, 40, 3, 3, (1, 1), (1, 1), (1, 1), 2),       # groups = 2
    (2, 100, 7, 9, 24, 1, 1, (1, 1), (0, 0), (1, 1), 1),      # 1x1, ragged channels
    (1, 70, 11, 10, 20, 5, 5, (2, 1), (2, 1), (1, 1), 1),     # 5x5, stride per axis, ragged channels
    (2, 64, 10, 12, 33, 3, 3, (1, 2), (2, 1), (2, 1), 1),     # dilation and stride per axis, 33 out-channels
    (1, 128, 8, 8, 48, 3, 3, (1, 1), (1, 1), (1, 2), 2),      # dilation_w = 2, groups = 2
]


@pytest.mark.parametrize('kx,kw', GRID)
def test_xnor_conv_other_geometries(kx, kw):
    i = GRID.index((kx, kw))
    for gi in (i % len(OTHER_GEOS), (i + 2) % len(OTHER_GEOS)):
        n, c, h, w, o, kh, kw_, stride, pad, dil, groups = OTHER_GEOS[gi]
        cs = _conv_case(f'planes.xo.{kx}.{kw}.{gi}', n, c, h, w, o, kh, kw_, stride, pad, dil, groups, kx, kw)
        y = _conv_run(cs)
        _assert_sees_deepest_planes(y, _conv_ref(cs), _conv_ref(cs, drop_x=True), _conv_ref(cs, drop_w=True), (kx, kw, gi))


@pytest.mark.parametrize('kx,kw', [p for p in GRID if (p[0] - 1) + (p[1] - 1) <= 12])
def test_xnor_conv_exact_with_power_of_two_scales(kx, kw):
    """Activation scales 2^-(p+1), weight scales 2^-(q+1), C = 64, 3x3, no bias: y equals the fp64 result bit for bit.

    Why it is exact: a plane pair (p, q) contributes I * 2^-(p+1) * 2^-(q+1) with an integer I, |I| <= 64 * 9 = 576 < 2^10
    (padded taps add exactly 0).  Every partial sum of such terms, in any order and grouping, is an integer multiple of
    2^-(kx+kw) of magnitude below 576 * (1 - 2^-kx) * (1 - 2^-kw) < 2^10, i.e. an integer below 2^(10+kx+kw) <= 2^24
    times 2^-(kx+kw) when (kx - 1) + (kw - 1) <= 12: exactly representable in fp32, so no step of the kernel rounds.
    The oracle's x_q and w_q are sums of at most 8 signed powers of two between 2^-1 and 2^-8: exact in fp32 too."""
    hip = _hip()
    n, o = 2, 32
    forced = torch.stack([torch.full((n,), 2.0 ** -(p + 1)) for p in range(kx)])
    wsc = torch.stack([torch.full((o,), 2.0 ** -(q + 1)) for q in range(kw)])
    cs = _conv_case(f'planes.xe.{kx}.{kw}', n, 64, 8, 9, o, 3, 3, (1, 1), (1, 1), (1, 1), 1, kx, kw, forced=forced, wsc=wsc,
                    bias=False)
    ref64 = _conv_ref(cs)
    assert torch.equal(ref64.float().double(), ref64)
    for impl in (True, False, 2):
        with hip.debug_switches(xnor_popcount=impl):
            y = _conv_run(cs).cpu()
        assert torch.equal(y, ref64.float()), (kx, kw, impl, float((y.double() - ref64).abs().max()))


# ================================================================================================ 4. lsq_signw_conv2d, kw = 3 .. 8
SIGNW_FAST = [  # (n, c, h, w, o, stride, pad, dil): 3x3, groups 1 -- lsq_signw_prepare_weight accepts these; without the
    (4, 32, 5, 9, 72, 1, 1, 1),                 # prepared weights both take signw_conv_patch
    (2, 64, 13, 13, 64, 2, 1, 1),
]


def _signw_ref(x, alpha, wt, wsc, b, stride, pad, dil, groups, drop_w=False):
    ws = [v.clone() for v in wsc.cpu()]
    if drop_w:
        ws[-1].zero_()
    wq = P.quantize_weight(wt.cpu(), f'gf-{len(ws)}', ws)
    xq = _clamped(x.cpu(), alpha)
    return F.conv2d(xq.double(), wq.double(), None if b is None else b.cpu().double(), stride, pad, dil, groups)


@pytest.mark.parametrize('kw', range(3, MAXP + 1))
@pytest.mark.parametrize('gi', range(len(SIGNW_FAST)))
def test_signw_fast_path_every_depth(gi, kw):
    """Prepared fast path = general kernels bit for bit across the epilogue variants; both within TOL of fp64, and the
    tolerance sees the deepest weight plane."""
    hip = _hip()
    n, c, h, w, o, stride, pad, dil = SIGNW_FAST[gi]
    tag = f'planes.sw.{gi}.{kw}'
    x = detgen.normal(tag + '.x', (n, c, h, w), scale=1.3).to(DEV)
    wt = detgen.uniform(tag + '.w', (o, c, 3, 3), -0.5, 0.5)
    wsc = torch.stack(P.weight_scales(wt, f'gf-{kw}')).to(DEV).contiguous()
    g = hip.make_geom(n, c, h, w, o, 3, 3, (stride, stride), (pad, pad), (dil, dil), 1)
    wbits, _ = hip.pack_weight(wt.to(DEV), g, wsc)
    wprep = hip.signw_prepare_weight(wbits, kw, g)
    assert wprep is not None
    ho, wo = hip.out_hw(g)
    shape = (n, o, ho, wo)
    bias = detgen.normal(tag + '.b', (o,), scale=0.2).to(DEV)
    pre = (detgen.uniform(tag + '.ps', (c,), 0.5, 1.5).to(DEV), detgen.normal(tag + '.pt', (c,), scale=0.2).to(DEV))
    r1, r2 = detgen.normal(tag + '.r1', shape).to(DEV), detgen.normal(tag + '.r2', shape).to(DEV)
    variants = [dict(alpha=2.0, bias=bias), dict(alpha=2.0, bias=bias, pre=pre, prelu=torch.full((1,), 0.25, device=DEV), res_post=r2),
                dict(alpha=3.0, bias=bias, pre=pre, relu=True, res_pre=r1),
                dict(alpha=-1.0, bias=None, prelu=detgen.uniform(tag + '.sl', (o,), 0.1, 0.4).to(DEV), res_pre=r1, res_post=r2)]
    for kwargs in variants:
        alpha, b = kwargs.pop('alpha'), kwargs.pop('bias')
        y_fast = torch.full(shape, float('nan'), device=DEV)
        y_gen = torch.full(shape, float('nan'), device=DEV)
        hip.signw_conv2d(x, alpha, wbits, wsc, b, g, y_fast, wprep=wprep, **kwargs)
        hip.signw_conv2d(x, alpha, wbits, wsc, b, g, y_gen, **kwargs)
        torch.cuda.synchronize()
        assert torch.equal(y_fast, y_gen), (gi, kw, sorted(kwargs), rel_err(y_fast, y_gen))
    args = (x, 2.0, wt, wsc, bias, stride, pad, dil, 1)
    for wp in (wprep, None):
        y = torch.empty(shape, device=DEV)
        hip.signw_conv2d(x, 2.0, wbits, wsc, bias, g, y, wprep=wp)
        torch.cuda.synchronize()
        ref = _signw_ref(*args)
        assert rel_err(y, ref) <= TOL, (gi, kw, wp is None, rel_err(y, ref))
        d = float((y.double().cpu() - _signw_ref(*args, drop_w=True)).abs().max() / ref.abs().max())
        assert d >= 10 * TOL, (gi, kw, d)


@pytest.mark.parametrize('kw', [1, 3, 8])
def test_signw_tiled_fallback_every_depth(kw):
    """Stride 2 over a 14x14 image with 64 out-channels: the input patch does not fit the patch kernel's LDS, so the general
    path is signw_conv_tiled, which sums over (tap, 32-channel chunk) in another order than the fast path and is therefore
    not bit-identical to it.  Both paths are within TOL of fp64 and see the deepest weight plane."""
    hip = _hip()
    n, c, h, w, o = 2, 64, 14, 14, 64
    tag = f'planes.swt.{kw}'
    x = detgen.normal(tag + '.x', (n, c, h, w), scale=1.3).to(DEV)
    wt = detgen.uniform(tag + '.w', (o, c, 3, 3), -0.5, 0.5)
    wsc = torch.stack(P.weight_scales(wt, f'gf-{kw}')).to(DEV).contiguous()
    g = hip.make_geom(n, c, h, w, o, 3, 3, (2, 2), (1, 1), (1, 1), 1)
    wbits, _ = hip.pack_weight(wt.to(DEV), g, wsc)
    wprep = hip.signw_prepare_weight(wbits, kw, g)
    assert wprep is not None
    bias = detgen.normal(tag + '.b', (o,), scale=0.2).to(DEV)
    args = (x, 2.0, wt, wsc, bias, 2, 1, 1, 1)
    ref = _signw_ref(*args)
    for wp in (wprep, None):
        y = torch.empty((n, o) + hip.out_hw(g), device=DEV)
        hip.signw_conv2d(x, 2.0, wbits, wsc, bias, g, y, wprep=wp)
        torch.cuda.synchronize()
        assert rel_err(y, ref) <= TOL, (kw, wp is None, rel_err(y, ref))
        if kw > 1:
            assert float((y.double().cpu() - _signw_ref(*args, drop_w=True)).abs().max() / ref.abs().max()) >= 10 * TOL


@pytest.mark.parametrize('kw', range(3, MAXP + 1))
def test_signw_general_kernel_every_depth(kw):
    """5x5, groups = 2: lsq_signw_prepare_weight declines; the general kernel is within TOL of fp64 and sees the last plane."""
    hip = _hip()
    n, c, h, w, o, groups = 2, 32, 9, 10, 24, 2
    tag = f'planes.swg.{kw}'
    x = detgen.normal(tag + '.x', (n, c, h, w), scale=1.3).to(DEV)
    wt = detgen.uniform(tag + '.w', (o, c // groups, 5, 5), -0.5, 0.5)
    wsc = torch.stack(P.weight_scales(wt, f'gf-{kw}')).to(DEV).contiguous()
    g = hip.make_geom(n, c, h, w, o, 5, 5, (1, 2), (2, 1), (1, 1), groups)
    wbits, _ = hip.pack_weight(wt.to(DEV), g, wsc)
    assert hip.signw_prepare_weight(wbits, kw, g) is None
    bias = detgen.normal(tag + '.b', (o,), scale=0.2).to(DEV)
    y = torch.empty((n, o) + hip.out_hw(g), device=DEV)
    hip.signw_conv2d(x, 2.0, wbits, wsc, bias, g, y)
    torch.cuda.synchronize()
    args = (x, 2.0, wt, wsc, bias, (1, 2), (2, 1), (1, 1), groups)
    ref = _signw_ref(*args)
    assert rel_err(y, ref) <= TOL, (kw, rel_err(y, ref))
    assert float((y.double().cpu() - _signw_ref(*args, drop_w=True)).abs().max() / ref.abs().max()) >= 10 * TOL


# ================================================================================================ 5. lsq_linear_xnor, QuantLinear
def _linear_operands(n, t, f, o, kx, kw, seed, bias):
    """GF(kx) activation planes of x [n, t * f] (free-running) and GF(kw) weight planes of w [o, f] (the oracle's scales)."""
    hip = _hip()
    x = detgen.uniform(f'planes.lin.x.{seed}', (n, t * f), -2.2, 2.2).to(DEV)
    gx = hip.make_geom(n, t * f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    planes = torch.zeros((kx * hip.act_plane_words(gx),), dtype=torch.int64, device=DEV)
    scales = torch.empty((kx, n), dtype=torch.float32, device=DEV)
    hip.act_quant(x, gx, GF, kx, 3, 2.0, planes, scales)
    w = detgen.uniform(f'planes.lin.w.{seed}', (o, f), -0.5, 0.5)
    wsc = torch.stack(P.weight_scales(w.view(o, f, 1, 1), f'gf-{kw}')).to(DEV).contiguous()
    gw = hip.make_geom(n * t, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    wbits, wsum = hip.pack_weight(w.to(DEV).view(o, f, 1, 1), gw, wsc)
    b = detgen.normal(f'planes.lin.b.{seed}', (o,), scale=0.2).to(DEV) if bias else None
    return planes, scales, kx, wbits, wsum.view(-1, o), wsc, b, gw


@pytest.mark.parametrize('t', [1, 3])
@pytest.mark.parametrize('kx,kw', GRID)
def test_linear_bit_identical_to_the_1x1_popcount_route(kx, kw, t):
    hip = _hip()
    i = GRID.index((kx, kw))
    n, f, o = (7, 200, 33) if t == 1 else (5, 128, 40)
    planes, scales, k, wbits, wsum, wsc, b, gw = _linear_operands(n, t, f, o, kx, kw, seed=100 * t + i, bias=i % 2 == 0)
    y = hip.linear_xnor(planes, k, scales, t, wbits, wsum, wsc, b, n * t, f, o)
    ref = _popcount_route(planes, scales, k, t, wbits, wsum, wsc, b, gw)
    torch.cuda.synchronize()
    bad = (y.view(torch.int32) != ref.view(torch.int32)).sum().item()
    assert bad == 0, (kx, kw, t, bad, (y - ref).abs().max().item())


def _linear_oracle(x, m, xs, ws):
    n, f, o = x.shape[0], m.in_features, m.out_features
    x4 = P.clamp_act(x.reshape(n, -1, 1, 1), CLAMP)
    xq = P.quant_gf(x4, len(xs), xs)[1]
    wq = P.quantize_weight(m.weight.detach().cpu().view(o, f, 1, 1), m.w_quant, ws).view(o, f)
    return F.linear(xq.reshape(x.shape).double(), wq.double(), m.bias.detach().cpu().double())


@pytest.mark.parametrize('xs,ws', [('gf-8', 'gf-8'), ('gf-5', 'gf-3')])
@pytest.mark.parametrize('shape', [(16, 300), (6, 3, 128)])
def test_quant_linear_deep_schemes(xs, ws, shape):
    from quant.binary import QuantLinear
    f, o = shape[-1], 40
    m = QuantLinear(xs, ws, f, o, CLAMP)
    detgen.fill_module(m, seed=51)
    with torch.no_grad():
        m.weight.copy_(detgen.uniform('planes.ql.w', (o, f), -0.5, 0.5))
        for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight.view(o, f, 1, 1), ws)):
            buf.copy_(v)
    x = detgen.uniform(f'planes.ql.x{len(shape)}', shape, -2.2, 2.2)
    m.eval().to(DEV)
    with torch.no_grad():
        y = m(x.to(DEV)).cpu()
    assert m.last_act_scales.shape[0] == int(xs[3:])
    v = [s.clone() for s in m.last_act_scales.cpu()]
    u = [s.detach().cpu().clone() for s in m.w_approximate.cached_scales()]
    ref = _linear_oracle(x, m, v, u)
    v0, u0 = [s.clone() for s in v], [s.clone() for s in u]
    v0[-1].zero_()
    u0[-1].zero_()
    _assert_sees_deepest_planes(y, ref, _linear_oracle(x, m, v0, u), _linear_oracle(x, m, v, u0), (xs, ws, shape))


# ================================================================================================ 7. QuantConv2d and a network
MODULE_GEOS = [  # (c, o, kernel, stride, padding, dilation, groups, image): matrix-core 3x3; 5x3 grouped and strided
    (64, 64, 3, 1, 1, 1, 1, (9, 9)),
    (48, 40, (5, 3), (2, 1), (2, 1), 1, 2, (11, 8)),
]


def _gf_module(xs, ws, gi, mode='off'):
    from quant.binary.binary_conv import QuantConv2d
    c, o, ks, stride, pad, dil, groups, _ = MODULE_GEOS[gi]
    conv = QuantConv2d(xs, ws, c, o, ks, CLAMP, moving_average_mode=mode, stride=stride, padding=pad, dilation=dil,
                       groups=groups, bias=True)
    detgen.fill_module(conv, seed=70 + gi)
    with torch.no_grad():
        for buf, v in zip(conv.w_approximate.cached_scales(), P.weight_scales(conv.weight, ws)):
            buf.copy_(v)
    return conv


def _module_ref(conv, x, x_scales, details=None):
    w, b = conv.weight.detach().cpu(), conv.bias.detach().cpu()
    wsc = [s.detach().cpu() for s in conv.w_approximate.cached_scales()]
    return P.quant_conv2d(x, w, b, conv.x_quant, conv.w_quant, wsc, CLAMP, conv.stride, conv.padding, conv.dilation,
                          conv.groups, x_scales=x_scales, details=details)


@pytest.mark.parametrize('gi', range(len(MODULE_GEOS)))
@pytest.mark.parametrize('xs,ws', [('gf-8', 'gf-8'), ('gf-4', 'gf-3'), ('gf-3', 'gf-7'), ('gf-5', 'gf-1')])
def test_quant_conv2d_gf_eval(xs, ws, gi):
    """Eval-mode QuantConv2d(gf-k, gf-j) on the GPU against P.quant_conv2d: free-running (the module's own scales, each
    mean |residual| within 1e-6) and with the oracle's scales injected."""
    conv = _gf_module(xs, ws, gi)
    c, _, _, _, _, _, _, (h, w) = MODULE_GEOS[gi]
    x = detgen.normal(f'planes.mod.x{gi}', (3, c, h, w), scale=1.3)
    conv.eval().to(DEV)
    with torch.no_grad():
        y = conv(x.to(DEV)).cpu()
    v = conv.last_act_scales.cpu()
    k = int(xs[3:])
    assert v.shape == (k, 3)
    resid = x.clamp(-2, 2).reshape(3, -1).clone()
    for q in range(k):
        assert torch.allclose(v[q].double(), resid.double().abs().mean(dim=1), rtol=1e-6, atol=0), (xs, q)
        resid = resid - v[q].view(-1, 1) * P.pm1(resid)
    ref = _module_ref(conv, x, list(v))
    assert rel_err(y, ref) <= TOL, (xs, ws, gi, rel_err(y, ref))
    details = {}
    ref2 = _module_ref(conv, x, None, details)
    conv.x_approximate._forced_scales = torch.stack([s.reshape(-1) for s in details['act_scales']]).to(DEV)
    try:
        with torch.no_grad():
            y2 = conv(x.to(DEV)).cpu()
    finally:
        conv.x_approximate._forced_scales = None
    assert rel_err(y2, ref2) <= TOL, (xs, ws, gi, rel_err(y2, ref2))


@pytest.mark.parametrize('xs,ws', [('gf-8', 'gf-2'), ('gf-4', 'gf-3')])
def test_quant_conv2d_moving_average_k_scales(xs, ws):
    """moving_average_mode='eval_only': the k stored averages are the given scales of every sample."""
    conv = _gf_module(xs, ws, 0, mode='eval_only')
    k = int(xs[3:])
    avg = torch.tensor([0.9 / 2 ** i for i in range(k)])
    with torch.no_grad():
        conv.x_approximate.moving_avg_module.moving_average.copy_(avg)
    x = detgen.normal('planes.mod.ma', (4, 64, 9, 9), scale=1.3)
    conv.eval().to(DEV)
    with torch.no_grad():
        y = conv(x.to(DEV)).cpu()
    assert torch.equal(conv.last_act_scales.cpu(), avg.view(-1, 1).expand(k, 4))
    ref = _module_ref(conv, x, [torch.full((4,), float(a)) for a in avg])
    assert rel_err(y, ref) <= TOL, (xs, ws, rel_err(y, ref))


def test_small_resnet_gf4_gf3_every_fused_layer():
    """QResNet (xnor blocks, double shortcuts, 64 / 128 / 256 channels) with gf-4 activations and gf-3 weights, batch 8 of
    3x32x32 through the fused forward: every QuantConv2d.fused_forward call is recorded in place and checked against an
    fp64 convolution of what it quantized (eval batch norm folded as one fma per element, the kernel's read) with the
    layer's own GPU scales, epilogue included; the scales are mean |residual| within 1e-6."""
    from quant.binary.binary_conv import QuantConv2d
    from quant.models.resnet import QResNet

    def layer():
        return {'x_quant': 'gf-4', 'w_quant': 'gf-3', 'clamp': {'kind': 'symmetric', 'alpha': 3}, 'double_shortcut': True}
    arch = {'moving_average_mode': 'off', 'moving_average_momentum': 0.9, 'block': 'xnor',
            'layer0': {'n_in_channels': 64, 'kernel_size': 3, 'stride': 1, 'padding': 1, 'bias': False,
                       'maxpool': {'type': 'identity'}},
            'layer1': layer(), 'layer2': layer(), 'layer3': layer(), 'layer4': None,
            'nonlins': ['relu', 'relu'], 'num_blocks': [1, 1, 1], 'output_classes': 10}
    model = QResNet(loss_fn=F.cross_entropy, **arch)
    detgen.fill_module(model, seed=9)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, QuantConv2d):
                for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight, 'gf-3')):
                    buf.copy_(v)
    model.eval().to(DEV)
    x = detgen.normal('planes.resnet.x', (8, 3, 32, 32))
    seen = []
    orig = QuantConv2d.fused_forward

    def spy(self, xin, pre_bn=None, relu=False, res_pre=None, res_post=None, prelu=None, next_q=None, res_ready=None):
        out = orig(self, xin, pre_bn, relu, res_pre, res_post, prelu, next_q, res_ready)
        cp = lambda t: None if t is None else t.detach().clone()        # noqa: E731
        seen.append((self, pre_bn, relu, cp(prelu), cp(xin), cp(res_pre), cp(res_post), cp(out), self.last_act_scales.clone()))
        return out
    QuantConv2d.fused_forward = spy
    try:
        with torch.no_grad():
            model(x.to(DEV))
    finally:
        QuantConv2d.fused_forward = orig
    assert len(seen) == 6
    for li, (conv, bn, relu, slope, xin, rpre, rpost, yout, scales) in enumerate(seen):
        alpha = conv._alpha()
        s, t = conv._folded_bn(bn)
        xb = (xin.double() * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1)).float().cpu()
        xc = xb.clamp(-alpha, alpha)
        sc = scales.cpu()
        assert sc.shape == (4, 8)
        resid = xc.reshape(8, -1).clone()
        for q in range(4):
            assert torch.allclose(sc[q].double(), resid.double().abs().mean(dim=1), rtol=1e-6, atol=0), (li, q)
            resid = resid - sc[q].view(-1, 1) * P.pm1(resid)
        xq = P.quant_gf(xc, 4, list(sc))[1]
        wq = P.quantize_weight(conv.weight.detach().cpu(), 'gf-3', [b.cpu() for b in conv.w_approximate.cached_scales()])
        ref = F.conv2d(xq.double(), wq.double(), None if conv.bias is None else conv.bias.detach().cpu().double(),
                       conv.stride, conv.padding)
        if rpre is not None:
            ref = ref + rpre.cpu().double()
        if relu:
            ref = ref.clamp_min(0)
        if slope is not None:
            ref = torch.where(ref > 0, ref, ref * slope.cpu().double().view(1, -1, 1, 1))
        if rpost is not None:
            ref = ref + rpost.cpu().double()
        assert rel_err(yout, ref) <= TOL, (li, rel_err(yout, ref))


# ================================================================================================ 8. the limit
def test_gf9_takes_the_torch_formulation(monkeypatch):
    """gf-9 on either side is beyond LSQ_MAX_PLANES: _hip_supports is False, no kernel is called, and the module's output
    on the device is the torch formulation's."""
    from quant import _hip as hipmod
    from quant.binary import QuantLinear
    from quant.binary.binary_conv import QuantConv2d

    def boom(*a, **k):
        raise AssertionError('a HIP kernel was called for a gf-9 module')
    for name in ('act_quant', 'pack_weight', 'xnor_conv2d', 'signw_conv2d', 'linear_xnor'):
        monkeypatch.setattr(hipmod, name, boom)
    for xs, ws in (('gf-9', 'gf-2'), ('gf-2', 'gf-9')):
        conv = _gf_module(xs, ws, 0).eval().to(DEV)
        x = detgen.normal('planes.gf9.x', (2, 64, 6, 6), scale=1.3).to(DEV)
        assert not conv._hip_supports(x)
        with torch.no_grad():
            y, want = conv(x), conv._forward_torch(x)
        assert torch.equal(y, want), (xs, ws)
        lin = QuantLinear(xs, ws, 64, 16, CLAMP)
        detgen.fill_module(lin, seed=3)
        lin.eval().to(DEV)
        xl = detgen.normal('planes.gf9.xl', (5, 64)).to(DEV)
        assert not lin._hip_supports(xl)
        with torch.no_grad():
            assert torch.equal(lin(xl), lin._forward_torch(xl)), (xs, ws)


def test_entry_points_refuse_nine_planes():
    """Every C entry point given 9 planes returns nonzero and leaves its sentinel-filled outputs untouched (every buffer
    is sized for 9 planes, so a missing check could not reach outside it either)."""
    hip = _hip()
    lib, st = hip.lib(), hip.stream_ptr(torch.device(DEV))
    n, c, h, w, o, k = 2, 64, 6, 6, 32, 9
    g = hip.make_geom(n, c, h, w, o, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    aw, ww = hip.act_plane_words(g), lib.lsq_weight_plane_words(ctypes.byref(g))
    ho, wo = hip.out_hw(g)
    sent = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A, torch.float32: 1234.5}
    x = detgen.normal('planes.nine.x', (n, c, h, w)).to(DEV)
    wt = detgen.normal('planes.nine.w', (o, c, 3, 3)).to(DEV)
    xplanes = torch.zeros((k * aw,), dtype=torch.int64, device=DEV)
    xs = torch.full((k, n), 0.5, device=DEV)
    wbits = torch.zeros((k * ww,), dtype=torch.int64, device=DEV)
    wsum = torch.zeros((k, o, 9), dtype=torch.int32, device=DEV)
    wsc = torch.full((k, o), 0.5, device=DEV)

    def sentinel(shape, dtype=torch.float32):
        return torch.full(shape, sent[dtype], dtype=dtype, device=DEV)

    def untouched(*ts):
        torch.cuda.synchronize()
        return all(torch.equal(t, sentinel(t.shape, t.dtype)) for t in ts)

    planes, scales = sentinel((k * aw,), torch.int64), sentinel((k, n))
    ws = hip.sweep_workspace(n, x.device)
    assert lib.lsq_act_quant(x.data_ptr(), ctypes.byref(g), GF, k, 3, 2.0, None, None, None, planes.data_ptr(), scales.data_ptr(),
                             ws.data_ptr(), ws.numel(), st) != 0
    assert untouched(planes, scales), 'act_quant'
    pb, ps = sentinel((k * ww,), torch.int64), sentinel((k, o, 9), torch.int32)
    assert lib.lsq_pack_weight(wt.data_ptr(), ctypes.byref(g), k, wsc.data_ptr(), pb.data_ptr(), ps.data_ptr(), st) != 0
    assert untouched(pb, ps), 'pack_weight'
    for kx, kw in ((9, 1), (1, 9)):
        y = sentinel((n, o, ho, wo))
        assert lib.lsq_xnor_conv2d(xplanes.data_ptr(), kx, xs.data_ptr(), wbits.data_ptr(), wsum.data_ptr(), kw, wsc.data_ptr(), None,
                                   ctypes.byref(g), 0, None, None, None, y.data_ptr(), st) != 0
        assert untouched(y), ('xnor_conv2d', kx, kw)
    y = sentinel((n, o, ho, wo))
    assert lib.lsq_signw_conv2d(x.data_ptr(), 2.0, None, None, wbits.data_ptr(), None, k, wsc.data_ptr(), None, ctypes.byref(g), 0,
                                None, None, None, y.data_ptr(), st) != 0
    assert untouched(y), 'signw_conv2d'
    m, f = n, c * h * w                           # linear over the flattened rows: nw = f / 64 words per row and plane
    lplanes = torch.zeros((k * m * (f // 64),), dtype=torch.int64, device=DEV)
    lbits = torch.zeros((k * (f // 64) * o,), dtype=torch.int64, device=DEV)
    for kx, kw in ((9, 1), (1, 9)):
        y = sentinel((m, o))
        assert hip.linear_lib().lsq_linear_xnor(lplanes.data_ptr(), kx, xs.data_ptr(), 1, lbits.data_ptr(), wsum.data_ptr(), kw,
                                                wsc.data_ptr(), None, m, f, o, y.data_ptr(), st) != 0
        assert untouched(y), ('linear_xnor', kx, kw)
    rows = torch.full((k, n), 0.5, device=DEV)
    out = sentinel(tuple(x.shape))
    assert lib.lsq_quant_values(x.data_ptr(), n, c * h * w, k, rows.data_ptr(), 2.0, out.data_ptr(), st) != 0
    assert untouched(out), 'quant_values'
    out = sentinel(tuple(x.shape))
    assert lib.lsq_ste_backward(x.data_ptr(), x.data_ptr(), n, c * h * w, k, rows.data_ptr(), 2.0, out.data_ptr(), st) != 0
    assert untouched(out), 'ste_backward'
    gy = detgen.normal('planes.nine.gy', (n, o, ho, wo)).to(DEV)
    out = sentinel((o, c, 3, 3))
    assert hip.train_lib().lsq_train_wgrad(xplanes.data_ptr(), k, xs.data_ptr(), gy.data_ptr(), ctypes.byref(g), out.data_ptr(),
                                           None, 0, st) != 0
    assert untouched(out), 'train_wgrad'
