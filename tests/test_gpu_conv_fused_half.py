"""lsq_signw_conv2d_fused_half (liblsq_hip_conv_fused_half.so) on the GPU: the contract of include/lsq_hip_conv_fused_half.h
against the EXISTING lsq_signw_conv2d_half on the folded tensor t composed in fp32 with torch (torch.equal: values), on every
case of tests/golden/conv_half_cases.py with the variants of tests/golden/conv_fused_half_cases.py; the identity bit for bit;
an exact integer anchor; accuracy against fp64; unaligned operands and guards; fp16 overflow of the folded value; refused
calls; the planes.

Every test prints the figure it asserts on (pytest -s shows them)."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_fused_half_cases as FC
import conv_half_cases as C
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = C.DTYPES
IDS = [c.id for c in C.CASES]
E_NULL, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5, -6


def _hip():
    from quant import _hip
    return _hip


def _bits(y):
    return y.contiguous().view(torch.int32 if y.dtype == torch.float32 else torch.int16)


_OPERANDS = {}


def _operands(cid, dt):
    """Operands of a case on the GPU, made once and shared (nothing below writes into them)."""
    key = (cid, dt)
    if key not in _OPERANDS:
        hip = _hip()
        c = C.BY_ID[cid]
        w, wsc, _, b = C.weights(cid)
        g = hip.make_geom(c.N, c.C, c.H, c.W, c.O, c.KH, c.KW, c.stride, c.pad, c.dil, c.groups)
        wbits, _ = hip.pack_weight(w.to(DEV), g, wsc.to(DEV))
        s, sh = FC.folded_bn(cid)
        _OPERANDS[key] = dict(c=c, g=g, x=C.batch(cid, dt).to(DEV), wbits=wbits, wsc=wsc.to(DEV), b=None if b is None else b.to(DEV),
                              alpha=C.alpha_in(C.ALPHAS[c.alpha], DTYPES[dt]), dtype=DTYPES[dt], pre=(s.to(DEV), sh.to(DEV)),
                              res_pre=FC.residual(cid, 'pre', dt).to(DEV), res_post=FC.residual(cid, 'post', dt).to(DEV),
                              one=FC.slopes(cid, 'one').to(DEV), channel=FC.slopes(cid, 'channel').to(DEV))
    return _OPERANDS[key]


def _args(p, v):
    """The epilogue's keyword arguments of variant ``v``."""
    return dict(relu=v.relu, prelu=None if v.prelu is None else p[v.prelu], res_pre=p['res_pre'] if v.res_pre else None,
                res_post=p['res_post'] if v.res_post else None)


def _fused(p, v, bn, out_dtype, planes=None, x=None, alpha=None):
    wsc = p['wsc'] if planes is None else p['wsc'][:planes].contiguous()
    return _hip().signw_conv2d_fused_half(p['x'] if x is None else x, p['alpha'] if alpha is None else alpha, p['wbits'], wsc, p['b'],
                                          p['g'], pre=p['pre'] if bn else None, out_dtype=out_dtype, **_args(p, v))


def _composition(p, v, bn, out_dtype, planes=None, x=None, alpha=None):
    """The contract's right-hand side: t in torch (two eager fp32 operations, one rounding), the EXISTING unfused kernel with
    an fp32 y, the epilogue in fp32 on the device, one rounding."""
    x = p['x'] if x is None else x
    t = FC.folded_input(x, p['pre']) if bn else x
    wsc = p['wsc'] if planes is None else p['wsc'][:planes].contiguous()
    y32 = _hip().signw_conv2d_half(t, p['alpha'] if alpha is None else alpha, p['wbits'], wsc, p['b'], p['g'], out_dtype=torch.float32)
    a = _args(p, v)
    return FC.compose(y32, v, a['res_pre'], a['res_post'], a['prelu']).to(out_dtype)


def _check(tag, y, ref):
    differ = int((y != ref).sum())
    print(f'{tag}: {differ} of {y.numel()} values differ from the composition')
    assert y.dtype == ref.dtype and y.shape == ref.shape and torch.isfinite(ref.float()).all()
    assert torch.equal(y, ref)


@pytest.mark.parametrize('cid', IDS)
@pytest.mark.parametrize('bn', (False, True), ids=('plain', 'bn'))
@pytest.mark.parametrize('dt', DTYPES)
def test_contract(dt, bn, cid):
    """Every case with its variant, with and without a folded batch norm, both output types."""
    p = _operands(cid, dt)
    v = FC.VARIANT_OF[cid]
    for out_dtype in (p['dtype'], torch.float32):
        _check(f'{cid} {dt} {v.id} bn={bn} y={out_dtype}', _fused(p, v, bn, out_dtype), _composition(p, v, bn, out_dtype))


@pytest.mark.parametrize('vid', [v.id for v in FC.VARIANTS])
@pytest.mark.parametrize('cid', FC.CROSS)
@pytest.mark.parametrize('dt', DTYPES)
def test_full_cross(dt, cid, vid):
    p = _operands(cid, dt)
    v = FC.VARIANT_BY_ID[vid]
    for bn in (False, True):
        _check(f'{cid} {dt} {vid} bn={bn}', _fused(p, v, bn, p['dtype']), _composition(p, v, bn, p['dtype']))


@pytest.mark.parametrize('cid', IDS)
@pytest.mark.parametrize('dt', DTYPES)
def test_identity_is_the_unfused_call_bit_for_bit(dt, cid):
    hip = _hip()
    p = _operands(cid, dt)
    for out_dtype in (p['dtype'], torch.float32):
        y = _fused(p, FC.VARIANT_BY_ID['none'], False, out_dtype)
        ref = hip.signw_conv2d_half(p['x'], p['alpha'], p['wbits'], p['wsc'], p['b'], p['g'], out_dtype=out_dtype)
        differ = int((_bits(y) != _bits(ref)).sum())
        print(f'{cid} {dt} y={out_dtype}: {differ} bit patterns differ from lsq_signw_conv2d_half')
        assert differ == 0


@pytest.mark.parametrize('dt', DTYPES)
def test_exact_integer_anchor(dt):
    """x of small integers, an all-(+1) 1x1 plane of scale 1, pre_scale 2, pre_shift -1, no clamp, integer residuals:
    y = prelu(sum_c (2 x_c - 1) + res_pre) + res_post exactly, with slope 0.25 (every sum is kept a multiple of 4)."""
    hip = _hip()
    dtype = DTYPES[dt]
    n, ch, h, w, o = 2, 24, 5, 7, 6
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (n, ch, h, w), generator=gen)
    res_pre = torch.randint(-8, 9, (n, o, h, w), generator=gen)
    res_post = torch.randint(-8, 9, (n, o, h, w), generator=gen)
    s = (2 * x - 1).sum(1, keepdim=True).expand(n, o, h, w)
    res_pre = res_pre - (s + res_pre) % 4                       # s + res_pre a multiple of 4: the PReLU branch is exact
    v = s + res_pre
    want = torch.where(v > 0, v, v // 4) + res_post
    assert want.abs().max() < 256 and (want < 0).any() and (want > 0).any()
    g = hip.make_geom(n, ch, h, w, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    wsc = torch.ones((1, o), device=DEV)
    wbits, _ = hip.pack_weight(torch.ones((o, ch, 1, 1), device=DEV), g, wsc)
    pre = (torch.full((ch,), 2.0, device=DEV), torch.full((ch,), -1.0, device=DEV))
    for out_dtype in (dtype, torch.float32):
        y = hip.signw_conv2d_fused_half(x.to(dtype).to(DEV), -1.0, wbits, wsc, None, g, pre=pre, res_pre=res_pre.to(dtype).to(DEV),
                                        res_post=res_post.to(dtype).to(DEV), prelu=torch.tensor([0.25], device=DEV),
                                        out_dtype=out_dtype)
        differ = int((y.cpu().double() != want.double()).sum())
        print(f'{dt} y={out_dtype}: {differ} of {y.numel()} outputs differ from the integer closed form')
        assert differ == 0


_WORST = {}


@pytest.mark.parametrize('cid', IDS)
@pytest.mark.parametrize('dt', DTYPES)
def test_accuracy_against_fp64(dt, cid):
    """max|y - y64| / max|y64| against the fp64 composition on t: one rounding of the output, (2^-8 | 2^-11) + 1e-5."""
    p = _operands(cid, dt)
    c, v = p['c'], FC.VARIANT_OF[cid]
    w, _, sc, b = C.weights(cid)
    wq = P.quantize_weight(w, c.ws, sc)
    t = FC.folded_input(C.batch(cid, dt), FC.folded_bn(cid))
    a = C.ALPHAS[c.alpha]
    tc = t.clamp(-a, a) if a >= 0 else t
    y64 = F.conv2d(tc.double(), wq.double(), None if b is None else b.double(), c.stride, c.pad, c.dil, c.groups)
    y64 = FC.compose(y64, v, FC.residual(cid, 'pre', dt), FC.residual(cid, 'post', dt),
                     None if v.prelu is None else FC.slopes(cid, v.prelu))
    y = _fused(p, v, True, p['dtype'])
    err = ((y.cpu().double() - y64).abs().max() / y64.abs().max()).item()
    bound = (2.0 ** -8 if dt == 'bf16' else 2.0 ** -11) + 1e-5
    _WORST[dt] = max(_WORST.get(dt, 0.0), err)
    print(f'{cid} {dt} {v.id}: max err / max|y64| = {err:.3e} (bound {bound:.3e}); worst so far {_WORST[dt]:.3e}')
    assert err <= bound


@pytest.mark.parametrize('cid', ('p1_wide', 's2_narrow', 'proj_wide'))
@pytest.mark.parametrize('dt', DTYPES)
def test_address_and_layout(dt, cid):
    """x, both residuals and y as views one element into larger buffers (2-byte alignment only); guards on both sides of y
    keep their pattern; the same bits as the aligned call."""
    hip = _hip()
    p = _operands(cid, dt)
    v = FC.VARIANT_BY_ID['preluC_both']
    want = _fused(p, v, True, p['dtype'])

    def shifted(t):
        buf = torch.zeros((t.numel() + 1,), dtype=t.dtype, device=DEV)
        out = buf[1:].view(t.shape)
        out.copy_(t)
        assert out.data_ptr() % 4 == 2 and out.is_contiguous()
        return out

    x, rpre, rpost = shifted(p['x']), shifted(p['res_pre']), shifted(p['res_post'])
    n = want.numel()
    guard = 3 if n % 2 == 0 else 4
    out = torch.full((n + 1 + guard,), 77.0, dtype=p['dtype'], device=DEV)
    yv = out[1:1 + n]
    assert yv.data_ptr() % 4 == 2
    lib = hip.conv_fused_half_lib()
    g, kw = p['g'], p['wsc'].shape[0]
    ydt = hip.LINEAR_HALF_DTYPES[p['dtype']]
    need = int(lib.lsq_signw_conv2d_fused_half_workspace_bytes(ctypes.byref(g), kw, ydt))
    ws = torch.empty((max(need, 4),), dtype=torch.uint8, device=DEV)
    rc = lib.lsq_signw_conv2d_fused_half(x.data_ptr(), ydt, p['alpha'], p['pre'][0].data_ptr(), p['pre'][1].data_ptr(),
                                         p['wbits'].data_ptr(), kw, p['wsc'].data_ptr(), hip.ptr(p['b']), ctypes.byref(g),
                                         hip.ACT_PRELU_CHANNEL, p['channel'].data_ptr(), rpre.data_ptr(), rpost.data_ptr(),
                                         yv.data_ptr(), ydt, ws.data_ptr(), ws.numel(), hip.stream_ptr(DEV))
    torch.cuda.synchronize()
    intact = bool((out[:1] == 77.0).all() and (out[1 + n:] == 77.0).all())
    inner = int((_bits(yv) != _bits(want).view(-1)).sum())
    print(f'{cid} {dt}: code {rc}, guards intact: {intact}, {inner} outputs differ from the aligned call')
    assert rc == 0 and intact and inner == 0


def test_fp16_overflow_of_the_folded_value_enters_as_the_bound():
    """A scale that pushes one element past 65504: t is +-inf, and under a finite bound it enters as +-bound."""
    p = _operands('p1_narrow', 'fp16')
    x = p['x'].clone()
    x[0, 3, 4, 4], x[1, 3, 2, 2] = 40.0, -40.0
    s, b = (t.clone() for t in p['pre'])
    s[3] = 2000.0
    pre = (s, b)
    q = dict(p, pre=pre)
    t = FC.folded_input(x, pre)
    assert int(torch.isinf(t).sum()) == 2
    v = FC.VARIANT_BY_ID['relu_pre']
    y, ref = _fused(q, v, True, torch.float16, x=x, alpha=2.0), _composition(q, v, True, torch.float16, x=x, alpha=2.0)
    _check('fp16 overflow under a bound of 2', y, ref)


def test_refused_calls_write_nothing():
    hip = _hip()
    p = _operands('gf8_patch', 'bf16')
    lib = hip.conv_fused_half_lib()
    code = hip.LINEAR_HALF_DTYPES
    bf, fp, f32 = code[torch.bfloat16], code[torch.float16], code[torch.float32]
    g, c = p['g'], p['c']
    n = p['res_pre'].numel()
    bad = hip.make_geom(c.N, c.C, c.H, c.W, c.O, 3, 3, (1, 1), (1, 1), (1, 1), 3)
    ps, pb, sl = p['pre'][0].data_ptr(), p['pre'][1].data_ptr(), p['channel'].data_ptr()
    # (geometry, x dtype, y dtype, planes, workspace bytes, pre_scale, pre_shift, act, slope, expected)
    refusals = ((g, f32, f32, 1, 4 * n, ps, pb, 1, None, E_UNSUPPORTED), (g, bf, fp, 1, 4 * n, ps, pb, 1, None, E_UNSUPPORTED),
                (g, bf, f32, 9, 4 * n, ps, pb, 1, None, E_UNSUPPORTED), (g, bf, bf, 8, 4 * n - 1, ps, pb, 1, None, E_WORKSPACE),
                (g, bf, bf, 2, 0, ps, pb, 1, None, E_WORKSPACE), (bad, bf, f32, 1, 4 * n, ps, pb, 1, None, E_SHAPE),
                (None, bf, f32, 1, 4 * n, ps, pb, 1, None, E_NULL), (g, bf, f32, 1, 4 * n, ps, None, 1, None, E_NULL),
                (g, bf, f32, 1, 4 * n, None, pb, 1, None, E_NULL), (g, bf, f32, 1, 4 * n, ps, pb, 2, None, E_NULL),
                (g, bf, f32, 1, 4 * n, ps, pb, 3, None, E_NULL), (g, bf, f32, 1, 4 * n, ps, pb, 4, sl, E_UNSUPPORTED),
                (g, bf, f32, 1, 4 * n, ps, pb, -1, sl, E_UNSUPPORTED))
    for geom, xdt, ydt, planes, wbytes, s, b, act, slope, expected in refusals:
        y = torch.full((n,), 123.0, device=DEV)
        ws = torch.full((n,), -5.0, device=DEV)
        rc = lib.lsq_signw_conv2d_fused_half(p['x'].data_ptr(), xdt, 2.0, s, b, p['wbits'].data_ptr(), planes, p['wsc'].data_ptr(),
                                             hip.ptr(p['b']), None if geom is None else ctypes.byref(geom), act, slope,
                                             p['res_pre'].data_ptr(), p['res_post'].data_ptr(), y.data_ptr(), ydt,
                                             ws.data_ptr() if wbytes else None, wbytes, hip.stream_ptr(DEV))
        torch.cuda.synchronize()
        print(f'x dtype {xdt}, y dtype {ydt}, planes {planes}, workspace {wbytes}, act {act}: code {rc}')
        assert rc == expected
        assert (y == 123.0).all() and (ws == -5.0).all()
    with pytest.raises(TypeError):
        hip.signw_conv2d_fused_half(p['x'], 2.0, p['wbits'], p['wsc'], p['b'], g, res_pre=p['res_pre'].float())
    with pytest.raises(ValueError):
        hip.signw_conv2d_fused_half(p['x'], 2.0, p['wbits'], p['wsc'], p['b'], g, res_post=p['res_post'][:1])


@pytest.mark.parametrize('planes', (1, 2, 3, 8))
@pytest.mark.parametrize('cid', ('gf8_patch', 'gf8_general'))
@pytest.mark.parametrize('dt', DTYPES)
def test_only_the_last_plane_applies_the_epilogue(dt, cid, planes):
    p = _operands(cid, dt)
    v = FC.VARIANT_BY_ID['relu_both']
    for out_dtype in (p['dtype'], torch.float32):
        _check(f'{cid} {dt} {planes} planes y={out_dtype}', _fused(p, v, True, out_dtype, planes=planes),
               _composition(p, v, True, out_dtype, planes=planes))
