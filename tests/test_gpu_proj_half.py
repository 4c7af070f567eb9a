"""lsq_pointwise_conv_half and lsq_xnor_conv2d_proj_half (include/lsq_hip_conv_proj_half.h; the __bf16 / _Float16 instantiations
of csrc/lsq_pointwise.hip and of the PROJ kernels of csrc/lsq_xnor_mfma.hip) on the GPU, bf16 and fp16.

Every contract is bit equality, every comparison torch.equal on the raw 16-bit patterns -- no tolerance anywhere:
  * lsq_pointwise_conv_half(x) == lsq_pointwise_conv(x.float()).to(dtype), over every kernel variant (the shapes of
    tests/golden/projection_cases.py; tests/test_proj_half_host.py shows which variant each reaches), and with the small integer
    grid of tests/golden/proj_half_cases.py == the exact integer answer (at most 256 in magnitude: a value of both types);
  * tensors that start one element into a storage are served, with the bits of the aligned call, and nothing outside y is
    written;
  * lsq_xnor_conv2d_proj_half == lsq_xnor_conv2d_proj on the widened operands, .to(dtype): ONE rounding;
  * refused calls write nothing."""

import ctypes

import pytest
import torch

import detgen
import proj_half_cases as PH
import projection_cases as PC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
CODES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
LS2, LST = 2, 3
E_SCHEME, E_UNSUPPORTED = -3, -6
MARGIN = 256            # elements on either side of a guarded tensor (even: one element further in is 2-byte aligned, no more)


def _hip():
    from quant import _hip
    return _hip


def _bits(y):
    assert y.dtype in (torch.bfloat16, torch.float16)
    return y.contiguous().view(torch.int16)


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------ lsq_pointwise_conv_half
@pytest.mark.parametrize('case', [c for c, _ in PC.PW_CASES], ids=[PC.pw_id(c) for c, _ in PC.PW_CASES])
def test_pointwise_half_on_every_variant(case):
    hip = _hip()
    n, c, h, w, o, stride = case
    # the anchor: integer operands, the exact answer in fp64 -- an integer of at most 256, so 16-bit rounding is the identity
    gx, gw, gb = (t.to(DEV) for t in PH.grid_operands(case))
    xs = gx[:, :, ::stride, ::stride].double()
    ho, wo = xs.shape[2:]
    exact = torch.matmul(gw.double(), xs.reshape(n, c, ho * wo)).reshape(n, o, ho, wo) + gb.double().view(1, -1, 1, 1)
    assert float(exact.abs().max()) <= PH.ANCHOR_MAX and torch.equal(exact, exact.round())
    # normal-distributed operands: the fp32 kernel on the widened input, rounded once
    nx = detgen.normal(f'projh.{PC.pw_id(case)}.nx', (n, c, h, w), scale=0.9).to(DEV)
    nw = detgen.normal(f'projh.{PC.pw_id(case)}.nw', (o, c), scale=c ** -0.5).to(DEV)
    nb = detgen.normal(f'projh.{PC.pw_id(case)}.nb', (o,), scale=0.3).to(DEV)
    for name, dtype in DTYPES.items():
        got = hip.pointwise_conv_half(gx.to(dtype), gw, gb, stride)
        assert got.dtype == dtype and got.shape == exact.shape
        assert torch.equal(got.double(), exact), (case, name, 'anchor', float((got.double() - exact).abs().max()))
        x16 = nx.to(dtype)
        for bias in (nb, None):
            want = hip.pointwise_conv(x16.float(), nw, bias, stride).to(dtype)
            got = hip.pointwise_conv_half(x16, nw, bias, stride)
            differ = int((_bits(got) != _bits(want)).sum())
            print(f'{PC.pw_id(case)} {name} bias={bias is not None}: {differ} of {want.numel()} outputs differ')
            assert _same(got, want), (case, name, bias is not None, differ)


def _raw_pointwise(x, w, b, stride, y, dtype_code):
    hip = _hip()
    n, c, h, wd = x.shape
    hip.lib()
    return hip.conv_proj_half_lib().lsq_pointwise_conv_half(x.data_ptr(), dtype_code, n, c, h, wd, w.data_ptr(), b.data_ptr(),
                                                            w.shape[0], stride, y.data_ptr(), hip.stream_ptr(torch.device(DEV)))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', PH.UNALIGNED_CASES, ids=[PC.pw_id(c) for c in PH.UNALIGNED_CASES])
def test_operands_one_element_into_their_storage(case, dt):
    hip = _hip()
    dtype = DTYPES[dt]
    n, c, h, w, o, stride = case
    x = detgen.normal(f'projh.{PC.pw_id(case)}.ux', (n, c, h, w), scale=0.9).to(DEV).to(dtype)
    wt = detgen.normal(f'projh.{PC.pw_id(case)}.uw', (o, c), scale=c ** -0.5).to(DEV)
    b = detgen.normal(f'projh.{PC.pw_id(case)}.ub', (o,), scale=0.3).to(DEV)
    aligned = hip.pointwise_conv_half(x, wt, b, stride)
    assert x.data_ptr() % 16 == 0 and aligned.data_ptr() % 16 == 0
    assert _same(aligned, hip.pointwise_conv(x.float(), wt, b, stride).to(dtype))
    xbuf = torch.full((x.numel() + 2 * MARGIN,), float('nan'), dtype=dtype, device=DEV)
    ybuf = torch.full((aligned.numel() + 2 * MARGIN,), float('nan'), dtype=dtype, device=DEV)
    xin = xbuf[MARGIN + 1:MARGIN + 1 + x.numel()].view(x.shape)
    yin = ybuf[MARGIN + 1:MARGIN + 1 + aligned.numel()].view(aligned.shape)
    xin.copy_(x)
    assert xin.data_ptr() % 4 == 2 and yin.data_ptr() % 4 == 2 and xin.is_contiguous() and yin.is_contiguous()
    assert PH.half_variant(case, xin.data_ptr(), yin.data_ptr())[2:] in ((False, False), ())      # the scalar-access variants
    assert _raw_pointwise(xin, wt, b, stride, yin, CODES[dtype]) == 0
    torch.cuda.synchronize()
    assert torch.isnan(ybuf[:MARGIN + 1]).all() and torch.isnan(ybuf[MARGIN + 1 + aligned.numel():]).all(), 'written outside y'
    assert not torch.isnan(yin).any(), 'outputs left unwritten'
    assert _same(yin, aligned)
    # x alone unaligned (the pair load falls back, the 8-byte store stays) and y alone unaligned
    y2 = torch.full_like(aligned, float('nan'))
    assert _raw_pointwise(xin, wt, b, stride, y2, CODES[dtype]) == 0 and _same(y2, aligned)
    ybuf.fill_(float('nan'))
    assert _raw_pointwise(x, wt, b, stride, yin, CODES[dtype]) == 0 and _same(yin, aligned)
    assert torch.isnan(ybuf[:MARGIN + 1]).all() and torch.isnan(ybuf[MARGIN + 1 + aligned.numel():]).all(), 'written outside y'


def test_pointwise_half_refusals_write_nothing():
    x = torch.zeros((2, 64, 6, 6), dtype=torch.bfloat16, device=DEV)
    w = torch.zeros((64, 64), device=DEV)
    b = torch.zeros((64,), device=DEV)
    y = torch.full((2, 64, 3, 3), float('nan'), dtype=torch.bfloat16, device=DEV)
    assert _raw_pointwise(x, w, b, 2, y, 0) == E_UNSUPPORTED and _raw_pointwise(x, w, b, 2, y, 3) == E_UNSUPPORTED       # another dtype
    assert _raw_pointwise(x, w, b, 0, y, 1) == -2                                                                     # LSQ_E_SHAPE, as lsq_pointwise_conv
    assert _raw_pointwise(x[:, :48].contiguous(), w[:, :48].contiguous(), b, 2, y, 1) == E_UNSUPPORTED               # C = 48
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
    with pytest.raises(TypeError):
        _hip().pointwise_conv_half(x.float(), w, b, 2)


# ---------------------------------------------------------------------------------------------- lsq_xnor_conv2d_proj_half
# name: (N, consumer C, consumer input H x W, consumer stride, O, projection Cp, projection input H x W) -- the five small cases of
# tests/test_gpu_proj_fused.py, restated
CASES = {
    'c64_o128': (3, 64, (12, 12), 2, 128, 64, (12, 12)),       # 108 pixels: tiles straddle images, the last one is partial
    'c128_o256': (2, 128, (10, 6), 2, 256, 128, (10, 6)),      # odd Wo, 30 pixels: one partial tile
    'c256_o512_n1': (1, 256, (8, 8), 2, 512, 256, (8, 8)),     # 16 pixels, 16 out-channel tiles
    'c256_o512_n5': (5, 256, (8, 8), 2, 512, 256, (8, 8)),     # 80 pixels: several tiles
    'c64_o64_pre': (2, 64, (6, 6), 1, 64, 64, (12, 12)),       # stride-1 consumer, projection input at stride 2
}
ALL_CASES = {**CASES, **PC.FUSED_CASES, **PC.CP_CASES}
# (act, projection as res_post, projection bias): the three of tests/test_gpu_proj_fused.py
EPILOGUES = (('relu', True, True), ('prelu', False, True), ('none', True, False))
EVERY_EPILOGUE = tuple((act, post, with_bias) for act in ('none', 'relu', 'prelu') for post in (False, True) for with_bias in (True, False))


def _operands(name, scheme):
    """The operands of tests/test_gpu_proj_fused.py's cases; the projection's x in fp32 (each test rounds it into its type)."""
    hip = _hip()
    n, c, (h, w), s, o, cp, (hx, wx) = ALL_CASES[name]
    geom = hip.make_geom(n, c, h, w, o, 3, 3, (s, s), (1, 1), (1, 1), 1)
    x = detgen.normal(f'projh.{name}.x', (n, c, h, w), scale=1.2).to(DEV)
    planes = torch.zeros((2 * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xs = torch.empty((2, n), dtype=torch.float32, device=DEV)
    hip.act_quant(x, geom, scheme, 2, 3, 2.0, planes, xs)
    wt = detgen.uniform(f'projh.{name}.w', (o, c, 3, 3), -0.5, 0.5).to(DEV)
    wsc = wt.abs().mean(dim=(1, 2, 3))[None].contiguous()
    wbits, wsum = hip.pack_weight(wt, geom, wsc)
    ho, wo = hip.out_hw(geom)
    return dict(hip=hip, geom=geom, planes=planes, xs=xs, wbits=wbits, wsum=wsum, wsc=wsc,
                bias=detgen.normal(f'projh.{name}.b', (o,), scale=0.2).to(DEV),
                px=detgen.normal(f'projh.{name}.px', (n, cp, hx, wx), scale=0.9).to(DEV),
                pw=detgen.normal(f'projh.{name}.pw', (o, cp), scale=cp ** -0.5).to(DEV),
                pb=detgen.normal(f'projh.{name}.pb', (o,), scale=0.3).to(DEV),
                slope=detgen.uniform(f'projh.{name}.slope', (o,), 0.05, 0.4).to(DEV), yshape=(n, o, ho, wo))


def _fp32_fused(cs, px16, act, post, with_bias, res_pre=None, res_post=None):
    """lsq_xnor_conv2d_proj on the widened operands: the reference, before its one rounding."""
    hip = cs['hip']
    y = torch.full(cs['yshape'], float('nan'), device=DEV)
    took = hip.xnor_conv2d_proj(cs['planes'], 2, cs['xs'], cs['wbits'], cs['wsum'], cs['wsc'], cs['bias'], cs['geom'], y,
                                (px16.float(), cs['pw'], cs['pb'] if with_bias else None, 2, post), relu=act == 'relu',
                                res_pre=None if res_pre is None else res_pre.float(),
                                res_post=None if res_post is None else res_post.float(),
                                prelu=cs['slope'] if act == 'prelu' else None)
    assert took and not torch.isnan(y).any()
    return y


def _half_fused(cs, px16, act, post, with_bias, res_pre=None, res_post=None, y=None):
    hip = cs['hip']
    if y is None:
        y = torch.full(cs['yshape'], float('nan'), dtype=px16.dtype, device=DEV)
    took, out = hip.xnor_conv2d_proj_half(cs['planes'], 2, cs['xs'], cs['wbits'], cs['wsum'], cs['wsc'], cs['bias'], cs['geom'],
                                          (px16, cs['pw'], cs['pb'] if with_bias else None, 2, post), px16.dtype,
                                          relu=act == 'relu', res_pre=res_pre, res_post=res_post,
                                          prelu=cs['slope'] if act == 'prelu' else None, y=y)
    assert took, 'lsq_xnor_conv2d_proj_half refused a geometry it documents as supported'
    assert out is y and not torch.isnan(y).any(), 'outputs left unwritten'
    return y


def _check(cs, epilogues, where):
    for name, dtype in DTYPES.items():
        px16 = cs['px'].to(dtype)
        for act, post, with_bias in epilogues:
            want = _fp32_fused(cs, px16, act, post, with_bias).to(dtype)
            got = _half_fused(cs, px16, act, post, with_bias)
            differ = int((_bits(got) != _bits(want)).sum())
            print(f'{where} {name} {act} post={post} bias={with_bias}: {differ} of {want.numel()} outputs differ')
            assert _same(got, want), (where, name, act, post, with_bias, differ)


@pytest.mark.parametrize('scheme', [LS2, LST], ids=['ls-2', 'ls-T'])
@pytest.mark.parametrize('name', list(CASES))
def test_fused_half_equals_the_fp32_kernel_rounded_once(name, scheme):
    _check(_operands(name, scheme), EVERY_EPILOGUE, (name, scheme))


@pytest.mark.parametrize('name', list(PC.FUSED_CASES) + list(PC.CP_CASES))
def test_fused_half_on_multi_tile_waves_and_every_channel_count(name):
    _check(_operands(name, LS2), EPILOGUES, name)


def test_a_16_bit_res_post_tensor_beside_a_res_pre_projection():
    cs = _operands('c64_o64_pre', LS2)
    for name, dtype in DTYPES.items():
        px16 = cs['px'].to(dtype)
        other = detgen.normal('projh.other', cs['yshape'], scale=0.7).to(DEV).to(dtype)
        want = _fp32_fused(cs, px16, 'relu', False, True, res_post=other).to(dtype)
        got = _half_fused(cs, px16, 'relu', False, True, res_post=other)
        assert _same(got, want), name


@pytest.mark.parametrize('dt', DTYPES)
def test_fused_half_writes_all_of_y_and_nothing_else_twice_the_same(dt):
    dtype = DTYPES[dt]
    cs = _operands(PC.FUSED_PARTIAL, LS2)
    px16 = cs['px'].to(dtype)
    first = _half_fused(cs, px16, 'relu', True, True)
    second = _half_fused(cs, px16, 'relu', True, True)
    assert _same(first, second)
    numel = first.numel()
    buf = torch.full((numel + 2 * MARGIN,), float('nan'), dtype=dtype, device=DEV)
    inside = buf[MARGIN + 1:MARGIN + 1 + numel].view(cs['yshape'])          # one element in: 2-byte alignment, no more
    assert inside.data_ptr() % 4 == 2
    _half_fused(cs, px16, 'relu', True, True, y=inside)
    assert torch.isnan(buf[:MARGIN + 1]).all() and torch.isnan(buf[MARGIN + 1 + numel:]).all(), 'written outside y'
    assert _same(inside, first)


def _raw_fused(cs, kx, px16, dtype_code, y, cp=None, res_pre=None, res_post=None, post=0):
    from quant import _sublibs
    hip = cs['hip']
    pd = _sublibs.ProjHalf(px16.data_ptr(), cs['pw'].data_ptr(), cs['pb'].data_ptr(), px16.shape[1] if cp is None else cp,
                           px16.shape[2], px16.shape[3], 2, post)
    hip.lib()
    return hip.conv_proj_half_lib().lsq_xnor_conv2d_proj_half(
        cs['planes'].data_ptr(), kx, cs['xs'].data_ptr(), cs['wbits'].data_ptr(), cs['wsum'].data_ptr(), 1, cs['wsc'].data_ptr(),
        cs['bias'].data_ptr(), ctypes.byref(cs['geom']), 1, None, None if res_pre is None else res_pre.data_ptr(),
        None if res_post is None else res_post.data_ptr(), ctypes.byref(pd), dtype_code, y.data_ptr(),
        hip.stream_ptr(torch.device(DEV)))


def test_fused_half_refusals_write_nothing():
    cs = _operands('c64_o128', LS2)
    px16 = cs['px'].to(torch.bfloat16)
    y = torch.full(cs['yshape'], float('nan'), dtype=torch.bfloat16, device=DEV)
    res = torch.zeros(cs['yshape'], dtype=torch.bfloat16, device=DEV)
    assert _raw_fused(cs, 2, px16, 0, y) == E_UNSUPPORTED and _raw_fused(cs, 2, px16, 3, y) == E_UNSUPPORTED      # another dtype
    assert _raw_fused(cs, 2, px16, 1, y, res_pre=res, post=0) == E_SCHEME                                         # a tensor in the projection's slot
    assert _raw_fused(cs, 2, px16, 1, y, res_post=res, post=1) == E_SCHEME
    assert _raw_fused(cs, 1, px16, 1, y) == E_UNSUPPORTED                                                         # kx = 1
    assert _raw_fused(cs, 2, px16, 1, y, cp=96) == E_UNSUPPORTED                                                  # Cp = 96
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
    assert _raw_fused(cs, 2, px16, 1, y) == 0                                                                     # (the operands themselves are fine)
    torch.cuda.synchronize()
    assert not torch.isnan(y).any()
