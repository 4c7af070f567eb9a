"""lsq_xnor_conv2d_gen_half (include/lsq_hip_conv_xnor_gen_half.h, csrc/conv_xnor_gen_half): the general fp4 matrix-core XNOR
convolution with a 16-bit epilogue and every plane pass in one launch, against lsq_xnor_conv2d_half on the same operands
(equal, bit for bit) and against F.conv2d in fp64 of the quantized tensors (one rounding into the type on top of the fp32
bound, README "Outputs"), at the smallest geometries that reach each of the kernel's paths; the fused epilogue, the refusals
and the ``QuantConv2d.xnor_general_half`` switch."""

import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ALPHA = 3.0
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}

# id: (N, C, O, H, W, (KH, KW), stride, pad, dilation, activation scheme, activation planes, weight planes)
CASES = {
    'c192_1x1_two_samples': (2, 192, 64, 9, 9, (1, 1), (1, 1), (0, 0), (1, 1), 'ls1', 1, 1),
    '5x5': (2, 64, 32, 7, 7, (5, 5), (1, 1), (2, 2), (1, 1), 'ls2', 2, 1),
    'c320_stride2_2x2': (2, 320, 64, 10, 13, (3, 3), (2, 2), (1, 1), (1, 1), 'ls2', 2, 2),
    'gf3_gf3': (2, 128, 32, 8, 8, (3, 3), (1, 1), (1, 1), (1, 1), 'gf', 3, 3),
    'planes_8x8': (1, 64, 32, 5, 5, (3, 3), (1, 1), (1, 1), (1, 1), 'gf', 8, 8),
    '3x3_dilated_o96': (2, 128, 96, 11, 11, (3, 3), (1, 1), (2, 2), (2, 2), 'ls1', 1, 1),
    '1x7_asymmetric': (2, 64, 64, 6, 12, (1, 7), (1, 2), (0, 3), (1, 1), 'ls1', 1, 1),
}


def _hip():
    from quant import _hip
    return _hip


@functools.lru_cache(maxsize=None)
def _case(cid):
    """Operands of a case and the fp64 convolution of the quantized tensors."""
    hip = _hip()
    n, c, o, h, w, kernel, stride, pad, dil, scheme, kx, kw = CASES[cid]
    gen = torch.Generator().manual_seed(1 + list(CASES).index(cid))
    x = (1.2 * torch.randn((n, c, h, w), generator=gen)).to(DEV)
    wt = torch.randn((o, c, *kernel), generator=gen).to(DEV)
    bias = torch.randn((o,), generator=gen).to(DEV)
    geom = hip.make_geom(n, c, h, w, o, *kernel, stride, pad, dil, 1)
    planes = torch.zeros((kx * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xscales = torch.empty((kx, n), dtype=torch.float32, device=DEV)
    hip.act_quant(x, geom, {'ls1': hip.SCHEME_LS1, 'ls2': hip.SCHEME_LS2, 'gf': hip.SCHEME_GF}[scheme], kx, 1, ALPHA, planes, xscales)
    res, rows = wt.reshape(o, -1).clone(), []
    for _ in range(kw):                              # the greedy chain: v_q = mean |r_q|, r_{q+1} = r_q - v_q sign(r_q)
        rows.append(res.abs().mean(dim=1))
        res = res - rows[-1][:, None] * torch.where(res >= 0, 1.0, -1.0)
    wscales = torch.stack(rows).contiguous()
    wbits, wsum = hip.pack_weight(wt, geom, wscales)
    x_q = hip.quant_values(x.reshape(n, -1), xscales, ALPHA).reshape(x.shape).cpu().double()
    w_q = hip.quant_values(wt.reshape(o, -1), wscales, -1.0).reshape(wt.shape).cpu().double()
    y64 = F.conv2d(x_q, w_q, bias.cpu().double(), stride, pad, dil)
    return (planes, kx, xscales, wbits, wsum, wscales, bias, geom), y64


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('cid', list(CASES))
def test_equals_xnor_conv2d_half_and_the_fp64_convolution(cid, dt):
    hip, dtype = _hip(), DTYPES[dt]
    args, y64 = _case(cid)
    assert hip.xnor_conv2d_gen_half_supported(args[-1], args[1], args[5].shape[0], dtype)
    want = hip.xnor_conv2d_half(*args, dtype)
    y = hip.xnor_conv2d_gen_half(*args, dtype)
    assert y is not None and y.dtype == dtype
    top = float(y64.abs().max())
    excess = float(((y.cpu().double() - y64).abs() - torch.finfo(dtype).eps / 2 * y64.abs() - 1e-4 * top).max())
    print(f'CONV-XNOR-GEN-HALF {cid} {dt} max|y64|={top:.4g} excess={excess:.3e} differ={int((y != want).sum())} of {y.numel()}')
    assert top < 6e4
    assert torch.equal(y, want), (cid, dt)
    assert excess <= 0, (cid, dt, excess)


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('cid', ['5x5', 'c320_stride2_2x2'])
@pytest.mark.parametrize('epilogue', ['pre_prelu_post', 'relu_post'])
def test_fused_epilogue(epilogue, cid, dt):
    hip, dtype = _hip(), DTYPES[dt]
    args, _ = _case(cid)
    plain = hip.xnor_conv2d_half(*args, dtype)
    gen = torch.Generator().manual_seed(77)
    pre, post = (torch.randn(plain.shape, generator=gen).to(DEV, dtype) for _ in range(2))
    slope = (0.25 + 0.5 * torch.rand((plain.shape[1],), generator=gen)).to(DEV)
    epi = dict(res_pre=pre, prelu=slope, res_post=post) if epilogue == 'pre_prelu_post' else dict(relu=True, res_post=post)
    want = hip.xnor_conv2d_half(*args, dtype, **epi)
    y = hip.xnor_conv2d_gen_half(*args, dtype, **epi)
    assert y is not None and torch.equal(y, want) and not torch.equal(want, plain)


@pytest.mark.parametrize('change', [dict(groups=2), dict(c=96), dict(o=48), dict(dtype=0)], ids=['groups2', 'C96', 'O48', 'fp32'])
def test_refusals_launch_nothing(change):
    hip = _hip()
    n, c, o, groups = 2, change.get('c', 128), change.get('o', 64), change.get('groups', 1)
    code = change.get('dtype', hip.LINEAR_HALF_DTYPES[torch.bfloat16])
    geom = hip.make_geom(n, c, 8, 8, o, 3, 3, (1, 1), (1, 1), (1, 1), groups)
    x = torch.randn((n, c, 8, 8), generator=torch.Generator().manual_seed(5)).to(DEV)
    wt = torch.randn((o, c // groups, 3, 3), generator=torch.Generator().manual_seed(6)).to(DEV)
    planes = torch.zeros((hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xscales = torch.empty((1, n), dtype=torch.float32, device=DEV)
    hip.act_quant(x, geom, hip.SCHEME_LS1, 1, 1, ALPHA, planes, xscales)
    wscales = wt.reshape(o, -1).abs().mean(dim=1)[None].contiguous()
    wbits, wsum = hip.pack_weight(wt, geom, wscales)
    y = torch.full((n, o, 8, 8), 12345.0, dtype=torch.float32, device=DEV)      # (room for either element size)
    lib = hip.conv_xnor_gen_half_lib()
    assert lib.lsq_xnor_conv2d_gen_half_supported(ctypes.byref(geom), 1, 1, code) == 0
    assert lib.lsq_xnor_conv2d_gen_half(planes.data_ptr(), 1, xscales.data_ptr(), wbits.data_ptr(), wsum.data_ptr(), 1,
                                        wscales.data_ptr(), None, ctypes.byref(geom), 0, None, None, None, code, y.data_ptr(),
                                        hip.stream_ptr(y.device)) == hip.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == 12345.0).all())


def test_module_switch_takes_the_general_kernel():
    hip = _hip()
    from quant.binary.binary_conv import QuantConv2d
    conv = QuantConv2d('ls-2', 'ls-1', 192, 64, 1, {'kind': 'symmetric', 'alpha': 3}, bias=True)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=torch.Generator().manual_seed(9)))
        conv.w_approximate.v1.copy_(conv.weight.abs().mean(dim=(1, 2, 3)))
    conv.eval().to(DEV)
    x = (1.2 * torch.randn((2, 192, 9, 9), generator=torch.Generator().manual_seed(10))).to(DEV, torch.bfloat16)
    assert QuantConv2d.xnor_general_half is False
    before = QuantConv2d.act_half, QuantConv2d.xnor_half
    outs, calls = {}, {}
    try:
        QuantConv2d.act_half, QuantConv2d.xnor_half = True, True
        for on in (False, True):
            QuantConv2d.xnor_general_half = on
            hip.enable_timing(True)
            with torch.no_grad():
                outs[on] = conv(x)
            torch.cuda.synchronize()
            calls[on] = {k: v[0] for k, v in hip.drain_timing().items()}
    finally:
        QuantConv2d.act_half, QuantConv2d.xnor_half = before
        QuantConv2d.xnor_general_half = False
        hip.enable_timing(False)
    assert outs[True].dtype == torch.bfloat16 and torch.equal(outs[True], outs[False]) and float(outs[False].abs().max()) > 0
    assert calls[False].get('lsq_xnor_conv2d_half') == 1 and 'lsq_xnor_conv2d_gen_half' not in calls[False]
    assert calls[True].get('lsq_xnor_conv2d_gen_half') == 1 and 'lsq_xnor_conv2d_half' not in calls[True]
