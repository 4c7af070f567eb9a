"""lsq_xnor_conv2d_narrow (include/lsq_hip_conv_xnor_narrow.h, csrc/conv_xnor_narrow): the fp4 matrix-core XNOR convolution for
any channel count, with and without its 2 x 2 pool, against lsq_xnor_conv2d on the same operands (equal, bit for bit; followed
by F.max_pool2d for pool 2) and against F.conv2d in fp64 of the quantized tensors (1e-4 of max |y|, README "Outputs"), at the
smallest geometries that reach each of the kernel's paths; the fused epilogue, the refusals and ``QuantConv2d.xnor_narrow``
under ``QLeNet5``."""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ALPHA = 3.0
SENT = 12345.0

# id: (N, C, O, H, W, (KH, KW), stride, pad, dilation, activation scheme, activation planes, weight planes)
CASES = {
    'lenet_conv2': (5, 20, 50, 12, 12, (5, 5), (1, 1), (0, 0), (1, 1), 'ls2', 2, 1),
    'c96_3x3': (2, 96, 96, 6, 6, (3, 3), (1, 1), (1, 1), (1, 1), 'ls1', 1, 1),
    'c16_stride2': (3, 16, 16, 9, 9, (3, 3), (2, 2), (1, 1), (1, 1), 'ls2', 2, 2),
    'c160_1x1': (2, 160, 40, 7, 7, (1, 1), (1, 1), (0, 0), (1, 1), 'ls1', 1, 1),
    'c33_dilated': (2, 33, 64, 9, 9, (3, 3), (1, 1), (2, 2), (2, 2), 'gf', 3, 2),
    'c48_1x7': (2, 48, 24, 6, 12, (1, 7), (1, 2), (0, 3), (1, 1), 'ls1', 1, 1),
    'c448_63_steps': (1, 448, 40, 5, 5, (3, 3), (1, 1), (1, 1), (1, 1), 'ls1', 1, 1),      # 65.6 KB of LDS: past the plain 64 KB
}


def _hip():
    from quant import _hip
    return _hip


@functools.lru_cache(maxsize=None)
def _case(cid, groups=1):
    """Operands of a case, the output of lsq_xnor_conv2d on them and the fp64 convolution of the quantized tensors."""
    hip = _hip()
    n, c, o, h, w, kernel, stride, pad, dil, scheme, kx, kw = CASES[cid]
    gen = torch.Generator().manual_seed(1 + list(CASES).index(cid))
    x = (1.2 * torch.randn((n, c, h, w), generator=gen)).to(DEV)
    wt = torch.randn((o, c // groups, *kernel), generator=gen).to(DEV)
    bias = torch.randn((o,), generator=gen).to(DEV)
    geom = hip.make_geom(n, c, h, w, o, *kernel, stride, pad, dil, groups)
    planes = torch.zeros((kx * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xscales = torch.empty((kx, n), dtype=torch.float32, device=DEV)
    hip.act_quant(x, geom, {'ls1': hip.SCHEME_LS1, 'ls2': hip.SCHEME_LS2, 'gf': hip.SCHEME_GF}[scheme], kx, 1, ALPHA, planes, xscales)
    res, rows = wt.reshape(o, -1).clone(), []
    for _ in range(kw):                              # the greedy chain: v_q = mean |r_q|, r_{q+1} = r_q - v_q sign(r_q)
        rows.append(res.abs().mean(dim=1))
        res = res - rows[-1][:, None] * torch.where(res >= 0, 1.0, -1.0)
    wscales = torch.stack(rows).contiguous()
    wbits, wsum = hip.pack_weight(wt, geom, wscales)
    ho, wo = hip.out_hw(geom)
    y_ref = torch.full((n, o, ho, wo), SENT, dtype=torch.float32, device=DEV)
    hip.xnor_conv2d(planes, kx, xscales, wbits, wsum, wscales, bias, geom, y_ref)
    x_q = hip.quant_values(x.reshape(n, -1), xscales, ALPHA).reshape(x.shape).cpu().double()
    w_q = hip.quant_values(wt.reshape(o, -1), wscales, -1.0).reshape(wt.shape).cpu().double()
    y64 = F.conv2d(x_q, w_q, bias.cpu().double(), stride, pad, dil, groups)
    return (planes, kx, xscales, wbits, wsum, wscales, bias, geom), y_ref, y64


@pytest.mark.parametrize('pool', [1, 2])
@pytest.mark.parametrize('cid', list(CASES))
def test_equals_xnor_conv2d_and_the_fp64_convolution(cid, pool):
    hip = _hip()
    args, y_ref, y64 = _case(cid)
    relu = pool == 2                                 # (the pooled runs: ReLU on both sides)
    want = y_ref
    if pool == 2:
        want = torch.full_like(y_ref, SENT)
        hip.xnor_conv2d(*args, want, relu=True)
        want, y64 = F.max_pool2d(want, 2, 2), F.max_pool2d(y64.relu(), 2, 2)
    assert hip.xnor_conv2d_narrow_supported(args[-1], args[1], args[5].shape[0], pool)
    y = torch.full_like(want, SENT)
    assert hip.xnor_conv2d_narrow(*args, y, relu=relu, pool=pool)
    err = float((y.cpu().double() - y64).abs().max() / y64.abs().max())
    print(f'CONV-XNOR-NARROW {cid} pool={pool} rel_err={err:.3e} differ={int((y != want).sum())} of {y.numel()}')
    assert torch.equal(y, want), (cid, pool)
    assert err <= 1e-4, (cid, pool, err)


@pytest.mark.parametrize('epilogue', ['pre_prelu_post', 'relu_post'])
def test_fused_epilogue(epilogue):
    hip = _hip()
    args, y_ref, _ = _case('c96_3x3')
    gen = torch.Generator().manual_seed(77)
    pre, post = (torch.randn(y_ref.shape, generator=gen).to(DEV) for _ in range(2))
    slope = (0.25 + 0.5 * torch.rand((y_ref.shape[1],), generator=gen)).to(DEV)
    epi = dict(res_pre=pre, prelu=slope, res_post=post) if epilogue == 'pre_prelu_post' else dict(relu=True, res_post=post)
    want, y = torch.full_like(y_ref, SENT), torch.full_like(y_ref, SENT)
    hip.xnor_conv2d(*args, want, **epi)
    assert hip.xnor_conv2d_narrow(*args, y, **epi)
    assert torch.equal(y, want) and not torch.equal(want, y_ref)


@pytest.mark.parametrize('what', ['groups2', 'fragments', 'pool3', 'pool2_res_post'])
def test_refusals_launch_nothing(what):
    hip = _hip()
    pool, post = {'pool3': 3, 'pool2_res_post': 2}.get(what, 1), what == 'pool2_res_post'
    if what == 'fragments':                          # 49 taps x 3 dwords of 96 channels > 128: operands are never read
        geom = hip.make_geom(2, 96, 8, 8, 96, 7, 7, (1, 1), (3, 3), (1, 1), 1)
        words = hip.lib().lsq_weight_plane_words(geom)
        args = (torch.zeros((hip.act_plane_words(geom),), dtype=torch.int64, device=DEV), 1, torch.ones((1, 2), device=DEV),
                torch.zeros((words,), dtype=torch.int64, device=DEV), torch.zeros((1, 96, 49), dtype=torch.int32, device=DEV),
                torch.ones((1, 96), device=DEV), None, geom)
        shape = (2, 96, 8, 8)
    else:
        args, y_ref, _ = _case('c96_3x3', 2 if what == 'groups2' else 1)
        shape = y_ref.shape
    geom, kx, kw = args[-1], args[1], args[5].shape[0]
    y = torch.full(shape if pool != 2 else (*shape[:2], shape[2] // 2, shape[3] // 2), SENT, dtype=torch.float32, device=DEV)
    res_post = torch.zeros(shape, device=DEV) if post else None
    assert post or not hip.xnor_conv2d_narrow_supported(geom, kx, kw, pool)
    assert not hip.xnor_conv2d_narrow(*args, y, res_post=res_post, pool=pool)
    torch.cuda.synchronize()
    assert bool((y == SENT).all())


def test_lenet_pools_inside_the_narrow_call(monkeypatch):
    hip = _hip()
    from quant.binary.binary_conv import QuantConv2d
    from quant.models.lenet import QLeNet5
    torch.manual_seed(3)
    net = QLeNet5(loss_fn=None, x_quant='ls-2', w_quant='ls-1', clamp={'kind': 'symmetric', 'alpha': ALPHA})
    with torch.no_grad():
        net.conv2.w_approximate.v1.copy_(net.conv2.weight.abs().mean(dim=(1, 2, 3)))
    net.eval().to(DEV)
    x = torch.randn((3, 1, 28, 28), generator=torch.Generator().manual_seed(4)).to(DEV)
    pools, real = [], hip.xnor_conv2d_narrow

    def counted(*args, **kwargs):
        pools.append(kwargs.get('pool', args[13] if len(args) > 13 else 1))
        return real(*args, **kwargs)

    monkeypatch.setattr(hip, 'xnor_conv2d_narrow', counted)
    assert QuantConv2d.xnor_narrow is False
    outs = {}
    try:
        for on in (False, True):
            QuantConv2d.xnor_narrow = on
            with torch.no_grad():
                outs[on] = net(x)
    finally:
        QuantConv2d.xnor_narrow = False
    assert pools == [2]
    assert torch.equal(outs[True], outs[False]) and bool(torch.isfinite(outs[False]).all())
