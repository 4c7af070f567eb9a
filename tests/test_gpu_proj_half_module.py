"""``quant.models.resnet.PROJ_HALF`` on the GPU: the projection shortcut of a 16-bit down-sampling ``XnorBasicBlock``.

An eval-mode ``XnorBasicBlock(64 -> 128, stride 2, ls-2)`` with ``act_half`` and ``xnor_half`` set, input 3 x 64 x 12 x 12 in bf16
and fp16, clamp bound 2.0 (a value of both types).  The wrappers are counted, and the block's output is held -- torch.equal on
the raw 16-bit patterns -- to the fp32 entry points composed on the block's own 16-bit intermediate:
  * switch off: neither new wrapper is called;
  * switch on, FUSE_PROJECTION: ONE lsq_xnor_conv2d_proj_half, no pointwise call; output == lsq_xnor_conv2d_proj on the widened
    operands, .to(dtype) -- the shortcut is never rounded on its own;
  * switch on, no fusion: ONE lsq_pointwise_conv_half; output == lsq_xnor_conv2d with lsq_pointwise_conv(x.float()).to(dtype)
    as the residual, .to(dtype) -- the shortcut rounded first;
  * an identity block (stride 1, 64 -> 64) is unaffected."""

import pytest
import torch

import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
CLAMP = {'kind': 'symmetric', 'alpha': 2}
COUNTED = ('pointwise_conv', 'pointwise_conv_half', 'xnor_conv2d_proj', 'xnor_conv2d_proj_half', 'xnor_conv2d_half', 'xnor_conv2d')


def _hip():
    from quant import _hip
    return _hip


def _bits(y):
    assert y.dtype in (torch.bfloat16, torch.float16)
    return y.contiguous().view(torch.int16)


def _block(cin, cout, stride, seed):
    from quant.models import resnet
    block = resnet.XnorBasicBlock(cin, cout, 'ls-2', 'ls-1', ['relu', 'relu'], stride=stride, clamp=CLAMP)
    detgen.fill_module(block, seed=seed)
    with torch.no_grad():
        for conv in (block.conv1, block.conv2):
            for buf, v in zip(conv.w_approximate.cached_scales(), P.weight_scales(conv.weight, 'ls-1')):
                buf.copy_(v)
    return block.eval().to(DEV)


@pytest.fixture
def switches(monkeypatch):
    """act_half and xnor_half on for every QuantConv2d, the gate open for (64, 128), and the wrappers counted."""
    from quant.binary.binary_conv import QuantConv2d
    hip = _hip()
    monkeypatch.setattr(QuantConv2d, 'act_half', True)
    monkeypatch.setattr(QuantConv2d, 'xnor_half', True)
    monkeypatch.setattr(hip, 'PROJ_FUSED_SHAPES', frozenset({(64, 128)}))
    calls = {name: 0 for name in COUNTED}

    def counted(name, real):
        def f(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return f

    for name in COUNTED:
        monkeypatch.setattr(hip, name, counted(name, getattr(hip, name)))
    return calls


def _took(calls, before):
    return {k: calls[k] - before[k] for k in calls if calls[k] != before[k]}


def _conv2_operands(block, x):
    """What conv2's launch reads, from the block's own 16-bit intermediate: the planes and scales of lsq_act_quant on
    bn2(first).float() (the bits lsq_act_quant_half gives), the packed weights, and the folded projection."""
    from quant.models import resnet
    hip = _hip()
    first = block.conv1.fused_forward(x, block.bn1, relu=True)
    assert first.dtype == x.dtype
    xin = block.bn2(first)
    conv = block.conv2
    geom = conv._geom_of(xin, hip)
    k = conv.x_approximate.n_planes
    planes = torch.zeros((k * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    scales = torch.empty((k, x.shape[0]), device=DEV)
    hip.act_quant(xin.float(), geom, conv.x_approximate.hip_scheme, k, conv.act_skip, conv._alpha_in(x.dtype), planes, scales)
    wbits, wsum, wscales, _ = conv._packed_weights(geom, hip)
    w, b = resnet._folded_conv_bn(block.shortcut, block.shortcut[0], block.shortcut[1])
    ho, wo = hip.out_hw(geom)
    return dict(geom=geom, k=k, planes=planes, scales=scales, wbits=wbits, wsum=wsum, wscales=wscales, bias=conv.bias.detach(),
                pw=w.view(128, 64), pb=b, yshape=(x.shape[0], 128, ho, wo))


@pytest.mark.parametrize('dt', DTYPES)
def test_switch_off_calls_neither_new_wrapper(dt, switches):
    from quant.models import resnet
    assert resnet.PROJ_HALF is False
    block = _block(64, 128, 2, seed=41)
    x = detgen.normal('projh.block.x', (3, 64, 12, 12), scale=1.0).to(DEV).to(DTYPES[dt])
    # (outside autocast the parent's 16-bit shortcut is a dtype error in torch.matmul; under an autocast of x's type it runs)
    with torch.no_grad(), torch.autocast('cuda', dtype=DTYPES[dt]):
        y = block(x)
    assert y.dtype == DTYPES[dt]
    assert switches['pointwise_conv_half'] == 0 and switches['xnor_conv2d_proj_half'] == 0


@pytest.mark.parametrize('dt', DTYPES)
def test_fused_projection_is_one_launch_rounded_once(dt, switches, monkeypatch):
    from quant.models import resnet
    hip = _hip()
    dtype = DTYPES[dt]
    block = _block(64, 128, 2, seed=41)
    x = detgen.normal('projh.block.x', (3, 64, 12, 12), scale=1.0).to(DEV).to(dtype)
    monkeypatch.setattr(resnet, 'PROJ_HALF', True)
    assert resnet.FUSE_PROJECTION is True
    before = dict(switches)
    with torch.no_grad():
        y = block(x)
    took = _took(switches, before)
    print(f'{dt} fused: calls {took}')
    assert took == {'xnor_conv2d_half': 1, 'xnor_conv2d_proj_half': 1}           # conv1, then conv2 with the projection inside
    with torch.no_grad():
        cs = _conv2_operands(block, x)
    ref = torch.full(cs['yshape'], float('nan'), device=DEV)
    assert hip.xnor_conv2d_proj(cs['planes'], cs['k'], cs['scales'], cs['wbits'], cs['wsum'], cs['wscales'], cs['bias'], cs['geom'],
                                ref, (x.float(), cs['pw'], cs['pb'], 2, False), relu=True)
    differ = int((_bits(y) != _bits(ref.to(dtype))).sum())
    print(f'{dt} fused: {differ} of {y.numel()} outputs differ from lsq_xnor_conv2d_proj on the widened operands, rounded once')
    assert y.dtype == dtype and differ == 0
    assert torch.equal(block.conv2.last_act_scales, cs['scales'])


@pytest.mark.parametrize('dt', DTYPES)
def test_unfused_projection_is_one_pointwise_half_launch(dt, switches, monkeypatch):
    from quant.models import resnet
    hip = _hip()
    dtype = DTYPES[dt]
    block = _block(64, 128, 2, seed=41)
    x = detgen.normal('projh.block.x', (3, 64, 12, 12), scale=1.0).to(DEV).to(dtype)
    monkeypatch.setattr(resnet, 'PROJ_HALF', True)
    monkeypatch.setattr(resnet, 'FUSE_PROJECTION', False)
    before = dict(switches)
    with torch.no_grad():
        y = block(x)
    took = _took(switches, before)
    print(f'{dt} unfused: calls {took}')
    assert took == {'pointwise_conv_half': 1, 'xnor_conv2d_half': 2}
    with torch.no_grad():
        cs = _conv2_operands(block, x)
    before = dict(switches)
    sc = hip.pointwise_conv(x.float(), cs['pw'], cs['pb'], 2).to(dtype)              # the shortcut, rounded on its own
    ref = torch.full(cs['yshape'], float('nan'), device=DEV)
    hip.xnor_conv2d(cs['planes'], cs['k'], cs['scales'], cs['wbits'], cs['wsum'], cs['wscales'], cs['bias'], cs['geom'], ref,
                    relu=True, res_pre=sc.float())
    differ = int((_bits(y) != _bits(ref.to(dtype))).sum())
    print(f'{dt} unfused: {differ} of {y.numel()} outputs differ from the fp32 composition with the 16-bit shortcut')
    assert y.dtype == dtype and differ == 0
    # the _ConvBN shortcut on its own: the same tensor
    with torch.no_grad():
        assert torch.equal(_bits(block.shortcut(x)), _bits(sc))


@pytest.mark.parametrize('dt', DTYPES)
def test_identity_block_is_unaffected(dt, switches, monkeypatch):
    from quant.models import resnet
    block = _block(64, 64, 1, seed=43)
    x = detgen.normal('projh.ident.x', (3, 64, 12, 12), scale=1.0).to(DEV).to(DTYPES[dt])
    with torch.no_grad():
        off = block(x)
        monkeypatch.setattr(resnet, 'PROJ_HALF', True)
        on = block(x)
    assert switches['pointwise_conv_half'] == 0 and switches['xnor_conv2d_proj_half'] == 0
    assert torch.equal(_bits(on), _bits(off))
