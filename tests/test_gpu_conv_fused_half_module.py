"""``QuantConv2d.fp_half_fused`` / ``fp_half_bn_fold`` on the GPU: ``fused_forward`` of a 16-bit input with ``fp`` activations.

Off: today's composition, no call of the new binding.  ``fp_half_fused``: exactly one lsq_signw_conv2d_fused_half, the result
of the fp32 composition around the EXISTING lsq_signw_conv2d_half with torch's batch norm in front, rounded once.  With
``fp_half_bn_fold``: the batch norm's forward is never reached and the result is that composition on the folded tensor.
Operands that do not fit fall back to the composition, bit for bit; a whole ``XnorBasicBlock('fp', 'ls-1', PReLU)`` equals the
block assembled by hand from the binding's calls."""

import pytest
import torch

import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
CLAMPS = ({'kind': 'identity'}, {'kind': 'symmetric', 'alpha': 2}, {'kind': 'symmetric', 'alpha': 1.3})
# (in channels, out channels, kernel, padding, stride, H = W, N): LAYERS of tests/test_gpu_conv_half.py, restated
LAYERS = ((64, 70, 3, 1, 1, 9, 5), (64, 70, 3, 1, 2, 9, 5), (65, 40, 1, 0, 1, 7, 5))
COUNTED = ('signw_conv2d_fused_half', 'signw_conv2d_half', 'signw_conv2d', 'pointwise_conv_half')


def _hip():
    from quant import _hip
    return _hip


def _bits(y):
    assert y.dtype in (torch.bfloat16, torch.float16)
    return y.contiguous().view(torch.int16)


def _module(ws, layer, clamp, seed):
    from quant.binary.binary_conv import QuantConv2d
    cin, cout, ksz, pad, stride = layer[:5]
    m = QuantConv2d('fp', ws, cin, cout, ksz, clamp, bias=True, padding=pad, stride=stride)
    detgen.fill_module(m, seed=seed)
    with torch.no_grad():
        for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight, ws)):
            buf.copy_(v)
    m = m.eval().to(DEV)
    m.fp_half = True
    return m


def _bn(ch, tag):
    bn = torch.nn.BatchNorm2d(ch).eval().to(DEV)
    with torch.no_grad():
        bn.running_mean.copy_(detgen.normal(f'qfused.bn.m.{tag}', (ch,), scale=0.2))
        bn.running_var.copy_(detgen.uniform(f'qfused.bn.v.{tag}', (ch,), 0.5, 1.5))
        bn.weight.copy_(detgen.uniform(f'qfused.bn.w.{tag}', (ch,), 0.5, 1.5))
        bn.bias.copy_(detgen.normal(f'qfused.bn.b.{tag}', (ch,), scale=0.3))
    return bn


def _input(tag, layer, dtype):
    cin, _, _, _, _, hw, n = layer
    return detgen.normal(f'qfused.x.{tag}', (n, cin, hw, hw), scale=1.3).to(DEV).to(dtype)


def _residual(tag, m, x, dtype):
    hip = _hip()
    ho, wo = hip.out_hw(m._geom_of(x, hip))
    return detgen.normal(f'qfused.res.{tag}', (x.shape[0], m.out_channels, ho, wo), scale=1.0).to(DEV).to(dtype)


@pytest.fixture
def calls(monkeypatch):
    hip = _hip()
    n = {name: 0 for name in COUNTED}

    def counted(name, real):
        def f(*a, **k):
            n[name] += 1
            return real(*a, **k)
        return f

    for name in COUNTED:
        monkeypatch.setattr(hip, name, counted(name, getattr(hip, name)))
    return n


def _took(calls, before):
    return {k: calls[k] - before[k] for k in calls if calls[k] != before[k]}


def _by_hand(m, t, relu=False, prelu=None, res_pre=None, res_post=None):
    """The contract's composition on the 16-bit tensor ``t`` the convolution reads: the existing kernel with an fp32 y, the
    epilogue in fp32, one rounding."""
    hip = _hip()
    geom = m._geom_of(t, hip)
    wbits, _, wscales, _ = m._packed_weights(geom, hip, prep=False)
    v = hip.signw_conv2d_half(t.contiguous(), m._alpha_in(t.dtype), wbits, wscales, m.bias.detach(), geom, out_dtype=torch.float32)
    if res_pre is not None:
        v = v + res_pre.float()
    if relu:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    if prelu is not None:
        sl = prelu.detach().float()
        v = torch.where(v > 0, v, (sl.view(1, -1, 1, 1) if sl.numel() > 1 else sl) * v)
    if res_post is not None:
        v = v + res_post.float()
    return v.to(t.dtype)


def _folded(m, bn, x):
    s, b = m._folded_bn(bn)
    return (x.float() * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)).to(x.dtype)


def _variant(li, m, x, dtype, relu_only=False):
    """(keyword arguments of fused_forward) of layer ``li``: ReLU + res_pre, one-slope PReLU + res_post, per-channel + both.
    ``relu_only``: ReLU in place of the PReLUs (torch's own F.prelu takes no fp32 slopes on a 16-bit tensor)."""
    if relu_only and li == 1:
        return dict(relu=True, res_post=_residual('b', m, x, dtype))
    if relu_only and li == 2:
        return dict(relu=True, res_pre=_residual('c', m, x, dtype), res_post=_residual('d', m, x, dtype))
    if li == 0:
        return dict(relu=True, res_pre=_residual('a', m, x, dtype))
    if li == 1:
        return dict(prelu=torch.tensor([0.25], device=DEV), res_post=_residual('b', m, x, dtype))
    slopes = detgen.uniform('qfused.slopes', (m.out_channels,), -0.5, 0.5).to(DEV)
    return dict(prelu=slopes, res_pre=_residual('c', m, x, dtype), res_post=_residual('d', m, x, dtype))


@pytest.mark.parametrize('li', range(len(LAYERS)))
@pytest.mark.parametrize('dt', DTYPES)
def test_default_is_todays_composition(dt, li, calls):
    dtype = DTYPES[dt]
    m = _module('ls-1', LAYERS[li], CLAMPS[1], seed=71 + li)
    bn = _bn(LAYERS[li][0], li)
    x = _input(li, LAYERS[li], dtype)
    kw = _variant(li, m, x, dtype, relu_only=True)
    with torch.no_grad():
        y = m.fused_forward(x, pre_bn=bn, **kw)
        ref = m(bn(x))
        if 'res_pre' in kw:
            ref = ref + kw['res_pre']
        ref = torch.relu(ref)
        if 'res_post' in kw:
            ref = ref + kw['res_post']
    print(f'default {dt} layer {li}: calls {calls}')
    assert calls['signw_conv2d_fused_half'] == 0 and calls['signw_conv2d_half'] == 2
    assert torch.equal(_bits(y), _bits(ref))


@pytest.mark.parametrize('li', range(len(LAYERS)))
@pytest.mark.parametrize('ws', ('ls-1', 'ls-2'))
@pytest.mark.parametrize('dt', DTYPES)
def test_fp_half_fused_is_one_launch_rounded_once(dt, ws, li, calls):
    dtype = DTYPES[dt]
    m = _module(ws, LAYERS[li], CLAMPS[(li + 1) % 3], seed=81 + li)
    m.fp_half_fused = True
    bn = _bn(LAYERS[li][0], li)
    x = _input(li, LAYERS[li], dtype)
    kw = _variant(li, m, x, dtype)
    with torch.no_grad():
        y = m.fused_forward(x, pre_bn=bn, **kw)
        took = dict(calls)
        ref = _by_hand(m, bn(x), **kw)
        with torch.autocast('cuda', dtype=dtype):
            ya = m.fused_forward(x, pre_bn=bn, **kw)
        plain = m.fused_forward(x, **kw)                      # no batch norm at all
        ref_plain = _by_hand(m, x, **kw)
    print(f'fused {dt} {ws} layer {li}: calls {took}; {int((_bits(y) != _bits(ref)).sum())} outputs differ from the composition')
    assert took['signw_conv2d_fused_half'] == 1 and took['signw_conv2d_half'] == 0 and took['signw_conv2d'] == 0
    assert y.dtype == dtype and torch.equal(y, ref)
    assert torch.equal(_bits(ya), _bits(y))
    assert torch.equal(plain, ref_plain)


@pytest.mark.parametrize('li', range(len(LAYERS)))
@pytest.mark.parametrize('dt', DTYPES)
def test_bn_fold_never_runs_the_batch_norm(dt, li, calls, monkeypatch):
    dtype = DTYPES[dt]
    m = _module('ls-2', LAYERS[li], CLAMPS[(li + 1) % 3], seed=91 + li)
    m.fp_half_fused = True
    bn = _bn(LAYERS[li][0], li)
    x = _input(li, LAYERS[li], dtype)
    kw = _variant(li, m, x, dtype)
    with torch.no_grad():
        unfolded = m.fused_forward(x, pre_bn=bn, **kw)
        m.fp_half_bn_fold = True
        before = dict(calls)

        def boom(*a, **k):
            raise AssertionError('the batch norm ran in torch')

        monkeypatch.setattr(bn, 'forward', boom)
        y = m.fused_forward(x, pre_bn=bn, **kw)
        took = _took(calls, before)
        ref = _by_hand(m, _folded(m, bn, x), **kw)
    differ = int((_bits(y) != _bits(unfolded)).sum())
    print(f'fold {dt} layer {li}: calls {took}; {differ} of {y.numel()} outputs differ from the unfolded route (printed, not asserted)')
    assert took == {'signw_conv2d_fused_half': 1}
    assert y.dtype == dtype and torch.equal(y, ref)


@pytest.mark.parametrize('dt', DTYPES)
def test_fallbacks_take_the_composition(dt, calls):
    """An fp32 residual, a residual of another shape (broadcast), a train-mode batch norm: the bits of the switches off."""
    dtype = DTYPES[dt]
    layer = LAYERS[0]
    m = _module('ls-1', layer, CLAMPS[1], seed=101)
    bn = _bn(64, 'fb')
    x = _input('fb', layer, dtype)
    res = _residual('fb', m, x, dtype)
    cases = [dict(pre_bn=bn, relu=True, res_pre=res.float()), dict(pre_bn=bn, relu=True, res_post=res[:, :, :1, :1].contiguous())]
    with torch.no_grad():
        for kw in cases:
            off = m.fused_forward(x, **kw)
            m.fp_half_fused = m.fp_half_bn_fold = True
            before = dict(calls)
            on = m.fused_forward(x, **kw)
            took = _took(calls, before)
            m.fp_half_fused = m.fp_half_bn_fold = False
            print(f'fallback {dt} {sorted(kw)}: calls {took}')
            assert took == {'signw_conv2d_half': 1}
            assert on.dtype == off.dtype and torch.equal(on, off)
        # a train-mode batch norm keeps the composition (its statistics put back between the two calls: the same batch norm)
        bn.train()
        state = {k: v.clone() for k, v in bn.state_dict().items()}
        kw = dict(pre_bn=bn, relu=True, res_pre=res)
        off = m.fused_forward(x, **kw)
        bn.load_state_dict(state)
        m.fp_half_fused = m.fp_half_bn_fold = True
        assert not m._fuses_fp_half(x, bn) and not m._folds_fp_half_bn(x, bn)
        before = dict(calls)
        on = m.fused_forward(x, **kw)
        took = _took(calls, before)
        print(f'fallback {dt} train-mode batch norm: calls {took}')
        assert took == {'signw_conv2d_half': 1}
        assert on.dtype == off.dtype and torch.equal(_bits(on), _bits(off))


# ------------------------------------------------------------------------------------------------ a whole block
def _block(cin, cout, stride, double_shortcut, seed):
    from quant.models import resnet
    block = resnet.XnorBasicBlock(cin, cout, 'fp', 'ls-1', ['prelu', 'prelu'], stride=stride, double_shortcut=double_shortcut,
                                  clamp=CLAMPS[1])
    detgen.fill_module(block, seed=seed)
    with torch.no_grad():
        for conv in (block.conv1, block.conv2):
            for buf, v in zip(conv.w_approximate.cached_scales(), P.weight_scales(conv.weight, 'ls-1')):
                buf.copy_(v)
    return block.eval().to(DEV)


@pytest.fixture
def block_switches(monkeypatch):
    from quant.binary.binary_conv import QuantConv2d
    monkeypatch.setattr(QuantConv2d, 'fp_half', True)
    monkeypatch.setattr(QuantConv2d, 'fp_half_fused', True)


def _block_by_hand(block, x, sc):
    c1, c2 = block.conv1, block.conv2
    p1, p2 = block.nonlin1.weight, block.nonlin2.weight
    if block.double_shortcut:
        first = _by_hand(c1, block.bn1(x), prelu=p1, res_post=sc)
        return _by_hand(c2, block.bn2(first), prelu=p2, res_post=first)
    first = _by_hand(c1, block.bn1(x), prelu=p1)
    return _by_hand(c2, block.bn2(first), prelu=p2, res_pre=sc)


@pytest.mark.parametrize('double_shortcut', (False, True), ids=('single', 'double'))
@pytest.mark.parametrize('dt', DTYPES)
def test_identity_block(dt, double_shortcut, block_switches, calls):
    dtype = DTYPES[dt]
    block = _block(64, 64, 1, double_shortcut, seed=111)
    x = detgen.normal('qfused.block.x', (2, 64, 9, 9), scale=1.0).to(DEV).to(dtype)
    with torch.no_grad():
        y = block(x)
        took = dict(calls)
        ref = _block_by_hand(block, x, x)
    print(f'block {dt} double={double_shortcut}: calls {took}; {int((_bits(y) != _bits(ref)).sum())} outputs differ')
    assert took['signw_conv2d_fused_half'] == 2 and took['signw_conv2d_half'] == 0
    assert y.dtype == dtype and torch.equal(y, ref)


@pytest.mark.parametrize('proj_half', (False, True), ids=('proj_torch', 'proj_half'))
@pytest.mark.parametrize('dt', DTYPES)
def test_downsampling_block(dt, proj_half, block_switches, calls, monkeypatch):
    from quant.models import resnet
    dtype = DTYPES[dt]
    monkeypatch.setattr(resnet, 'PROJ_HALF', proj_half)
    block = _block(64, 128, 2, False, seed=121)
    x = detgen.normal('qfused.block.x2', (2, 64, 9, 9), scale=1.0).to(DEV).to(dtype)
    # (outside autocast the 16-bit shortcut on torch is a dtype error in torch.matmul; under an autocast of x's type it runs)
    with torch.no_grad(), torch.autocast('cuda', dtype=dtype, enabled=not proj_half):
        y = block(x)
        took = dict(calls)
        sc = block.shortcut(x)
        assert sc.dtype == dtype
        ref = _block_by_hand(block, x, sc)
    print(f'block 64->128 {dt} PROJ_HALF={proj_half}: calls {took}; {int((_bits(y) != _bits(ref)).sum())} outputs differ')
    assert took['signw_conv2d_fused_half'] == 2 and took['signw_conv2d_half'] == 0
    assert took['pointwise_conv_half'] == (1 if proj_half else 0)
    assert y.dtype == dtype and torch.equal(y, ref)
