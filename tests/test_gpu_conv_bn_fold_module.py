"""QuantConv2d.fused_forward with ``act_half_bn_fold`` on the GPU: with the switch on, an eval-mode batch norm in front of a
16-bit layer is not run in torch but folded into the quantizer's read (lsq_act_quant_bn_half), and the result is bit for
bit the layer on ``folded(x, *conv._folded_bn(bn))`` -- with ``xnor_half`` (one quantizer launch, one lsq_xnor_conv2d_half
launch) and without it (the composition in torch); with the switch off, and for every input the fold does not cover, the
route is the one it was and the new kernel is never called."""

import pytest
import torch

import conv_act_bn_half_cases as B
import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = B.DTYPES
N = 3
# (in channels, out channels, kernel, padding, stride, H = W)
LAYERS = ((64, 64, 3, 1, 1, 8), (64, 128, 3, 1, 2, 14))
XQS = ('ls-1', 'ls-2')
CLAMP = {'kind': 'symmetric', 'alpha': 2}


def _hip():
    from quant import _hip
    return _hip


def _module(xq, layer, seed, **attrs):
    from quant.binary.binary_conv import QuantConv2d
    cin, cout, ksz, pad, stride, _ = layer
    m = QuantConv2d(xq, 'ls-1', cin, cout, ksz, CLAMP, padding=pad, stride=stride, bias=True)
    detgen.fill_module(m, seed=seed)
    with torch.no_grad():
        for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight, 'ls-1')):
            buf.copy_(v)
    m.__dict__.update(attrs)
    return m.eval().to(DEV)


def _bn(c, seed):
    bn = torch.nn.BatchNorm2d(c)
    detgen.fill_module(bn, seed=seed)              # affine parameters and running statistics
    return bn.eval().to(DEV)


def _operands(layer, dtype, tag):
    cin, cout, ksz, pad, stride, hw = layer
    ho = (hw + 2 * pad - ksz) // stride + 1
    x = detgen.normal(f'bnfold.x.{tag}', (N, cin, hw, hw), scale=1.3).to(DEV).to(dtype)
    res = detgen.normal(f'bnfold.r.{tag}', (N, cout, ho, ho), scale=1.0).to(DEV).to(dtype)
    return x, res


def _bits(y):
    return y.contiguous().view(torch.int32 if y.dtype == torch.float32 else torch.int16)


@pytest.fixture
def counters(monkeypatch):
    hip = _hip()
    names = {'bn_half': 'act_quant_bn_half', 'half': 'act_quant_half', 'act': 'act_quant', 'xnor_half': 'xnor_conv2d_half',
             'xnor': 'xnor_conv2d'}
    calls = {name: 0 for name in names}
    real = {name: getattr(hip, attr) for name, attr in names.items()}     # (a missing wrapper fails here)

    def counted(name):
        def f(*a, **k):
            calls[name] += 1
            return real[name](*a, **k)
        return f

    for name, attr in names.items():
        monkeypatch.setattr(hip, attr, counted(name))
    return calls


def _count_forwards(bn):
    seen = [0]
    bn.register_forward_pre_hook(lambda *a: seen.__setitem__(0, seen[0] + 1))
    return seen


@pytest.mark.parametrize('li', range(len(LAYERS)))
@pytest.mark.parametrize('xq', XQS)
@pytest.mark.parametrize('dt', DTYPES)
def test_switch_off_is_the_route_it_was(dt, xq, li, counters):
    """The default: torch's batch norm in front, lsq_act_quant_bn_half never called, the output bit-equal to the layer on
    bn(x) -- with and without xnor_half."""
    layer, dtype = LAYERS[li], DTYPES[dt]
    from quant.binary.binary_conv import QuantConv2d
    assert QuantConv2d.act_half_bn_fold is False
    x, res = _operands(layer, dtype, f'off.{li}')
    bn = _bn(layer[0], seed=5 + li)
    for xnor_half in (True, False):
        m = _module(xq, layer, seed=31 + li, act_half=True, xnor_half=xnor_half)
        seen = _count_forwards(bn)
        with torch.no_grad():
            y = m.fused_forward(x, pre_bn=bn, relu=True, res_pre=res)
            assert seen[0] == 1
            ref = m.fused_forward(bn(x), pre_bn=None, relu=True, res_pre=res)
        differ = (_bits(y) != _bits(ref)).sum().item()
        print(f'off {xq} {dt} layer {layer} xnor_half={xnor_half}: {differ} outputs differ; calls {counters}')
        assert differ == 0 and y.dtype == dtype
        assert counters['bn_half'] == 0 and counters['half'] > 0


@pytest.mark.parametrize('xnor_half', (True, False))
@pytest.mark.parametrize('li', range(len(LAYERS)))
@pytest.mark.parametrize('xq', XQS)
@pytest.mark.parametrize('dt', DTYPES)
def test_switch_on_folds_the_batch_norm(dt, xq, li, xnor_half, counters):
    """fused_forward(x, pre_bn=bn, relu, res_pre) is bit for bit fused_forward(folded(x, *conv._folded_bn(bn)), None, relu,
    res_pre); bn's forward is not called; last_act_scales is equal too.  With xnor_half: one lsq_act_quant_bn_half and one
    lsq_xnor_conv2d_half launch; without: the composition branch around lsq_act_quant_bn_half + lsq_xnor_conv2d."""
    layer, dtype = LAYERS[li], DTYPES[dt]
    x, res = _operands(layer, dtype, f'on.{li}')
    bn = _bn(layer[0], seed=7 + li)
    m = _module(xq, layer, seed=41 + li, act_half=True, xnor_half=xnor_half, act_half_bn_fold=True)
    seen = _count_forwards(bn)
    with torch.no_grad():
        y = m.fused_forward(x, pre_bn=bn, relu=True, res_pre=res)
        scales = m.last_act_scales.clone()
        assert seen[0] == 0
        assert (counters['bn_half'], counters['half'], counters['act']) == (1, 0, 0)
        assert (counters['xnor_half'], counters['xnor']) == ((1, 0) if xnor_half else (0, 1))
        t = B.folded(x, *m._folded_bn(bn))
        ref = m.fused_forward(t, pre_bn=None, relu=True, res_pre=res)
        ref_scales = m.last_act_scales.clone()
    assert (counters['bn_half'], counters['half']) == (1, 1)
    differ = (_bits(y) != _bits(ref)).sum().item()
    differ_scales = (scales.view(torch.int32) != ref_scales.view(torch.int32)).sum().item()
    # how far torch's own batch norm is from the folded tensor, in elements (a record, not a gate)
    with torch.no_grad():
        moved = (_bits(bn(x)) != _bits(t)).float().mean().item()
    print(f'on {xq} {dt} layer {layer} xnor_half={xnor_half}: {differ} outputs, {differ_scales} scales differ from the layer on the '
          f'folded tensor; torch batch norm differs from it in {moved:.2%} of the elements')
    assert differ == 0 and differ_scales == 0 and y.dtype == dtype and seen[0] == 1


@pytest.mark.parametrize('dt', DTYPES)
def test_what_the_fold_does_not_cover_keeps_its_route(dt, counters):
    """Switch on, but: a train-mode batch norm, a batch norm without running statistics, fp activations, a CPU tensor, the
    cast comparator (act_half_kernel = False) -- torch's batch norm runs and the new kernel is never called; the result is
    the layer on bn(x)."""
    layer, dtype = LAYERS[0], DTYPES[dt]
    x, res = _operands(layer, dtype, 'keep')
    on = dict(act_half=True, xnor_half=True, act_half_bn_fold=True)

    def bn_train():
        bn = _bn(64, seed=9).train()
        bn.momentum = 0.0                          # (batch statistics; the running ones stay, so a second forward is the first)
        return bn

    def bn_no_stats():
        return torch.nn.BatchNorm2d(64, track_running_stats=False).eval().to(DEV)

    cases = [('train-mode bn', _module('ls-1', layer, 51, **on), bn_train(), x),
             ('bn without running stats', _module('ls-2', layer, 52, **on), bn_no_stats(), x),
             ('fp activations', _module('fp', layer, 53, fp_half=True, **on), _bn(64, seed=10), x),
             ('cast comparator', _module('ls-1', layer, 54, act_half_kernel=False, **on), _bn(64, seed=11), x),
             ('cpu tensor', _module('ls-1', layer, 55, **on).cpu(), _bn(64, seed=12).cpu(), x.cpu())]
    for what, m, bn, xin in cases:
        seen = _count_forwards(bn)
        r = res.to(xin.device)
        with torch.no_grad(), torch.autocast(xin.device.type, dtype=dtype, enabled=not xin.is_cuda):
            y = m.fused_forward(xin, pre_bn=bn, relu=True, res_pre=r)
            assert seen[0] == 1, what
            ref = m.fused_forward(bn(xin), pre_bn=None, relu=True, res_pre=r)
        print(f'{what} {dt}: {(_bits(y) != _bits(ref)).sum().item()} outputs differ from the layer on bn(x)')
        assert torch.equal(_bits(y), _bits(ref)), what
    assert counters['bn_half'] == 0
