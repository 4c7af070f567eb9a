"""QuantLinear on the host (no GPU): constructor and attributes as QuantConv2d's, the CPU forward against the oracle on the
4-D views, the same operands and results as a 1x1 QuantConv2d, LeNet's optional binary fc1, and the C ABI of
liblsq_hip_linear.so (header, exports, argument errors returned before any launch)."""

import itertools
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import detgen
from oracle import ref_port as P
from quant.binary import QuantLinear
from quant.binary.binary_conv import QuantConv2d
from quant.models.lenet import QLeNet5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_linear.h')
E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -6
CLAMP = {'kind': 'symmetric', 'alpha': 2}
SCHEMES = ['fp', 'ls-1', 'ls-2', 'ls-T', 'gf-2', 'gf-3']


# ------------------------------------------------------------------ constructor
def test_schemes_clamps_and_value_errors_as_quant_conv2d():
    for xs, ws in itertools.product(SCHEMES, SCHEMES):
        m = QuantLinear(xs, ws, 5, 3)
        assert m.x_quant == xs and m.w_quant == ws
        assert type(m.x_approximate) is type(QuantConv2d(xs, ws, 5, 3, 1).x_approximate)
        assert type(m.w_approximate) is type(QuantConv2d(xs, ws, 5, 3, 1).w_approximate)
    for bad in (('ls', 'ls-1'), ('l2', 'ls-1'), ('ls-1', 'ls-3'), ('ls-1', 'l2'), ('gf-', 'fp')):
        with pytest.raises(ValueError):
            QuantLinear(bad[0], bad[1], 5, 3)
        with pytest.raises(ValueError):
            QuantConv2d(bad[0], bad[1], 5, 3, 1)
    with pytest.raises(ValueError):
        QuantLinear('ls-1', 'ls-2', 5, 3, clamp={'kind': 'sym'})
    x = torch.linspace(-4, 4, 17)
    assert torch.equal(QuantLinear('ls-1', 'ls-1', 5, 3, CLAMP).clamping_fn(x), x.clamp(-2, 2))
    assert torch.equal(QuantLinear('ls-1', 'ls-1', 5, 3).clamping_fn(x), x)


@pytest.mark.parametrize('bias', (True, False))
@pytest.mark.parametrize('ws', ['ls-1', 'ls-2', 'gf-3'])
def test_quantized_parameters_and_state_dict_keys_as_quant_conv2d(ws, bias):
    lin = QuantLinear('ls-2', ws, 64, 10, CLAMP, 'eval_only', bias=bias)
    conv = QuantConv2d('ls-2', ws, 64, 10, 1, CLAMP, 'eval_only', bias=bias)
    assert {k: len(v) for k, v in lin.quantized_parameters.items()} == {k: len(v) for k, v in conv.quantized_parameters.items()}
    assert lin.quantized_parameters[ws][0] is lin.weight
    assert list(lin.state_dict().keys()) == list(conv.state_dict().keys())
    assert not any('hip' in k or 'cache' in k for k in lin.state_dict())


def test_quant_linear_is_exported():
    import quant.binary
    assert quant.binary.QuantLinear is QuantLinear


# ------------------------------------------------------------------ CPU forward
def _fill(m, seed, w_quant):
    detgen.fill_module(m, seed=seed)
    o, f = m.weight.shape
    with torch.no_grad():
        if w_quant != 'fp':
            for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight.view(o, f, 1, 1), w_quant)):
                buf.copy_(v)
    return m


def _oracle(x, m, x_scales=None):
    n, (o, f) = x.shape[0], m.weight.shape
    _, xq = P.quantize_activation(P.clamp_act(x.reshape(n, -1, 1, 1), CLAMP), m.x_quant, scales=x_scales)
    wq = P.quantize_weight(m.weight.detach().view(o, f, 1, 1), m.w_quant, m.w_approximate.cached_scales()
                           if m.w_quant != 'fp' else []).view(o, f)
    return F.linear(xq.reshape(x.shape), wq, m.bias.detach())


@pytest.mark.parametrize('xs,ws', list(itertools.product(['fp', 'ls-1', 'ls-2', 'ls-T', 'gf-3'], ['fp', 'ls-1', 'ls-2', 'ls-T', 'gf-2'])))
@pytest.mark.parametrize('shape', [(6, 96), (4, 3, 40)])
def test_cpu_forward_against_the_oracle(xs, ws, shape):
    f, o = shape[-1], 24
    m = _fill(QuantLinear(xs, ws, f, o, CLAMP), 41, ws).eval()
    x = detgen.normal('linh.x', shape, scale=1.2)
    with torch.no_grad():
        y = m(x)
        ref = _oracle(x, m)
    assert y.shape == (*shape[:-1], o)
    assert ((y - ref).abs().max() / ref.abs().max()).item() <= 1e-6, (xs, ws)


@pytest.mark.parametrize('xs', ['ls-1', 'ls-2', 'ls-T', 'gf-3'])
def test_cpu_forward_moving_average_eval(xs):
    m = _fill(QuantLinear(xs, 'ls-1', 40, 12, CLAMP, 'eval_only'), 43, 'ls-1').eval()
    nsc = m.x_approximate.num_scaling_factors
    avg = torch.tensor([0.9, 0.4, 0.2][:nsc])
    with torch.no_grad():
        m.x_approximate.moving_avg_module.moving_average.copy_(avg)
    x = detgen.normal('linh.ma.x', (5, 2, 40))
    with torch.no_grad():
        y = m(x)
        ref = _oracle(x, m, [torch.full((5,), float(v)) for v in avg])
    assert ((y - ref).abs().max() / ref.abs().max()).item() <= 1e-6


# ------------------------------------------------------------------ the same operands as a 1x1 convolution
def _pair(xs, ws, f, o, seed):
    lin = _fill(QuantLinear(xs, ws, f, o, CLAMP), seed, ws)
    conv = QuantConv2d(xs, ws, f, o, 1, CLAMP)
    with torch.no_grad():
        conv.weight.copy_(lin.weight.view(o, f, 1, 1))
        conv.bias.copy_(lin.bias)
        for a, b in zip(conv.w_approximate.cached_scales(), lin.w_approximate.cached_scales()):
            a.copy_(b)
    return lin, conv


def _capture(m):
    seen = {}
    m.x_approximate.register_forward_hook(lambda mod, i, out: seen.__setitem__('x', out.detach().clone()))
    m.w_approximate.register_forward_hook(lambda mod, i, out: seen.__setitem__('w', out.detach().clone()))
    return seen


@pytest.mark.parametrize('xs,ws', [('ls-1', 'ls-1'), ('ls-2', 'ls-1'), ('ls-T', 'ls-2'), ('gf-3', 'gf-2'), ('ls-2', 'ls-T')])
def test_same_operands_and_results_as_a_1x1_quant_conv2d(xs, ws):
    n, f, o = 8, 200, 30
    lin, conv = _pair(xs, ws, f, o, seed=47)
    x = detgen.normal('linh.pair.x', (n, f), scale=1.2)
    for train in (False, True):
        lin.train(train)
        conv.train(train)
        sl, sc = _capture(lin), _capture(conv)
        xl = x.clone().requires_grad_(train)
        xc = x.clone().view(n, f, 1, 1).requires_grad_(train)
        with torch.set_grad_enabled(train):
            yl = lin(xl)
            yc = conv(xc).view(n, o)
        assert torch.equal(sl['x'].view(n, f), sc['x'].view(n, f)), train
        assert torch.equal(sl['w'].view(o, f), sc['w'].view(o, f)), train
        bound = 1e-5 * yc.abs().max().item()
        assert (yl - yc).abs().max().item() <= bound
        if train:
            gy = detgen.normal('linh.pair.gy', (n, o))
            yl.backward(gy)
            yc.backward(gy)
            gbound = lambda t: 1e-5 * t.abs().max().item()        # noqa: E731
            assert (xl.grad - xc.grad.view(n, f)).abs().max().item() <= gbound(xc.grad)
            assert (lin.weight.grad - conv.weight.grad.view(o, f)).abs().max().item() <= gbound(conv.weight.grad)
            assert (lin.bias.grad - conv.bias.grad).abs().max().item() <= gbound(conv.bias.grad)
        for m in (lin, conv):
            m.x_approximate._forward_hooks.clear()
            m.w_approximate._forward_hooks.clear()


def test_cpu_forward_rejects_a_wrong_feature_count():
    with pytest.raises(ValueError):
        QuantLinear('ls-1', 'ls-1', 8, 3)(torch.randn(2, 9))


# ------------------------------------------------------------------ LeNet
def test_lenet_fc1_quant():
    plain = QLeNet5(loss_fn=None, x_quant='ls-2', w_quant='ls-1', clamp=CLAMP)
    again = QLeNet5(loss_fn=None, x_quant='ls-2', w_quant='ls-1', clamp=CLAMP, fc1_quant=None)
    assert type(plain.fc1) is torch.nn.Linear and list(plain.state_dict()) == list(again.state_dict())
    detgen.fill_module(plain, seed=2)
    again.load_state_dict(plain.state_dict())
    x = detgen.normal('linh.lenet.x', (3, 1, 28, 28))
    plain.eval()
    again.eval()
    with torch.no_grad():
        assert torch.equal(plain(x), again(x))
    q = QLeNet5(loss_fn=None, x_quant='ls-2', w_quant='ls-1', clamp=CLAMP,
                fc1_quant={'x_quant': 'ls-1', 'w_quant': 'ls-2', 'clamp': CLAMP})
    assert isinstance(q.fc1, QuantLinear) and (q.fc1.in_features, q.fc1.out_features) == (800, 500)
    assert q.fc1.x_quant == 'ls-1' and q.fc1.w_quant == 'ls-2' and q.fc1.clamp_config == CLAMP
    keys = set(q.state_dict()) - set(plain.state_dict())
    assert keys and all(k.startswith('fc1.') for k in keys)
    q.train()
    q(x).sum().backward()                       # the torch formulation trains through the binary fc1
    assert q.fc1.weight.grad is not None and q.fc1.w_approximate.v1.abs().sum() > 0


# ------------------------------------------------------------------ the C ABI
def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.linear_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.linear_library_path())
    assert hip.linear_lib().lsq_linear_abi_version() == hip.LINEAR_ABI_VERSION == 1


def test_header_declares_exactly_the_linear_entry_points():
    assert declared_functions() == ['lsq_linear_abi_version', 'lsq_linear_xnor']


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('no nm on this machine')
    out = subprocess.run([nm, '-D', '--defined-only', hip.linear_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def _call(hip, planes=1 << 20, kx=2, scales=1 << 20, t=1, wbits=1 << 20, wsum=1 << 20, kw=1, wscales=1 << 20, bias=None,
          M=64, F=800, O=500, y=1 << 20):
    return hip.linear_lib().lsq_linear_xnor(planes, kx, scales, t, wbits, wsum, kw, wscales, bias, M, F, O, y, None)


def test_argument_errors_return_before_a_launch(hip):
    # the pointers are never dereferenced on these paths: every call below must fail its checks first
    for name in ('planes', 'scales', 'wbits', 'wsum', 'wscales', 'y'):
        assert _call(hip, **{name: None}) == E_NULL, name
    for kw in (dict(M=0), dict(F=0), dict(O=0), dict(M=-1), dict(t=0), dict(M=64, t=3)):
        assert _call(hip, **kw) == E_SHAPE, kw
    for kw in (dict(kx=0), dict(kx=9), dict(kw=0), dict(kw=9), dict(F=1 << 22), dict(M=1 << 31), dict(O=1 << 21),
               dict(M=63, F=800, t=3)):
        assert _call(hip, **kw) == E_UNSUPPORTED, kw
    assert hip.E_UNSUPPORTED == E_UNSUPPORTED


def test_python_wrapper_checks_operands_on_the_host(hip):
    t64 = torch.zeros(8, dtype=torch.int64)
    f32 = torch.zeros((1, 4), dtype=torch.float32)
    with pytest.raises(TypeError):
        hip.linear_xnor(t64.float(), 1, f32, 1, t64, torch.zeros(4, dtype=torch.int32), f32, None, 4, 64, 4)
    with pytest.raises(ValueError):               # CPU tensors: the kernel reads device memory only
        hip.linear_xnor(t64, 1, f32, 1, torch.zeros(16, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), f32, None,
                        4, 64, 4)
