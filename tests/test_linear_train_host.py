"""The C ABI of liblsq_hip_linear_train.so on the host (no GPU): header, exports, argument errors returned before any
launch, the Python wrapper's operand checks, the missing-library error, and QuantLinear's train-step dispatch on the CPU."""

import os
import re
import shutil
import subprocess

import pytest
import torch

import detgen
from quant.binary import QuantLinear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_linear_train.h')
E_NULL, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5, -6


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.linear_train_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def test_header_declares_exactly_the_new_entry_points():
    assert declared_functions() == ['lsq_linear_signw_dgrad', 'lsq_linear_signw_dgrad_workspace_bytes',
                                    'lsq_linear_train_abi_version']
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_LINEAR_TRAIN_ABI_VERSION\s+1\b', text)


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.linear_train_library_path())
    assert hip.linear_train_lib().lsq_linear_train_abi_version() == hip.LINEAR_TRAIN_ABI_VERSION == 1


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('no nm on this machine')
    out = subprocess.run([nm, '-D', '--defined-only', hip.linear_train_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def _need(hip, kw=1, F=800, O=500):
    return int(hip.linear_train_lib().lsq_linear_signw_dgrad_workspace_bytes(kw, F, O))


def _call(hip, gy=1 << 20, wbits=1 << 20, kw=1, wscales=1 << 20, M=64, F=800, O=500, gx=1 << 20, ws=1 << 20, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 40                        # (never touched: every call below fails its checks first)
    return hip.linear_train_lib().lsq_linear_signw_dgrad(gy, wbits, kw, wscales, M, F, O, gx, ws, ws_bytes, None)


def test_workspace_size(hip):
    # the transposed plane image: kw * ceil(O / 64) * ceil16(F) words
    assert _need(hip, 1, 800, 500) == 8 * 800 * 8
    assert _need(hip, 3, 65, 64) == 3 * 1 * 80 * 8
    assert _need(hip, 2, 1, 65) == 2 * 2 * 16 * 8


def test_argument_errors_return_before_a_launch(hip):
    # the pointers are never dereferenced on these paths: every call below must fail its checks first
    for name in ('gy', 'wbits', 'wscales', 'gx'):
        assert _call(hip, **{name: None}) == E_NULL, name
    for kw in (dict(M=0), dict(F=0), dict(O=0), dict(M=-1), dict(F=-64), dict(O=-3)):
        assert _call(hip, **kw) < 0, kw
    for kw in (dict(kw=0), dict(kw=9), dict(kw=-1), dict(F=1 << 22), dict(M=1 << 31), dict(O=1 << 21)):
        assert _call(hip, **kw) == E_UNSUPPORTED, kw
    need = _need(hip)
    assert need > 0
    assert _call(hip, ws_bytes=need - 1) == E_WORKSPACE
    assert _call(hip, ws_bytes=0) == E_WORKSPACE
    assert _call(hip, ws=None) < 0
    assert _call(hip, kw=2, ws_bytes=need) == E_WORKSPACE         # two planes need twice the image


def test_python_wrapper_checks_operands_on_the_host(hip):
    gy = torch.zeros((4, 4), dtype=torch.float32)
    wbits = torch.zeros((16,), dtype=torch.int64)
    wsc = torch.ones((1, 4), dtype=torch.float32)
    with pytest.raises(TypeError):
        hip.linear_signw_dgrad(gy.double(), wbits, wsc, 4, 64, 4)
    with pytest.raises(TypeError):
        hip.linear_signw_dgrad(gy, wbits.int(), wsc, 4, 64, 4)
    with pytest.raises(TypeError):
        hip.linear_signw_dgrad(gy, wbits, wsc.half(), 4, 64, 4)
    with pytest.raises(ValueError, match='cuda device'):          # CPU tensors: the kernel reads device memory only
        hip.linear_signw_dgrad(gy, wbits, wsc, 4, 64, 4)
    with pytest.raises(ValueError, match='contiguous'):
        hip.linear_signw_dgrad(torch.zeros((4, 8))[:, ::2], wbits, wsc, 4, 64, 4)
    with pytest.raises(ValueError, match='do not match'):         # planes of another (kw, F, O)
        hip.linear_signw_dgrad(gy, wbits, wsc, 4, 65, 4)
    with pytest.raises(ValueError, match='do not match'):
        hip.linear_signw_dgrad(gy, wbits, torch.ones((2, 4)), 4, 64, 4)
    with pytest.raises(ValueError, match='do not match'):
        hip.linear_signw_dgrad(gy, wbits, torch.ones((1, 5)), 4, 64, 4)
    with pytest.raises(ValueError, match='bad sizes'):
        hip.linear_signw_dgrad(gy, wbits, wsc, 5, 64, 4)


def test_a_missing_library_is_an_error(hip, monkeypatch, tmp_path):
    monkeypatch.setattr(hip, '_LIB_DIR', str(tmp_path))              # (where the libraries are looked for: none is there)
    monkeypatch.delitem(hip._handles, 'linear_train', raising=False)
    assert hip.linear_train_library_path() == str(tmp_path / 'liblsq_hip_linear_train.so')
    with pytest.raises(hip.LsqHipError, match='csrc/linear_train'):
        hip.linear_train_lib()


def test_supported_is_false_on_the_cpu():
    from quant.binary import hip_train_linear
    m = QuantLinear('ls-2', 'ls-1', 64, 8).train()
    assert not hip_train_linear.supported(m, torch.zeros((4, 64)))
    assert not hip_train_linear.supported(QuantLinear('fp', 'ls-1', 64, 8).train(), torch.zeros((4, 3, 64)))


@pytest.mark.parametrize('xs,ws', [('ls-2', 'ls-1'), ('fp', 'ls-2')])
def test_cpu_train_step_stays_the_torch_formulation(xs, ws):
    assert QuantLinear.hip_train is False
    clamp = {'kind': 'symmetric', 'alpha': 2}
    x = detgen.normal('lintrain.host.x', (6, 3, 64), scale=1.2)
    gy = detgen.normal('lintrain.host.gy', (6, 3, 10))
    res = []
    for flag in (True, False):
        m = QuantLinear(xs, ws, 64, 10, clamp)
        with torch.no_grad():
            m.weight.copy_(detgen.normal('lintrain.host.w', m.weight.shape, scale=0.3))
            m.bias.copy_(detgen.normal('lintrain.host.b', m.bias.shape, scale=0.1))
        m.hip_train = flag
        m.train()
        xi = x.clone().requires_grad_()
        y = m(xi)
        ref = m._forward_torch(xi)
        assert torch.equal(y, ref)
        assert type(y.grad_fn).__name__ != '_QuantLinearStepBackward'
        y.backward(gy)
        res.append((y.detach(), xi.grad, m.weight.grad, m.bias.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)
