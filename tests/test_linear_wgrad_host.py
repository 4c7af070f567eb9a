"""The C ABI of liblsq_hip_linear_wgrad.so on the host (no GPU): header, exports, the workspace formula, argument errors
returned before any launch, the Python wrapper's operand checks, the missing-library error, the WGRAD_KERNEL flag of
QuantLinear's train step on the CPU -- and the kernel's prescribed arithmetic emulated on the CPU at every case of the GPU
accuracy test (tests/test_gpu_linear_wgrad.py), which is what fixes that test's seeds."""

import os
import re
import shutil
import subprocess

import pytest
import torch

import detgen
import linear_wgrad_cases as C
from quant.binary import QuantLinear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_linear_wgrad.h')
E_NULL, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5, -6


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.linear_wgrad_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def test_header_declares_exactly_the_new_entry_points():
    assert declared_functions() == ['lsq_linear_signx_wgrad', 'lsq_linear_signx_wgrad_workspace_bytes',
                                    'lsq_linear_wgrad_abi_version']
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_LINEAR_WGRAD_ABI_VERSION\s+1\b', text)


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.linear_wgrad_library_path())
    assert hip.linear_wgrad_lib().lsq_linear_wgrad_abi_version() == hip.LINEAR_WGRAD_ABI_VERSION == 1


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('no nm on this machine')
    out = subprocess.run([nm, '-D', '--defined-only', hip.linear_wgrad_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def _need(hip, kx=1, N=64, T=1, F=800, O=500):
    return int(hip.linear_wgrad_lib().lsq_linear_signx_wgrad_workspace_bytes(kx, N, T, F, O))


def _call(hip, gy=1 << 20, x=1 << 20, kx=1, xscales=1 << 20, alpha=2.0, N=64, T=1, F=800, O=500, gwq=1 << 20, ws=1 << 20,
          ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 40                        # (never touched: every call below fails its checks first)
    return hip.linear_wgrad_lib().lsq_linear_signx_wgrad(gy, x, kx, xscales, alpha, N, T, F, O, gwq, ws, ws_bytes, None)


def test_workspace_size(hip):
    # the sign image: kx * ceil(M / 64) * ceil16(F) words, M = N * T
    assert _need(hip, 1, 64, 1, 800, 500) == 1 * 1 * 800 * 8
    assert _need(hip, 2, 8192, 1, 4096, 4096) == 2 * 128 * 4096 * 8
    assert _need(hip, 3, 5, 13, 65, 7) == 3 * 2 * 80 * 8          # M = 65: M % 64 != 0, F % 16 != 0
    for kw in (dict(kx=0), dict(kx=9), dict(N=65536), dict(F=1 << 22), dict(O=1 << 21), dict(N=65535, T=1 << 16)):
        assert _need(hip, **kw) == 0, kw


def test_argument_errors_return_before_a_launch(hip):
    # the pointers are never dereferenced on these paths: every call below must fail its checks first
    for name in ('gy', 'x', 'xscales', 'gwq'):
        assert _call(hip, **{name: None}) == E_NULL, name
    for kw in (dict(N=0), dict(T=0), dict(F=0), dict(O=0), dict(N=-1), dict(F=-64), dict(O=-3)):
        assert _call(hip, **kw) == E_SHAPE, kw
    for kw in (dict(kx=0), dict(kx=9), dict(kx=-1), dict(N=65536), dict(F=1 << 22), dict(O=1 << 21),
               dict(N=65535, T=1 << 16)):                         # (the last: M = N * T >= 2^31)
        assert _call(hip, **kw) == E_UNSUPPORTED, kw
    need = _need(hip)
    assert need > 0
    assert _call(hip, ws_bytes=need - 1) == E_WORKSPACE
    assert _call(hip, ws_bytes=0) == E_WORKSPACE
    assert _call(hip, ws=None) == E_WORKSPACE
    assert _call(hip, ws=(1 << 20) + 4) == E_WORKSPACE            # not 8-byte aligned
    assert _call(hip, kx=2, ws_bytes=need) == E_WORKSPACE         # two planes need twice the image


def test_python_wrapper_checks_operands_on_the_host(hip):
    gy = torch.zeros((4, 4), dtype=torch.float32)
    x = torch.zeros((4, 64), dtype=torch.float32)
    xs = torch.ones((1, 4), dtype=torch.float32)
    with pytest.raises(TypeError):
        hip.linear_signx_wgrad(gy.double(), x, xs, 2.0, 4, 1, 64, 4)
    with pytest.raises(TypeError):
        hip.linear_signx_wgrad(gy, x.half(), xs, 2.0, 4, 1, 64, 4)
    with pytest.raises(TypeError):
        hip.linear_signx_wgrad(gy, x, xs.double(), 2.0, 4, 1, 64, 4)
    with pytest.raises(ValueError, match='cuda device'):          # CPU tensors: the kernel reads device memory only
        hip.linear_signx_wgrad(gy, x, xs, 2.0, 4, 1, 64, 4)
    with pytest.raises(ValueError, match='contiguous'):
        hip.linear_signx_wgrad(torch.zeros((4, 8))[:, ::2], x, xs, 2.0, 4, 1, 64, 4)
    with pytest.raises(ValueError, match='contiguous'):
        hip.linear_signx_wgrad(gy, torch.zeros((4, 128))[:, ::2], xs, 2.0, 4, 1, 64, 4)
    with pytest.raises(ValueError, match='do not match'):         # scales of another sample count
        hip.linear_signx_wgrad(gy, x, torch.ones((1, 5)), 2.0, 4, 1, 64, 4)
    with pytest.raises(ValueError, match='do not match'):         # per-row scales where the rows share a sample's
        hip.linear_signx_wgrad(gy, x, xs, 2.0, 2, 2, 64, 4)
    with pytest.raises(ValueError, match='do not match'):
        hip.linear_signx_wgrad(gy, x, torch.ones((4,)), 2.0, 4, 1, 64, 4)
    with pytest.raises(ValueError, match='bad sizes'):
        hip.linear_signx_wgrad(gy, x, xs, 2.0, 5, 1, 64, 4)
    with pytest.raises(ValueError, match='bad sizes'):
        hip.linear_signx_wgrad(gy, x, xs, 2.0, 4, 1, 65, 4)
    with pytest.raises(ValueError, match='bad sizes'):
        hip.linear_signx_wgrad(gy, x, xs, 2.0, 4, 0, 64, 4)


def test_a_missing_library_is_an_error(hip, monkeypatch, tmp_path):
    monkeypatch.setattr(hip, '_LIB_DIR', str(tmp_path))              # (where the libraries are looked for: none is there)
    monkeypatch.delitem(hip._handles, 'linear_wgrad', raising=False)
    assert hip.linear_wgrad_library_path() == str(tmp_path / 'liblsq_hip_linear_wgrad.so')
    with pytest.raises(hip.LsqHipError, match='csrc/linear_wgrad'):
        hip.linear_wgrad_lib()


def test_the_flag_is_off_by_default():
    from quant.binary import hip_train_linear
    assert hip_train_linear.WGRAD_KERNEL is False


@pytest.mark.parametrize('xs,ws', [('ls-2', 'ls-1'), ('fp', 'ls-2')])
def test_cpu_train_step_stays_the_torch_formulation_with_the_flag_on(xs, ws, monkeypatch):
    from quant.binary import hip_train_linear
    monkeypatch.setattr(hip_train_linear, 'WGRAD_KERNEL', True)
    clamp = {'kind': 'symmetric', 'alpha': 2}
    x = detgen.normal('linwgrad.host.x', (6, 3, 64), scale=1.2)
    gy = detgen.normal('linwgrad.host.gy', (6, 3, 10))
    res = []
    for flag in (True, False):
        m = QuantLinear(xs, ws, 64, 10, clamp)
        with torch.no_grad():
            m.weight.copy_(detgen.normal('linwgrad.host.w', m.weight.shape, scale=0.3))
            m.bias.copy_(detgen.normal('linwgrad.host.b', m.bias.shape, scale=0.1))
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


def test_prescribed_arithmetic_stays_inside_half_the_bound():
    """For every case of the GPU accuracy test: the signs of the fp32 chain, a = fl32(gy xs), hi = bf16(a), lo = bf16(a - hi)
    -- the kernel's operands -- summed EXACTLY (fp64) against the fp64 reference gy^T . (sum_p xs_p b_p).  What the split
    alone costs has to stay within half of the bound the kernel is held to, so that the GPU test measures the kernel and
    not a draw in which max |ref| cancels; the seed base is the first of 0, 1000, 2000, ... for which that holds at every
    case (measured here: worst 4.8e-6 at (ls-T, M = 1, 33 x 16), 2.0-3.5e-6 elsewhere).  Where M >= 1000 a single bf16
    operand is at least 10 bounds away (measured 1.5-2.8e-3), so the GPU test can tell that the lo pass is present."""
    assert C.SEED_BASE % 1000 == 0
    cases = C.accuracy_cases()
    assert len(cases) == len(C.SCHEMES) * len(C.MS)
    worst = 0.0
    for scheme, m, o, f, seed in cases:
        assert o * f >= 10
        c = C.make(m, 1, f, o, scheme, seed)
        assert len(c['signs']) == C.planes(scheme) == c['xs'].shape[0]
        ref = C.reference64(c)
        scale = ref.abs().max().item()
        err = (C.emulated64(c) - ref).abs().max().item()
        worst = max(worst, err / scale)
        assert err <= 0.5 * C.BOUND * scale, (scheme, m, o, f, err / scale)
        if m >= 1000:
            e1 = (C.emulated64(c, lo_pass=False) - ref).abs().max().item()
            assert e1 >= 10 * C.BOUND * scale, (scheme, m, o, f, e1 / scale)
    print(f'prescribed arithmetic, worst case: {worst:.3e} of max |ref|')
