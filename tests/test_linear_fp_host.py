"""The C ABI of liblsq_hip_linear_fp.so on the host (no GPU): header, exports, argument errors returned before any launch,
the Python wrapper's operand checks, and QuantLinear's kernel limits for fp activations."""

import os
import re
import shutil
import subprocess

import pytest
import torch

from quant.binary import QuantLinear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_linear_fp.h')
E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -6


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.linear_fp_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def test_header_declares_exactly_the_new_entry_points():
    assert declared_functions() == ['lsq_linear_fp_abi_version', 'lsq_linear_signw']
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_LINEAR_FP_ABI_VERSION\s+1\b', text)


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.linear_fp_library_path())
    assert hip.linear_fp_lib().lsq_linear_fp_abi_version() == hip.LINEAR_FP_ABI_VERSION == 1


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('no nm on this machine')
    out = subprocess.run([nm, '-D', '--defined-only', hip.linear_fp_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def _call(hip, x=1 << 20, alpha=2.0, wbits=1 << 20, kw=1, wscales=1 << 20, bias=None, M=64, F=800, O=500, y=1 << 20):
    return hip.linear_fp_lib().lsq_linear_signw(x, alpha, wbits, kw, wscales, bias, M, F, O, y, None)


def test_argument_errors_return_before_a_launch(hip):
    # the pointers are never dereferenced on these paths: every call below must fail its checks first
    for name in ('x', 'wbits', 'wscales', 'y'):
        assert _call(hip, **{name: None}) == E_NULL, name
    for kw in (dict(M=0), dict(F=0), dict(O=0), dict(M=-1), dict(F=-64), dict(O=-3)):
        assert _call(hip, **kw) == E_SHAPE, kw
    for kw in (dict(kw=0), dict(kw=9), dict(kw=-1), dict(F=1 << 22), dict(M=1 << 31), dict(O=1 << 21)):
        assert _call(hip, **kw) == E_UNSUPPORTED, kw
    assert hip.E_UNSUPPORTED == E_UNSUPPORTED


def test_python_wrapper_checks_operands_on_the_host(hip):
    x = torch.zeros((4, 64), dtype=torch.float32)
    wbits = torch.zeros((16,), dtype=torch.int64)
    wsc = torch.ones((1, 4), dtype=torch.float32)
    with pytest.raises(TypeError):
        hip.linear_signw(x.double(), 2.0, wbits, wsc, None, 4, 64, 4)
    with pytest.raises(TypeError):
        hip.linear_signw(x, 2.0, wbits.int(), wsc, None, 4, 64, 4)
    with pytest.raises(TypeError):
        hip.linear_signw(x, 2.0, wbits, wsc.half(), None, 4, 64, 4)
    with pytest.raises(ValueError):               # CPU tensors: the kernel reads device memory only
        hip.linear_signw(x, 2.0, wbits, wsc, None, 4, 64, 4)


def test_hip_supports_fp_activations():
    from quant import _hip
    m = QuantLinear('fp', 'ls-1', 65, 3).eval()
    assert m._hip_supports(torch.zeros((2, 3, 65)))
    assert QuantLinear('fp', 'gf-8', 65, 3)._hip_supports(torch.zeros((2, 65)))
    assert not QuantLinear('fp', 'gf-9', 65, 3)._hip_supports(torch.zeros((2, 65)))
    assert not m._hip_supports(torch.zeros((2, 3, 65), dtype=torch.float64))
    assert not QuantLinear('fp', 'ls-1', 1, _hip.LINEAR_MAX_OUTPUTS)._hip_supports(torch.zeros((2, 1)))
    # CPU tensors and ('fp', 'fp') never reach the kernel
    assert not m._wants_hip(torch.zeros((2, 3, 65)))
    assert not QuantLinear('fp', 'fp', 65, 3).eval()._wants_hip(torch.zeros((2, 65)))
