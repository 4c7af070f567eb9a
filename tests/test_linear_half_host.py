"""The C ABI of liblsq_hip_linear_half.so on the host (no GPU): header, exports, argument errors returned before any launch,
the Python wrapper's operand checks, QuantLinear's kernel limits for 16-bit inputs, and the clamp contract of the header
(the bound rounded into the tensor's type) checked on torch's own clamp."""

import os
import re
import shutil
import subprocess

import pytest
import torch

from quant.binary import QuantLinear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_linear_half.h')
E_NULL, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5, -6
F32, BF16, F16 = 0, 1, 2
ENTRY_POINTS = ['lsq_linear_half_abi_version', 'lsq_linear_signw_half', 'lsq_linear_signw_half_workspace_bytes']


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.linear_half_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def test_header_declares_exactly_the_new_entry_points():
    assert declared_functions() == ENTRY_POINTS
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_LINEAR_HALF_ABI_VERSION\s+1\b', text)
    assert re.search(r'LSQ_DTYPE_F32\s*=\s*0,\s*LSQ_DTYPE_BF16\s*=\s*1,\s*LSQ_DTYPE_F16\s*=\s*2', text)


def test_the_library_is_a_sublib_of_the_build():
    import __graft_entry__
    row = [s for s in __graft_entry__.SUBLIBS if s[0] == 'linear_half']
    assert len(row) == 1
    assert row[0][1:3] == ('linear_half_lib', 'lsq_hip_linear_half.h') and row[0][5] == 'LINEAR_HALF_ABI_VERSION'
    assert sorted(row[0][4]) == ENTRY_POINTS
    assert sorted(set(re.findall(r'\b(' + row[0][3] + r')\s*\(', open(HEADER).read()))) == ENTRY_POINTS


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.linear_half_library_path())
    assert hip.linear_half_lib().lsq_linear_half_abi_version() == hip.LINEAR_HALF_ABI_VERSION == 1
    assert hip.LINEAR_HALF_DTYPES == {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('no nm on this machine')
    out = subprocess.run([nm, '-D', '--defined-only', hip.linear_half_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def _call(hip, x=1 << 20, xdt=BF16, alpha=2.0, wbits=1 << 20, kw=1, wscales=1 << 20, bias=None, M=64, F=800, O=500, y=1 << 20,
          ydt=None, ws=None, ws_bytes=0):
    return hip.linear_half_lib().lsq_linear_signw_half(x, xdt, alpha, wbits, kw, wscales, bias, M, F, O, y,
                                                       xdt if ydt is None else ydt, ws, ws_bytes, None)


def test_argument_errors_return_before_a_launch(hip):
    # the pointers are never dereferenced on these paths: every call below must fail its checks first
    for xdt in (BF16, F16):
        for name in ('x', 'wbits', 'wscales', 'y'):
            assert _call(hip, xdt=xdt, **{name: None}) == E_NULL, name
        for kw in (dict(M=0), dict(F=0), dict(O=0), dict(M=-1), dict(F=-64), dict(O=-3)):
            assert _call(hip, xdt=xdt, **kw) == E_SHAPE, kw
        for kw in (dict(kw=0), dict(kw=9), dict(kw=-1), dict(F=1 << 22), dict(M=1 << 31), dict(O=1 << 21)):
            assert _call(hip, xdt=xdt, **kw) == E_UNSUPPORTED, kw
            assert _call(hip, xdt=xdt, ydt=F32, **kw) == E_UNSUPPORTED, kw
    # types: x must be 16-bit, y fp32 or x's type
    for xdt, ydt in ((F32, F32), (F32, BF16), (3, 3), (-1, F32), (BF16, F16), (F16, BF16), (BF16, 3), (F16, -1)):
        assert _call(hip, xdt=xdt, ydt=ydt) == E_UNSUPPORTED, (xdt, ydt)
    assert hip.E_UNSUPPORTED == E_UNSUPPORTED


def test_workspace_size_and_errors(hip):
    need = hip.linear_half_lib().lsq_linear_signw_half_workspace_bytes
    for dt in (BF16, F16):
        assert need(64, 500, 1, dt) == 0 and need(64, 500, 2, dt) == 0
        for kw in range(3, 9):
            assert need(64, 500, kw, dt) == 4 * 64 * 500          # the fp32 running sum between launches
        assert need((1 << 31) - 1, (1 << 21) - 1, 8, dt) == 4 * ((1 << 31) - 1) * ((1 << 21) - 1)
    for kw in range(1, 9):
        assert need(64, 500, kw, F32) == 0                        # an fp32 y holds its own running sum
    for xdt in (BF16, F16):
        # needed and missing, too small or misaligned: refused before a launch
        assert _call(hip, xdt=xdt, kw=3) == E_WORKSPACE
        assert _call(hip, xdt=xdt, kw=3, ws=1 << 20, ws_bytes=4 * 64 * 500 - 1) == E_WORKSPACE
        assert _call(hip, xdt=xdt, kw=8, ws=(1 << 20) + 2, ws_bytes=4 * 64 * 500) == E_WORKSPACE
        assert _call(hip, xdt=xdt, kw=8, ws=None, ws_bytes=1 << 30) == E_WORKSPACE


def test_python_wrapper_checks_operands_on_the_host(hip):
    wbits = torch.zeros((16,), dtype=torch.int64)
    wsc = torch.ones((1, 4), dtype=torch.float32)
    bias = torch.zeros((4,), dtype=torch.float32)
    for dtype, other in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)):
        x = torch.zeros((4, 64), dtype=dtype)
        for bad in (x.float(), x.double(), x.to(torch.int16)):
            with pytest.raises(TypeError):
                hip.linear_signw_half(bad, 2.0, wbits, wsc, None, 4, 64, 4)
        with pytest.raises(TypeError):
            hip.linear_signw_half(x, 2.0, wbits.int(), wsc, None, 4, 64, 4)
        with pytest.raises(TypeError):
            hip.linear_signw_half(x, 2.0, wbits, wsc.to(dtype), None, 4, 64, 4)
        with pytest.raises(TypeError):
            hip.linear_signw_half(x, 2.0, wbits, wsc, bias.to(dtype), 4, 64, 4)
        for out_dtype in (other, torch.float64):
            with pytest.raises(TypeError):
                hip.linear_signw_half(x, 2.0, wbits, wsc, None, 4, 64, 4, out_dtype=out_dtype)
        with pytest.raises(ValueError, match='bad sizes'):
            hip.linear_signw_half(x, 2.0, wbits, wsc, None, 5, 64, 4)
        with pytest.raises(ValueError, match='do not match'):
            hip.linear_signw_half(x, 2.0, wbits[:8], wsc, None, 4, 64, 4)
        for out_dtype in (None, dtype, torch.float32):            # CPU tensors: the kernel reads device memory only
            with pytest.raises(ValueError, match='cuda device'):
                hip.linear_signw_half(x, 2.0, wbits, wsc, bias, 4, 64, 4, out_dtype=out_dtype)


def test_hip_supports_sixteen_bit_inputs():
    for dtype in (torch.bfloat16, torch.float16):
        m = QuantLinear('fp', 'ls-1', 65, 3).eval()
        assert m._hip_supports(torch.zeros((2, 3, 65), dtype=dtype))
        assert QuantLinear('fp', 'gf-8', 65, 3)._hip_supports(torch.zeros((2, 65), dtype=dtype))
        assert not QuantLinear('fp', 'gf-9', 65, 3)._hip_supports(torch.zeros((2, 65), dtype=dtype))
        # binary activations: lsq_act_quant is fp32
        assert not QuantLinear('ls-2', 'ls-1', 64, 3)._hip_supports(torch.zeros((2, 64), dtype=dtype))
        # 16-bit weights stay on torch, whatever the input
        half = QuantLinear('fp', 'ls-1', 65, 3).to(dtype)
        assert not half._hip_supports(torch.zeros((2, 65), dtype=dtype))
        assert not half._hip_supports(torch.zeros((2, 65)))
        # CPU tensors never reach the kernel
        assert not m._wants_hip(torch.zeros((2, 3, 65), dtype=dtype))
    m = QuantLinear('fp', 'ls-1', 65, 3).eval()
    assert m._hip_supports(torch.zeros((2, 65)))                  # fp32 as before
    assert not m._hip_supports(torch.zeros((2, 3, 65), dtype=torch.float64))
    assert not QuantLinear('ls-2', 'ls-1', 64, 3)._hip_supports(torch.zeros((2, 64), dtype=torch.float64))


def test_tile_classes_follow_the_kernels_rule():
    cls = QuantLinear._tile_class
    assert cls(16, 4096) == 'split' and cls(1000, 1033) == 'small' and cls(1024, 1000) == 'small'
    assert cls(2040, 2050) == 'big' and cls(2048, 2048) == 'big' and cls(8192, 4096) == 'big'
    assert cls(64 * 255, 64) == 'split' and cls(64 * 256, 64) == 'small'
    assert QuantLinear.half_kernel_classes <= {'split', 'small', 'big'}


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16))
def test_clamp_rounds_its_bound_into_the_tensors_type(dtype):
    """The header's clamp contract is Tensor.clamp's: x16.clamp(-a, a) clamps to a rounded to nearest into the type, so
    every clamped value is a value of the type."""
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((64, 257), generator=g) * 2).to(dtype)
    known = {(torch.bfloat16, 1.3): 1.296875, (torch.float16, 0.7): 0.7001953125}
    for alpha in (0.7, 1.3, 2, 3):
        a = torch.tensor(alpha, dtype=dtype)
        if (dtype, alpha) in known:
            assert a.item() == known[(dtype, alpha)]
        y = x.clamp(-alpha, alpha)
        assert y.dtype == dtype
        assert torch.equal(y, torch.minimum(torch.maximum(x, -a), a))
        assert y.max().item() == a.item() and y.min().item() == -a.item()
        assert torch.equal(y.float(), x.float().clamp(-a.item(), a.item()))
