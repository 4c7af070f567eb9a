"""The C ABI of liblsq_hip_linear_act_half.so on the host (no GPU): header, exports, argument errors returned before any
launch, the Python wrapper's operand checks, QuantLinear's dispatch truth table for 16-bit inputs with binary activations,
and the clamp bound the module hands to the kernel (rounded into the tensor's type, as Tensor.clamp rounds it)."""

import os
import re
import shutil
import subprocess

import pytest
import torch

from quant.binary import QuantLinear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_linear_act_half.h')
E_NULL, E_SHAPE, E_SCHEME, E_UNSUPPORTED = -1, -2, -3, -6
F32, BF16, F16 = 0, 1, 2
LS1, LS2, LST, GF = 1, 2, 3, 4
ENTRY_POINTS = ['lsq_linear_act_half_abi_version', 'lsq_linear_act_quant_half']


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.linear_act_half_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def test_header_declares_exactly_the_new_entry_points():
    assert declared_functions() == ENTRY_POINTS
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_LINEAR_ACT_HALF_ABI_VERSION\s+1\b', text)
    assert '#include "lsq_hip_linear_half.h"' in text          # LSQ_DTYPE_* are that header's


def test_the_library_is_a_sublib_of_the_build():
    import __graft_entry__
    row = [s for s in __graft_entry__.SUBLIBS if s[0] == 'linear_act_half']
    assert len(row) == 1
    assert row[0][1:3] == ('linear_act_half_lib', 'lsq_hip_linear_act_half.h') and row[0][5] == 'LINEAR_ACT_HALF_ABI_VERSION'
    assert sorted(row[0][4]) == ENTRY_POINTS
    assert sorted(set(re.findall(r'\b(' + row[0][3] + r')\s*\(', open(HEADER).read()))) == ENTRY_POINTS
    assert os.path.exists(os.path.join(ROOT, 'ml-quant_amd', 'csrc', 'linear_act_half', 'Makefile'))


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.linear_act_half_library_path())
    assert hip.linear_act_half_lib().lsq_linear_act_half_abi_version() == hip.LINEAR_ACT_HALF_ABI_VERSION == 1


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('no nm on this machine')
    out = subprocess.run([nm, '-D', '--defined-only', hip.linear_act_half_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def _call(hip, x=1 << 20, xdt=BF16, N=64, L=800, scheme=LS1, k=1, alpha=2.0, forced=None, planes=1 << 21, scales=1 << 22):
    return hip.linear_act_half_lib().lsq_linear_act_quant_half(x, xdt, N, L, scheme, k, alpha, forced, planes, scales, None)


def test_argument_errors_return_before_a_launch(hip):
    # the pointers are null or garbage and never dereferenced on these paths: every call below must fail its checks first
    for xdt in (BF16, F16):
        for forced in (None, 1 << 23):
            for name in ('x', 'planes', 'scales'):
                assert _call(hip, xdt=xdt, forced=forced, **{name: None}) == E_NULL, name
            for kw in (dict(N=0), dict(L=0), dict(N=-1), dict(L=-64)):
                assert _call(hip, xdt=xdt, forced=forced, **kw) == E_SHAPE, kw
            for kw in (dict(scheme=0), dict(scheme=5), dict(scheme=-1), dict(scheme=GF, k=0), dict(scheme=GF, k=9),
                       dict(scheme=GF, k=-1), dict(scheme=LS1, k=0), dict(scheme=LS1, k=2), dict(scheme=LS2, k=1),
                       dict(scheme=LST, k=3), dict(scheme=LS2, k=9)):
                assert _call(hip, xdt=xdt, forced=forced, **kw) == E_SCHEME, kw
            for kw in (dict(L=1 << 31), dict(N=1 << 31), dict(L=1 << 40, scheme=GF, k=3)):
                assert _call(hip, xdt=xdt, forced=forced, **kw) == E_UNSUPPORTED, kw
        # the free-running ls-2 / ls-T solve is not this library's
        assert _call(hip, xdt=xdt, scheme=LS2, k=2) == E_UNSUPPORTED
        assert _call(hip, xdt=xdt, scheme=LST, k=2) == E_UNSUPPORTED
    for xdt in (F32, 3, -1):
        for scheme, k, forced in ((LS1, 1, None), (GF, 3, None), (LS2, 2, 1 << 23), (LST, 2, 1 << 23)):
            assert _call(hip, xdt=xdt, scheme=scheme, k=k, forced=forced) == E_UNSUPPORTED, (xdt, scheme)
    assert hip.E_UNSUPPORTED == E_UNSUPPORTED


def test_python_wrapper_checks_operands_on_the_host(hip):
    n, L, k = 4, 100, 2
    words = k * n * 2
    for dtype in (torch.bfloat16, torch.float16):
        x = torch.zeros((n, L), dtype=dtype)
        planes = torch.zeros((words,), dtype=torch.int64)
        scales = torch.zeros((k, n), dtype=torch.float32)
        forced = torch.ones((k, n), dtype=torch.float32)
        q = hip.linear_act_quant_half
        for bad in (x.float(), x.double(), x.to(torch.int16)):
            with pytest.raises(TypeError, match='bfloat16 or float16'):
                q(bad, GF, k, 2.0, planes, scales)
        with pytest.raises(TypeError, match='planes must be'):
            q(x, GF, k, 2.0, planes.int(), scales)
        with pytest.raises(TypeError, match='scales must be'):
            q(x, GF, k, 2.0, planes, scales.to(dtype))
        with pytest.raises(TypeError, match='forced must be'):
            q(x, GF, k, 2.0, planes, scales, forced.double())
        with pytest.raises(ValueError, match='contiguous'):
            q(torch.zeros((n, 2 * L), dtype=dtype)[:, :L], GF, k, 2.0, planes, scales)
        with pytest.raises(ValueError, match='bad sizes'):
            q(x.view(-1), GF, k, 2.0, planes, scales)
        with pytest.raises(ValueError, match='bad sizes'):
            q(x, GF, 0, 2.0, planes, scales)
        with pytest.raises(ValueError, match='do not match'):
            q(x, GF, k, 2.0, planes[:words - 1], scales)
        with pytest.raises(ValueError, match='do not match'):
            q(x, GF, k, 2.0, planes, scales[:1])
        with pytest.raises(ValueError, match='do not match'):
            q(x, GF, k, 2.0, planes, scales, forced.t().contiguous())
        for scheme in (LS2, LST):
            with pytest.raises(ValueError, match='forced scales'):
                q(x, scheme, 2, 2.0, planes, scales)
        for f in (None, forced):                                  # CPU tensors: the kernel reads device memory only
            with pytest.raises(ValueError, match='cuda device'):
                q(x, GF, k, 2.0, planes, scales, f)
        with pytest.raises(ValueError, match='cuda device'):
            q(x, LS2, 2, 2.0, planes, scales, forced)


def _lin(xq, wq='ls-1', f=64, o=3, **kw):
    return QuantLinear(xq, wq, f, o, {'kind': 'symmetric', 'alpha': 2}, **kw).eval()


def test_dispatch_truth_table_for_sixteen_bit_inputs():
    for dtype in (torch.bfloat16, torch.float16):
        x2, x3 = torch.zeros((2, 64), dtype=dtype), torch.zeros((2, 3, 64), dtype=dtype)
        for xq in ('ls-1', 'gf-3', 'gf-8'):
            assert _lin(xq)._hip_supports(x2) and _lin(xq)._hip_supports(x3), xq
            assert _lin(xq, 'gf-8')._hip_supports(x2)
            assert not _lin(xq, 'gf-9')._hip_supports(x2)
            assert not _lin(xq)._wants_hip(x2)                    # CPU tensors never reach the kernel
        assert not _lin('gf-9')._hip_supports(x2)
        for xq in ('ls-2', 'ls-T'):
            assert not _lin(xq)._hip_supports(x2), xq              # free-running: the solve reads fp32 rows
            assert _lin(xq)._hip_supports(x2.float())
            assert _lin(xq, moving_average_mode='eval_only')._hip_supports(x2), xq
            assert _lin(xq, moving_average_mode='train_and_eval')._hip_supports(x3), xq
            m = _lin(xq)
            m.x_approximate._forced_scales = torch.ones((m.x_approximate.num_scaling_factors, 2))
            assert m._hip_supports(x2), xq
        # 16-bit weights stay on torch whatever the activations
        for xq in ('ls-1', 'gf-3'):
            assert not _lin(xq).to(dtype)._hip_supports(x2)
        assert not _lin('ls-2', moving_average_mode='eval_only').to(dtype)._hip_supports(x2)
        # the rows of a sample must start on whole plane words
        assert _lin('ls-1', f=100)._hip_supports(torch.zeros((5, 100), dtype=dtype))
        assert _lin('ls-1', f=100)._hip_supports(torch.zeros((5, 1, 100), dtype=dtype))
        assert not _lin('ls-1', f=100)._hip_supports(torch.zeros((5, 3, 100), dtype=dtype))
        assert not _lin('gf-3', f=65)._hip_supports(torch.zeros((5, 2, 65), dtype=dtype))
        assert _lin('gf-3', f=128)._hip_supports(torch.zeros((5, 2, 128), dtype=dtype))
    assert not _lin('ls-1')._hip_supports(torch.zeros((2, 64), dtype=torch.float64))
    assert QuantLinear.act_half_kernel in (True, False)


@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float16))
def test_the_bound_handed_to_the_kernel_is_tensor_clamps(dtype):
    """QuantLinear._alpha_in(dtype) is the bound Tensor.clamp uses on a tensor of the type: clamping x.float() to it gives
    x.clamp(-alpha, alpha) exactly."""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn((32, 129), generator=g) * 2).to(dtype)
    known = {(torch.bfloat16, 1.3): 1.296875, (torch.float16, 1.3): 1.2998046875, (torch.float16, 0.7): 0.7001953125}
    for alpha in (0.7, 1.3, 2, 3):
        m = QuantLinear('ls-1', 'ls-1', 129, 3, {'kind': 'symmetric', 'alpha': alpha})
        a = m._alpha_in(dtype)
        assert a == torch.tensor(alpha, dtype=dtype).item()
        if (dtype, alpha) in known:
            assert a == known[(dtype, alpha)]
        assert torch.equal(x.float().clamp(-a, a), x.clamp(-alpha, alpha).float())
    assert QuantLinear('ls-1', 'ls-1', 129, 3)._alpha_in(dtype) == -1.0
