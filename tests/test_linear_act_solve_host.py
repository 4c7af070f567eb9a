"""The C ABI of liblsq_hip_linear_act_solve.so on the host (no GPU): header, exports, argument errors returned before any
launch, the Python wrapper's operand checks, the numpy model of the kernel's arithmetic against the exact oracle on every
case the GPU tests run, and QuantLinear's ``act_half_solve`` switch in the dispatch."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import act_solve_half_cases as C
from quant.binary import QuantLinear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_linear_act_solve.h')
E_NULL, E_SHAPE, E_SCHEME, E_UNSUPPORTED = -1, -2, -3, -6
F32, BF16, F16 = 0, 1, 2
LS1, LS2, LST, GF = 1, 2, 3, 4
ENTRY_POINTS = ['lsq_linear_act_quant_solve_half', 'lsq_linear_act_solve_abi_version']


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.linear_act_solve_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def test_header_declares_exactly_the_two_entry_points():
    assert declared_functions() == ENTRY_POINTS
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_LINEAR_ACT_SOLVE_ABI_VERSION\s+1\b', text)
    assert '#include "lsq_hip_linear_half.h"' in text          # LSQ_DTYPE_* are that header's


def test_the_library_is_a_sublib_of_the_build():
    import __graft_entry__
    row = [s for s in __graft_entry__.SUBLIBS if s[0] == 'linear_act_solve']
    assert len(row) == 1
    assert row[0][1:3] == ('linear_act_solve_lib', 'lsq_hip_linear_act_solve.h') and row[0][5] == 'LINEAR_ACT_SOLVE_ABI_VERSION'
    assert sorted(row[0][4]) == ENTRY_POINTS
    assert sorted(set(re.findall(r'\b(' + row[0][3] + r')\s*\(', open(HEADER).read()))) == ENTRY_POINTS
    assert os.path.exists(os.path.join(ROOT, 'ml-quant_amd', 'csrc', 'linear_act_solve', 'Makefile'))
    # the row of liblsq_hip_linear_act_half.so does not claim the new symbols
    other = [s for s in __graft_entry__.SUBLIBS if s[0] == 'linear_act_half'][0]
    assert not any(re.fullmatch(other[3], name) for name in ENTRY_POINTS)


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.linear_act_solve_library_path())
    assert hip.linear_act_solve_lib().lsq_linear_act_solve_abi_version() == hip.LINEAR_ACT_SOLVE_ABI_VERSION == 1


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('no nm on this machine')
    out = subprocess.run([nm, '-D', '--defined-only', hip.linear_act_solve_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def test_argument_errors_return_before_a_launch(hip):
    """Host buffers filled with a sentinel stand in for planes, scales and status: a refused call never dereferences a
    pointer (x is garbage) and leaves every byte as it was."""
    n, L = 4, 100
    planes = np.full((2 * n * 2,), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    scales = np.full((2, n), 12345.0, dtype=np.float32)
    status = np.full((n,), -77, dtype=np.int32)
    keep = planes.copy(), scales.copy(), status.copy()

    def call(x=1 << 20, xdt=BF16, N=n, L=L, scheme=LS2, skip=3, alpha=2.0, p=planes.ctypes.data, s=scales.ctypes.data,
             t=status.ctypes.data):
        return hip.linear_act_solve_lib().lsq_linear_act_quant_solve_half(x, xdt, N, L, scheme, skip, alpha, p, s, t, None)

    for xdt in (BF16, F16):
        for scheme in (LS2, LST):
            for name in ('x', 'p', 's'):
                assert call(xdt=xdt, scheme=scheme, **{name: None}) == E_NULL, name
            for kw in (dict(N=0), dict(L=0), dict(N=-1), dict(L=-64), dict(skip=0), dict(skip=-3)):
                assert call(xdt=xdt, scheme=scheme, **kw) == E_SHAPE, kw
            for kw in (dict(L=1 << 31), dict(N=1 << 31), dict(L=1 << 40)):
                assert call(xdt=xdt, scheme=scheme, **kw) == E_UNSUPPORTED, kw
        for scheme in (0, LS1, GF, 5, -1):
            assert call(xdt=xdt, scheme=scheme) == E_SCHEME, scheme
    for xdt in (F32, 3, -1):
        assert call(xdt=xdt) == E_UNSUPPORTED and call(xdt=xdt, scheme=LST, t=None) == E_UNSUPPORTED, xdt
    assert hip.E_UNSUPPORTED == E_UNSUPPORTED
    assert all(np.array_equal(a, b) for a, b in zip(keep, (planes, scales, status)))


def test_python_wrapper_checks_operands_on_the_host(hip):
    n, L = 4, 100
    words = 2 * n * 2
    q = hip.linear_act_quant_solve_half
    for dtype in (torch.bfloat16, torch.float16):
        x = torch.zeros((n, L), dtype=dtype)
        planes = torch.zeros((words,), dtype=torch.int64)
        scales = torch.zeros((2, n), dtype=torch.float32)
        status = torch.zeros((n,), dtype=torch.int32)
        for bad in (x.float(), x.double(), x.to(torch.int16)):
            with pytest.raises(ValueError, match='bfloat16 or float16'):
                q(bad, LS2, 3, 2.0, planes, scales)
        for scheme in (LS1, GF, 0):
            with pytest.raises(ValueError, match='ls-2 or ls-T'):
                q(x, scheme, 3, 2.0, planes, scales)
        with pytest.raises(TypeError, match='planes must be'):
            q(x, LS2, 3, 2.0, planes.int(), scales)
        with pytest.raises(TypeError, match='scales must be'):
            q(x, LS2, 3, 2.0, planes, scales.to(dtype))
        with pytest.raises(TypeError, match='status must be'):
            q(x, LS2, 3, 2.0, planes, scales, status.long())
        with pytest.raises(ValueError, match='contiguous'):
            q(torch.zeros((n, 2 * L), dtype=dtype)[:, :L], LS2, 3, 2.0, planes, scales)
        with pytest.raises(ValueError, match='bad sizes'):
            q(x.view(-1), LS2, 3, 2.0, planes, scales)
        with pytest.raises(ValueError, match='bad sizes'):
            q(x, LST, 0, 2.0, planes, scales)
        with pytest.raises(ValueError, match='do not match'):
            q(x, LS2, 3, 2.0, planes[:words - 1], scales)
        with pytest.raises(ValueError, match='do not match'):
            q(x, LS2, 3, 2.0, planes, scales[:1])
        with pytest.raises(ValueError, match='do not match'):
            q(x, LS2, 3, 2.0, planes, scales, status[:n - 1])
        for t in (None, status):                                  # CPU tensors: the kernel reads device memory only
            with pytest.raises(ValueError, match='cuda device'):
                q(x, LST, 3, 2.0, planes, scales, t)


@pytest.mark.parametrize('dt', C.DTYPES)
def test_the_model_of_the_kernels_arithmetic_equals_the_exact_oracle(dt):
    """Counts per distinct key, prefix sums in key order, the run-wise candidate test, the cost without sum a^2 and the
    (cost, position) argmin give lsq_exact's v1 bit for bit, and its found / not found, on every case of the GPU tests."""
    rows = differ = without = 0
    for li, L, d, bound, skip, scheme in C.cases():
        if d != dt:
            continue
        want, found = C.oracle(li, dt, bound, skip, scheme)
        xc = C.clamped32(C.rows(li, dt), C.rounded(bound, C.DTYPES[dt]))
        got, got_found = C.model_rows(xc, scheme == 'ls-T', skip)
        bad = int((want.view(np.int32) != got.view(np.int32)).sum()) + int((found != got_found).sum())
        if bad:
            print(f'{scheme} {dt} L={L} bound={bound} skip={skip}: oracle {want} model {got}')
        rows, differ, without = rows + len(want), differ + bad, without + int((~found).sum())
    print(f'{dt}: {differ} of {rows} rows differ between the model and lsq_exact; {without} rows have no candidate')
    assert rows == len(C.cases()) // 2 // len(C.LS) * sum(C.n_rows(L) for L in C.LS)
    assert differ == 0
    assert without > 0                                             # the v1 = 0 path is among the cases


def test_the_clamped_rows_are_values_of_their_type():
    """The bound rounded into the type keeps every clamped element a value of the type: its magnitude is a 15-bit key."""
    for dt, dtype in C.DTYPES.items():
        for bound in C.BOUNDS:
            xc = torch.from_numpy(C.clamped32(C.rows(5, dt), C.rounded(bound, dtype)))
            assert torch.equal(xc.to(dtype).float(), xc)
    assert C.rounded(1.3, torch.bfloat16) == 1.296875 and C.rounded(1.3, torch.float16) == 1.2998046875


def _lin(xq, wq='ls-1', f=64, o=3, **kw):
    return QuantLinear(xq, wq, f, o, {'kind': 'symmetric', 'alpha': 2}, **kw).eval()


def test_act_half_solve_is_off_by_default_and_switches_the_dispatch():
    assert QuantLinear.act_half_solve is False
    for dtype in (torch.bfloat16, torch.float16):
        x2, x3 = torch.zeros((2, 64), dtype=dtype), torch.zeros((2, 3, 64), dtype=dtype)
        for xq in ('ls-2', 'ls-T'):
            m = _lin(xq)
            assert not m._hip_supports(x2) and not m._hip_supports(x3)
            m.act_half_solve = True
            assert m._hip_supports(x2) and m._hip_supports(x3)
            assert not m._wants_hip(x2)                            # CPU tensors never reach the kernel
            # every other limit stays: 16-bit weights, whole plane words per row of a sample, the solver's key limit
            assert not _lin(xq).to(dtype)._hip_supports(x2)
            odd = _lin(xq, f=100)
            odd.act_half_solve = True
            assert odd._hip_supports(torch.zeros((5, 100), dtype=dtype))
            assert not odd._hip_supports(torch.zeros((5, 3, 100), dtype=dtype))
            from quant import _hip
            long_rows = _lin(xq, f=64)
            long_rows.act_half_solve = True
            t = (_hip.MAX_SOLVER_KEYS * long_rows.act_skip) // 64 + 1
            assert not long_rows._hip_supports(torch.zeros((1, t, 64), dtype=dtype).expand(1, t, 64))
            # given scales keep taking lsq_linear_act_quant_half, with the attribute on or off
            assert _lin(xq, moving_average_mode='eval_only')._hip_supports(x2)
        # the schemes without a solve do not depend on the attribute
        assert _lin('ls-1')._hip_supports(x2) and _lin('gf-3')._hip_supports(x2)
    assert QuantLinear.act_half_solve is False
