"""The C ABI of liblsq_hip_conv_half.so on the host (no GPU): header, build row, exports, argument errors returned before any
launch, the workspace rule, the case table of tests/golden/conv_half_cases.py against lsq_signw_conv2d_half_plan, the table's
fp64 reference against an independent restatement and against fp32 arithmetic, the Python wrapper's operand checks and
QuantConv2d's ``fp_half`` switch in the dispatch."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_half_cases as C
from oracle import ref_port as P
from quant.binary.binary_conv import QuantConv2d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_conv_half.h')
E_NULL, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5, -6
F32, BF16, F16 = 0, 1, 2
ENTRY_POINTS = ['lsq_conv_half_abi_version', 'lsq_signw_conv2d_half', 'lsq_signw_conv2d_half_plan',
                'lsq_signw_conv2d_half_workspace_bytes']
PATTERN = r'lsq_conv_half_[a-z0-9_]+|lsq_signw_conv2d_half[a-z0-9_]*'


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.conv_half_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def _geom(hip, c):
    return hip.make_geom(c.N, c.C, c.H, c.W, c.O, c.KH, c.KW, c.stride, c.pad, c.dil, c.groups)


def test_header_declares_exactly_the_four_entry_points():
    assert declared_functions() == ENTRY_POINTS
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_CONV_HALF_ABI_VERSION\s+1\b', text)
    assert '#include "lsq_hip.h"' in text
    assert '#include "lsq_hip_linear_half.h"' in text          # LSQ_DTYPE_* are that header's
    bits = dict(re.findall(r'\b(LSQ_CONV_HALF_[A-Z_]+)\s*=\s*(\d+)', text))
    assert bits == {'LSQ_CONV_HALF_PATCH': '1', 'LSQ_CONV_HALF_WIDE': '2', 'LSQ_CONV_HALF_UNIT_STRIDE': '4',
                    'LSQ_CONV_HALF_MANY_TAPS': '8'}
    assert (C.PATCH, C.WIDE, C.UNIT, C.MANY) == (1, 2, 4, 8)


def test_the_library_is_a_sublib_of_the_build():
    import __graft_entry__
    row = [s for s in __graft_entry__.SUBLIBS if s[0] == 'conv_half']
    assert len(row) == 1
    assert row[0][1:3] == ('conv_half_lib', 'lsq_hip_conv_half.h') and row[0][5] == 'CONV_HALF_ABI_VERSION'
    assert row[0][3] == PATTERN
    assert sorted(row[0][4]) == ENTRY_POINTS
    assert sorted(set(re.findall(r'\b(' + PATTERN + r')\s*\(', open(HEADER).read()))) == ENTRY_POINTS
    assert os.path.exists(os.path.join(ROOT, 'ml-quant_amd', 'csrc', 'conv_half', 'Makefile'))
    # no other row's regex claims the new symbols, and the new row claims none of theirs (nor a main-library name)
    for other in __graft_entry__.SUBLIBS:
        if other[0] != 'conv_half':
            assert not any(re.fullmatch(other[3], name) for name in ENTRY_POINTS), other[0]
            assert not any(re.fullmatch(PATTERN, name) for name in other[4]), other[0]
            with open(os.path.join(ROOT, 'include', other[2])) as f:
                assert not re.findall(r'\b(' + PATTERN + r')\s*\(', f.read()), other[2]
    with open(os.path.join(ROOT, 'include', 'lsq_hip.h')) as f:
        assert not re.findall(r'\b(' + PATTERN + r')\s*\(', f.read())


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.conv_half_library_path())
    assert hip.conv_half_lib().lsq_conv_half_abi_version() == hip.CONV_HALF_ABI_VERSION == 1


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm') or shutil.which('llvm-nm') or '/opt/rocm/llvm/bin/llvm-nm'
    out = subprocess.run([nm, '-D', '--defined-only', hip.conv_half_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def test_argument_errors_return_before_a_launch(hip):
    """Host buffers filled with a sentinel stand in for y and the workspace: a refused call never dereferences a pointer (x
    and the weights are garbage addresses) and leaves every byte as it was."""
    y = np.full((4 * 64 * 7 * 7,), 12345.0, dtype=np.float32)
    ws = np.full((4 * 64 * 7 * 7,), -77.0, dtype=np.float32)
    keep = y.copy(), ws.copy()
    lib = hip.conv_half_lib()
    fn, plan, wsb = lib.lsq_signw_conv2d_half, lib.lsq_signw_conv2d_half_plan, lib.lsq_signw_conv2d_half_workspace_bytes

    def geom(N=4, C=100, H=7, W=7, O=64, K=3, groups=1, pad=1, stride=1, dil=1):
        return hip.make_geom(N, C, H, W, O, K, K, (stride, stride), (pad, pad), (dil, dil), groups)

    def call(x=1 << 20, xdt=BF16, alpha=2.0, wb=1 << 21, k=1, sc=1 << 22, bias=None, g=None, yp=y.ctypes.data, ydt=F32,
             w=ws.ctypes.data, wbytes=ws.nbytes, no_geom=False):
        gp = None if no_geom else ctypes.byref(g if g is not None else geom())
        return fn(x, xdt, alpha, wb, k, sc, bias, gp, yp, ydt, w, wbytes, None)

    for xdt in (BF16, F16):
        for k in (1, 2, 8):
            for ydt in (F32, xdt):
                kw = dict(xdt=xdt, k=k, ydt=ydt)
                for name in ('x', 'wb', 'sc', 'yp'):
                    assert call(**kw, **{name: None}) == E_NULL, name
                assert call(**kw, no_geom=True) == E_NULL
                for g in (geom(N=0), geom(C=0), geom(H=-1), geom(W=0), geom(O=0), geom(K=0), geom(groups=0), geom(stride=0),
                          geom(dil=0), geom(pad=-1), geom(C=100, groups=3), geom(O=64, C=99, groups=3)):
                    assert call(**kw, g=g) == E_SHAPE
                    assert plan(ctypes.byref(g)) == E_SHAPE and wsb(ctypes.byref(g), k, ydt) == 0
                empty = geom(H=2, W=2, K=5, pad=1)                               # H + 2 p < k: no output
                assert call(**kw, g=empty) == E_SHAPE and plan(ctypes.byref(empty)) == E_SHAPE
                # N C H W >= 2^31; N O Ho Wo >= 2^31; the padded planes >= 2^31; 2^28 weight words; 65536 out-channel tiles
                for g in (geom(N=1 << 11, C=1 << 10, H=32, W=32), geom(N=1 << 10, C=1, H=1 << 10, W=1 << 10, O=4, K=1, pad=0),
                          geom(N=2, C=1, H=1, W=1, O=1, K=1, pad=1 << 15), geom(N=1, C=1 << 18, H=1, W=1, O=1 << 16, K=1, pad=0),
                          geom(N=1, C=1 << 16, H=1, W=1, O=1 << 16, K=1, pad=0, groups=1 << 16)):
                    assert call(**kw, g=g) == E_UNSUPPORTED
                    assert plan(ctypes.byref(g)) == E_UNSUPPORTED and wsb(ctypes.byref(g), k, ydt) == 0
        for k in (0, -1, 9):
            assert call(xdt=xdt, k=k) == E_UNSUPPORTED, k
        other = F16 if xdt == BF16 else BF16
        for ydt in (other, 3, -1):
            assert call(xdt=xdt, ydt=ydt) == E_UNSUPPORTED, ydt
        # a 16-bit y of two or more planes needs the workspace: NULL, misaligned, one byte short
        need = 4 * 4 * 64 * 7 * 7
        assert wsb(ctypes.byref(geom()), 2, xdt) == need == ws.nbytes
        assert call(xdt=xdt, k=2, ydt=xdt, w=None) == E_WORKSPACE
        assert call(xdt=xdt, k=2, ydt=xdt, w=ws.ctypes.data + 2) == E_WORKSPACE
        assert call(xdt=xdt, k=2, ydt=xdt, wbytes=need - 1) == E_WORKSPACE
    for xdt in (F32, 3, -1):
        assert call(xdt=xdt) == E_UNSUPPORTED and call(xdt=xdt, ydt=xdt) == E_UNSUPPORTED, xdt
    assert plan(None) == E_NULL
    assert hip.E_UNSUPPORTED == E_UNSUPPORTED
    assert all(np.array_equal(a, b) for a, b in zip(keep, (y, ws)))


def test_workspace_bytes_are_as_documented(hip):
    """4 N O Ho Wo for a 16-bit y of two or more planes (a launch holds one plane), 0 otherwise."""
    wsb = hip.conv_half_lib().lsq_signw_conv2d_half_workspace_bytes
    for c in C.CASES:
        g = _geom(hip, c)
        ho, wo = C.out_hw(c)
        assert hip.out_hw(g) == (ho, wo)
        for k in range(1, 9):
            assert wsb(ctypes.byref(g), k, F32) == 0
            for ydt in (BF16, F16):
                assert wsb(ctypes.byref(g), k, ydt) == (4 * c.N * c.O * ho * wo if k >= 2 else 0), (c.id, k)
        assert wsb(ctypes.byref(g), 0, BF16) == 0 and wsb(ctypes.byref(g), 2, 3) == 0
    assert wsb(None, 2, BF16) == 0


def test_plan_pins_every_case_to_its_kernel_and_the_table_is_complete(hip):
    plan = hip.conv_half_lib().lsq_signw_conv2d_half_plan
    seen = set()
    for c in C.CASES:
        got = plan(ctypes.byref(_geom(hip, c)))
        print(f'{c.id}: plan {got}')
        assert got == c.plan, (c.id, got, c.plan)
        assert bool(got & C.PATCH) == C.fp32_patch(c), c.id          # the patch rule is lsq_signw_conv2d's
        assert bool(got & C.WIDE) == (c.O // c.groups > 64)
        if got & C.PATCH:
            assert bool(got & C.UNIT) == (c.stride == (1, 1)) and bool(got & C.MANY) == (c.KH * c.KW > 9)
        else:
            assert not got & (C.UNIT | C.MANY)
        seen |= C.kinds(c)
    assert seen >= C.REQUIRED_KINDS, sorted(C.REQUIRED_KINDS - seen)
    assert len({c.id for c in C.CASES}) == len(C.CASES)
    # all ten kernels of a type are reached
    assert len({c.plan for c in C.CASES}) == 10
    for c in C.CASES:                               # small enough for a test of about a second
        assert c.N * c.C * c.H * c.W <= 1 << 17 and c.N * c.O * C.out_hw(c)[0] * C.out_hw(c)[1] <= 1 << 17


_im2col64 = C.im2col64      # the sum written out tap by tap in fp64 (shared with tests/test_gpu_signw_conv_cases.py)


@pytest.mark.parametrize('dt', C.DTYPES)
@pytest.mark.parametrize('cid', [c.id for c in C.CASES])
def test_reference_against_a_restatement_and_against_fp32(cid, dt):
    """The table's fp64 reference equals the sum written out tap by tap (to fp64 rounding), and a plain fp32 F.conv2d of the
    same operands stays within 1e-5 of max |y64|: the GPU test's bound is not tighter than fp32 arithmetic on these inputs."""
    c = C.BY_ID[cid]
    w, wsc, sc, b = C.weights(cid)
    assert wsc.shape == (C.planes(c.ws), c.O)
    wq = P.quantize_weight(w, c.ws, sc)
    xc = C.clamped(cid, dt)
    a = C.ALPHAS[c.alpha]
    if a >= 0:
        assert float(xc.float().abs().max()) <= C.alpha_in(a, C.DTYPES[dt]) and (xc != C.batch(cid, dt)).any()
    y64 = C.reference(cid, dt)
    assert y64.dtype == torch.float64 and tuple(y64.shape) == (c.N, c.O, *C.out_hw(c))
    scale = y64.abs().max().item()
    again = _im2col64(xc.double().numpy(), wq.double().numpy(), None if b is None else b.double().numpy(), c)
    err = np.abs(again - y64.numpy()).max()
    assert err <= 1e-12 * scale, (cid, err / scale)
    y32 = F.conv2d(xc.float(), wq, b, c.stride, c.pad, c.dil, c.groups)
    e32 = (y32.double() - y64).abs().max().item()
    print(f'{cid} {dt}: fp32 conv2d err / max|y64| = {e32 / scale:.3e}')
    assert e32 <= 1e-5 * scale, (cid, e32 / scale)


def test_python_wrapper_checks_operands_on_the_host(hip):
    n, c, h, w, o = 2, 20, 5, 6, 24
    geom = hip.make_geom(n, c, h, w, o, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    words = 9 * 1 * 32
    f = hip.signw_conv2d_half
    for dtype in (torch.bfloat16, torch.float16):
        x = torch.zeros((n, c, h, w), dtype=dtype)
        wbits = torch.zeros((2 * words,), dtype=torch.int64)
        wsc = torch.ones((2, o), dtype=torch.float32)
        bias = torch.zeros((o,), dtype=torch.float32)
        for bad in (x.float(), x.double(), x.to(torch.int16)):
            with pytest.raises(TypeError, match='bfloat16 or float16'):
                f(bad, 2.0, wbits, wsc, bias, geom)
        with pytest.raises(TypeError, match='out_dtype must be'):
            f(x, 2.0, wbits, wsc, bias, geom, out_dtype=torch.float16 if dtype == torch.bfloat16 else torch.bfloat16)
        with pytest.raises(TypeError, match='wscales must be'):
            f(x, 2.0, wbits, wsc.to(dtype), bias, geom)
        with pytest.raises(TypeError, match='bias must be'):
            f(x, 2.0, wbits, wsc, bias.to(dtype), geom)
        with pytest.raises(TypeError, match='wbits must be'):
            f(x, 2.0, wbits.int(), wsc, bias, geom)
        with pytest.raises(ValueError, match='contiguous'):
            f(x.to(memory_format=torch.channels_last), 2.0, wbits, wsc, bias, geom)
        with pytest.raises(ValueError, match='bad sizes'):
            f(x.view(n, -1), 2.0, wbits, wsc, bias, geom)
        with pytest.raises(ValueError, match='bad sizes'):
            f(x, 2.0, wbits, wsc[0], bias, geom)
        with pytest.raises(ValueError, match='geometry and x'):
            f(x[:, :10].contiguous(), 2.0, wbits, wsc, bias, geom)
        with pytest.raises(ValueError, match='do not match'):
            f(x, 2.0, wbits[:2 * words - 1], wsc, bias, geom)
        with pytest.raises(ValueError, match='do not match'):
            f(x, 2.0, wbits, wsc[:, :o - 1].contiguous(), bias, geom)
        with pytest.raises(ValueError, match='do not match'):
            f(x, 2.0, wbits, wsc, bias[:o - 1], geom)
        for b in (None, bias):                                    # CPU tensors: the kernel reads device memory only
            with pytest.raises(ValueError, match='cuda device'):
                f(x, 2.0, wbits, wsc, b, geom)


def _conv(xq, wq='ls-1', c=64, o=64, k=3, **kw):
    return QuantConv2d(xq, wq, c, o, k, {'kind': 'symmetric', 'alpha': 2}, padding=1, **kw).eval()


def test_fp_half_is_off_by_default_and_switches_the_dispatch(hip):
    assert QuantConv2d.fp_half is False and QuantConv2d.fp_half_kernel is True
    for dtype in (torch.bfloat16, torch.float16):
        x = torch.zeros((2, 64, 8, 8), dtype=dtype)
        for wq in ('ls-1', 'ls-2', 'ls-T', 'gf-3', 'gf-8'):
            m = _conv('fp', wq)
            assert not m._hip_supports_uncached(x) and not m._hip_supports(x)
            assert m._hip_supports(x.float())
            m.act_half = True                                             # the other switch does not open this path
            assert not m._hip_supports_uncached(x) and not m._hip_supports(x)
            m.fp_half = True
            assert m._hip_supports_uncached(x) and m._hip_supports(x)     # (the memo follows the switch)
            assert m._hip_supports(x.float())
            assert not m._wants_hip(x)                                    # CPU tensors never reach the kernel
            m.act_half = False
            assert m._hip_supports_uncached(x) and m._hip_supports(x)
            half_w = _conv('fp', wq).to(dtype)
            half_w.fp_half = True
            assert not half_w._hip_supports_uncached(x)
            assert not m._hip_supports_uncached(x.double()) and not m._hip_supports_uncached(x.to(torch.int16))
        many = _conv('fp', 'gf-9')
        many.fp_half = True
        assert not many._hip_supports_uncached(x)
        plain = _conv('fp', 'fp')
        plain.fp_half = True
        assert not plain._wants_hip(x)
        binary = _conv('ls-1')                                            # fp_half does not open the binary-activation path
        binary.fp_half = True
        assert not binary._hip_supports_uncached(x)
    assert QuantConv2d.fp_half is False and QuantConv2d.act_half is False


def test_the_dispatch_mirrors_the_librarys_index_limits(hip):
    """A geometry lsq_signw_conv2d_half refuses (here N O Ho Wo >= 2^31) takes the torch formulation instead of raising; the
    memo tells batch sizes apart.  (Meta tensors: only the shape is read.)"""
    m = QuantConv2d('fp', 'ls-1', 1, 4, 1, {'kind': 'identity'}).eval()
    m.fp_half = True
    small = torch.empty((2, 1, 1 << 10, 1 << 10), dtype=torch.bfloat16, device='meta')
    big = torch.empty((1 << 10, 1, 1 << 10, 1 << 10), dtype=torch.bfloat16, device='meta')
    assert hip.signw_conv2d_half_supported(m._geom_of(small, hip)) and not hip.signw_conv2d_half_supported(m._geom_of(big, hip))
    assert m._hip_supports(small) and not m._hip_supports(big) and m._hip_supports(small)
    assert not m._hip_supports_uncached(big)
    m.fp_half = False
    assert not m._hip_supports(small)
