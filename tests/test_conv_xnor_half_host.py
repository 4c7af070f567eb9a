"""The C ABI of liblsq_hip_conv_xnor_half.so on the host (no GPU): header, build row, exports, the workspace rule, the Python
wrapper's operand checks (which refuse before any library is touched), QuantConv2d's ``xnor_half`` switch, and the case table of
tests/golden/conv_xnor_half_cases.py against the kernels' eligibility and launch arithmetic."""

import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import conv_xnor_half_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_conv_xnor_half.h')
ENTRY_POINTS = ['lsq_conv_xnor_half_abi_version', 'lsq_xnor_conv2d_half', 'lsq_xnor_conv2d_half_workspace_bytes']
PATTERN = r'lsq_conv_xnor_half_[a-z0-9_]+|lsq_xnor_conv2d_half[a-z0-9_]*'


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.conv_xnor_half_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def _geom(hip, g):
    return hip.make_geom(g.N, g.C, g.H, g.W, g.O, g.k, g.k, g.stride, g.pad, g.dil, g.groups)


def test_header_declares_exactly_the_three_entry_points():
    assert declared_functions() == ENTRY_POINTS
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_CONV_XNOR_HALF_ABI_VERSION\s+1\b', text)
    assert '#include "lsq_hip.h"' in text and '#include "lsq_hip_linear_half.h"' in text          # LSQ_DTYPE_* are that header's
    # the main header and its ABI version are what they were
    main = open(os.path.join(ROOT, 'include', 'lsq_hip.h')).read()
    assert re.search(r'#define\s+LSQ_ABI_VERSION\s+12\b', main) and not re.findall(r'\b(' + PATTERN + r')\s*\(', main)


def test_the_table_row_matches_the_header():
    import __graft_entry__
    from quant import _sublibs
    row = [s for s in __graft_entry__.SUBLIBS if s[0] == 'conv_xnor_half']
    assert len(row) == 1
    assert row[0][1:3] == ('conv_xnor_half_lib', 'lsq_hip_conv_xnor_half.h') and row[0][5] == 'CONV_XNOR_HALF_ABI_VERSION'
    assert row[0][3] == PATTERN
    assert sorted(row[0][4]) == ENTRY_POINTS
    assert sorted(set(re.findall(r'\b(' + PATTERN + r')\s*\(', open(HEADER).read()))) == ENTRY_POINTS
    assert os.path.exists(os.path.join(ROOT, 'ml-quant_amd', 'csrc', 'conv_xnor_half', 'Makefile'))
    protos = _sublibs.BY_DIR['conv_xnor_half'].prototypes
    assert protos['lsq_xnor_conv2d_half_workspace_bytes'][0] is ctypes.c_size_t
    assert len(protos['lsq_xnor_conv2d_half'][1]) == 18 and protos['lsq_xnor_conv2d_half'][1][16] is ctypes.c_size_t
    for other in __graft_entry__.SUBLIBS:
        if other[0] != 'conv_xnor_half':
            assert not any(re.fullmatch(other[3], name) for name in ENTRY_POINTS), other[0]
            assert not any(re.fullmatch(PATTERN, name) for name in other[4]), other[0]


def test_the_library_builds_loads_and_exports_the_declared_entry_points(hip):
    assert hip.conv_xnor_half_lib().lsq_conv_xnor_half_abi_version() == hip.CONV_XNOR_HALF_ABI_VERSION == 1
    nm = shutil.which('nm') or shutil.which('llvm-nm') or '/opt/rocm/llvm/bin/llvm-nm'
    out = subprocess.run([nm, '-D', '--defined-only', hip.conv_xnor_half_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def test_workspace_bytes_are_as_documented(hip):
    """0 for a call of one launch -- (kx, kw) = (1, 1), (2, 1) --, 4 N O Ho Wo for several; 0 for arguments the call refuses."""
    wsb = hip.conv_xnor_half_lib().lsq_xnor_conv2d_half_workspace_bytes
    for g in C.GEOMS + (C.STREAM,):
        geom = _geom(hip, g)
        ho, wo = C.out_hw(g)
        assert hip.out_hw(geom) == (ho, wo)
        for kx, kw in ((1, 1), (2, 1)):
            assert wsb(ctypes.byref(geom), kx, kw) == 0 == C.workspace_bytes(g, kx, kw), (g.id, kx, kw)
        for kx, kw in ((2, 2), (3, 1), (3, 2), (1, 2), (8, 8)):
            assert wsb(ctypes.byref(geom), kx, kw) == 4 * g.N * g.O * ho * wo == C.workspace_bytes(g, kx, kw), (g.id, kx, kw)
        for kx, kw in ((0, 2), (3, 0), (9, 1), (3, 9)):
            assert wsb(ctypes.byref(geom), kx, kw) == 0
    assert wsb(None, 3, 2) == 0
    g = C.GEOMS[0]
    assert wsb(ctypes.byref(hip.make_geom(g.N, g.C, 2, 2, g.O, 5, 5, (1, 1), (1, 1), (1, 1), 1)), 3, 2) == 0      # no output


def test_refusals_of_the_entry_point_write_nothing(hip):
    """Host buffers with a sentinel stand in for y and the workspace (the other pointers are garbage addresses): a refused call
    dereferences nothing and leaves every byte."""
    import numpy as np
    g = C.BY_ID['m128_s2']
    geom = _geom(hip, g)
    y = np.full((C.outputs(g),), 0x5A5A, dtype=np.uint16)
    ws = np.full((C.outputs(g),), -77.0, dtype=np.float32)
    keep = y.copy(), ws.copy()
    fn = hip.conv_xnor_half_lib().lsq_xnor_conv2d_half

    def call(x=1 << 20, kx=3, xs=1 << 21, wb=1 << 22, wsum=1 << 23, kw=2, wsc=1 << 24, gp=geom, act=0, slope=None, dtype=1,
             yp=y.ctypes.data, w=ws.ctypes.data, wbytes=ws.nbytes):
        return fn(x, kx, xs, wb, wsum, kw, wsc, None, None if gp is None else ctypes.byref(gp), act, slope, None, None, dtype, yp,
                  w, wbytes, None)

    for dtype in (1, 2):
        for name in ('x', 'xs', 'wb', 'wsum', 'wsc', 'yp'):
            assert call(dtype=dtype, **{name: None}) == -1, name                        # LSQ_E_NULL
        assert call(dtype=dtype, gp=None) == -1
        assert call(dtype=dtype, kx=0) == -3 and call(dtype=dtype, kw=9) == -3          # LSQ_E_SCHEME
        assert call(dtype=dtype, act=2) == -3                                           # (PReLU without slopes)
        assert call(dtype=dtype, gp=hip.make_geom(g.N, g.C, 2, 2, g.O, 5, 5, (1, 1), (1, 1), (1, 1), 1)) == -2      # LSQ_E_SHAPE
        assert call(dtype=dtype, w=None) == -5 and call(dtype=dtype, wbytes=ws.nbytes - 1) == -5      # LSQ_E_WORKSPACE
        assert call(dtype=dtype, w=ws.ctypes.data + 2) == -5
    for dtype in (0, 3, -1):
        assert call(dtype=dtype) == -6 and call(dtype=dtype, kx=2, kw=1, w=None, wbytes=0) == -6      # LSQ_E_UNSUPPORTED
    assert all(np.array_equal(a, b) for a, b in zip(keep, (y, ws)))


def _wrapper_operands(dtype):
    g = C.BY_ID['p24_o20']
    ho, wo = C.out_hw(g)
    words = g.N * 1 * (g.H + 2) * (g.W + 2)
    return g, dict(planes=torch.zeros((2 * words,), dtype=torch.int64), k=2, xscales=torch.ones((2, g.N)),
                   wbits=torch.zeros((9 * 1 * 32,), dtype=torch.int64), wsum=torch.zeros((1, g.O, 9), dtype=torch.int32),
                   wscales=torch.ones((1, g.O)), bias=torch.zeros((g.O,))), torch.zeros((g.N, g.O, ho, wo), dtype=dtype)


def test_python_wrapper_refuses_before_touching_a_library(monkeypatch):
    """Wrong residual dtype or shape, non-contiguous operands, CPU tensors: raised by the host checks -- neither library's loader is
    reached (both are replaced by one that fails the test)."""
    from quant import _hip

    def loaded(*a, **k):
        raise AssertionError('an operand check let the call through to a library')

    monkeypatch.setattr(_hip, 'conv_xnor_half_lib', loaded)
    monkeypatch.setattr(_hip, 'lib', loaded)
    f = _hip.xnor_conv2d_half
    for dtype in (torch.bfloat16, torch.float16):
        other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
        g, ops, res = _wrapper_operands(dtype)
        geom = _geom(_hip, g)
        args = lambda **kw: {**ops, 'geom': geom, 'dtype': dtype, **kw}
        with pytest.raises(TypeError, match='dtype must be'):
            f(**args(dtype=torch.float32))
        for bad in (res.float(), res.to(other)):
            with pytest.raises(TypeError, match='res_pre must be'):
                f(**args(res_pre=bad))
            with pytest.raises(TypeError, match='res_post must be'):
                f(**args(res_post=bad))
        with pytest.raises(TypeError, match='xscales must be'):
            f(**args(xscales=ops['xscales'].to(dtype)))
        with pytest.raises(TypeError, match='bias must be'):
            f(**args(bias=ops['bias'].to(dtype)))
        with pytest.raises(TypeError, match='planes must be'):
            f(**args(planes=ops['planes'].int()))
        with pytest.raises(ValueError, match='shape of y'):
            f(**args(res_pre=res[:, :, :-1].contiguous()))
        with pytest.raises(ValueError, match='shape of y'):
            f(**args(res_post=res.view(-1)))
        with pytest.raises(ValueError, match='contiguous'):
            f(**args(res_pre=res.to(memory_format=torch.channels_last)))
        with pytest.raises(ValueError, match='contiguous'):
            f(**args(res_post=res.transpose(2, 3).contiguous().transpose(2, 3)))
        with pytest.raises(ValueError, match='do not match'):
            f(**args(xscales=ops['xscales'][:1].contiguous()))
        with pytest.raises(ValueError, match='do not match'):
            f(**args(wscales=ops['wscales'][:, :-1].contiguous()))
        with pytest.raises(ValueError, match='prelu'):
            f(**args(prelu=torch.ones((3,))))
        for kw in ({}, {'res_pre': res}, {'res_post': res, 'relu': True}):              # CPU tensors: the kernel reads device memory
            with pytest.raises(ValueError, match='cuda device'):
                f(**args(**kw))


def test_a_default_module_never_loads_the_library():
    """In a fresh interpreter: importing the package and running a default QuantConv2d (eval and train, fp32 and bf16, on the CPU)
    leaves the entry of the handle table empty; the switch is off on the class."""
    code = '\n'.join([
        'import torch',
        'from quant import _hip',
        'from quant.binary.binary_conv import QuantConv2d',
        'assert QuantConv2d.xnor_half is False',
        "m = QuantConv2d('ls-1', 'ls-1', 8, 8, 3, {'kind': 'symmetric', 'alpha': 2}, padding=1)",
        'x = torch.randn(2, 8, 5, 5)',
        'm.eval()(x); m.train()(x).sum().backward()',
        'm.eval().fused_forward(x, relu=True, res_pre=torch.zeros(2, 8, 5, 5))',
        'm.xnor_half = True',
        'm.fused_forward(x.bfloat16().float(), relu=True)',
        "assert 'conv_xnor_half' not in _hip._handles, list(_hip._handles)",
        "print('not loaded')"])
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, 'ml-quant_amd')]))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'not loaded' in out.stdout, out.stderr[-2000:]


def test_the_switch_does_not_change_the_dispatch(hip):
    from quant.binary.binary_conv import QuantConv2d
    assert QuantConv2d.xnor_half is False and QuantConv2d.act_half is False and QuantConv2d.hip_train_half is False
    m = QuantConv2d('ls-1', 'ls-1', 64, 64, 3, {'kind': 'symmetric', 'alpha': 2}, padding=1).eval()
    x = torch.zeros((2, 64, 8, 8), dtype=torch.bfloat16)
    m.xnor_half = True                                   # a switch of its own: it opens no path
    assert not m._hip_supports_uncached(x) and not m._wants_hip(x)
    m.act_half = True
    assert m._hip_supports_uncached(x) and not m._wants_hip(x)          # (CPU tensors never reach the kernels)
    res = torch.zeros((2, 64, 8, 8), dtype=torch.bfloat16)
    assert not m._half_epilogue_fits(x, res, None, None)                # CPU residuals
    assert not m._half_epilogue_fits(x.float(), None, None, None)


def test_the_case_table_stays_inside_its_limits():
    ids = [g.id for g in C.GEOMS]
    assert len(set(ids)) == len(ids) == 10 and len(C.MFMA) == 6 and len(C.POPCOUNT) == 4
    for g in C.GEOMS:
        assert g.N * g.C * g.H * g.W <= C.MAX_ELEMENTS and C.outputs(g) <= C.MAX_ELEMENTS, g.id
        assert min(C.out_hw(g)) >= 1
    assert all(C.mfma_eligible(g, 1) and C.mfma_eligible(g, 2) for g in C.MFMA)
    assert not any(C.mfma_eligible(g) for g in C.POPCOUNT)
    assert C.PLANES == ((1, 1), (2, 1), (3, 2)) and [C.launches(*p) for p in C.PLANES] == [1, 1, 4]
    assert C.EPILOGUE_PLANES == ((2, 1), (2, 2)) and set(C.EPILOGUE_GEOMS) <= set(ids) and len(C.EPILOGUES) == 5
    # the shapes the table names: a 3-lane tail, less than one tile, three out-channel tiles
    tail, small, o96 = C.BY_ID['m64_tail'], C.BY_ID['m512_small'], C.BY_ID['m256_o96']
    assert C.out_hw(tail) == (5, 7) and tail.N * 35 == 32 + 3
    assert small.N * C.out_hw(small)[0] * C.out_hw(small)[1] < 32 and o96.O // 32 == 3
    assert C.out_hw(C.BY_ID['m64_nopad']) == (4, 4) and C.BY_ID['m64_nopad'].pad == (0, 0)
    # the multi-tile case: more pixel tiles than waves that stride over them, so some waves take a second tile and request the
    # residuals of a tile that is not the next one in memory
    tiles, gx, waves = C.mfma_launch(C.BY_ID[C.MULTI_TILE])
    assert (tiles, gx, waves) == (196, 16, 192) and waves < tiles < 2 * waves
    for g in C.MFMA:
        if g.id != C.MULTI_TILE:
            t, _, w = C.mfma_launch(g)
            assert t <= w, g.id
    # popcount shapes: C not a multiple of 64, O not a multiple of 16, groups, dilation, a 7x7 kernel
    p = C.BY_ID['p24_o20']
    assert p.C % 64 and p.O % 16 and C.BY_ID['pgroups'].groups == 2 and C.BY_ID['pgroups'].dil == (2, 1) and C.BY_ID['p7x7'].k == 7
    # the non-temporal case: residual + output in 16-bit exceed the Infinity Cache, and with fewer samples they would not
    s = C.STREAM
    assert 2 * 2 * C.outputs(s) > C.INFINITY_CACHE_BYTES >= 2 * 2 * C.outputs(s._replace(N=s.N - 2))
    assert C.mfma_eligible(s, 2) and C.outputs(s) < 1 << 30
