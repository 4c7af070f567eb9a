"""The C ABI of liblsq_hip_conv_act_bn_half.so on the host (no GPU): header, exports, the table row and its prototype,
argument errors returned before any launch, the Python wrapper's operand checks, the fixtures' folded tensor, and
QuantConv2d's ``act_half_bn_fold`` switch in the dispatch."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import conv_act_bn_half_cases as B
from quant import _sublibs
from quant.binary.binary_conv import QuantConv2d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_conv_act_bn_half.h')
E_NULL, E_SHAPE, E_SCHEME, E_UNSUPPORTED = -1, -2, -3, -6
F32, BF16, F16 = 0, 1, 2
LS1, LS2, LST, GF = 1, 2, 3, 4
ENTRY_POINTS = ['lsq_act_quant_bn_half', 'lsq_conv_act_bn_half_abi_version']
PATTERN = r'lsq_conv_act_bn_half_[a-z0-9_]+|lsq_act_quant_bn_half[a-z0-9_]*'


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.conv_act_bn_half_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def test_header_declares_exactly_the_two_entry_points():
    assert declared_functions() == ENTRY_POINTS
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_CONV_ACT_BN_HALF_ABI_VERSION\s+1\b', text)
    assert '#include "lsq_hip.h"' in text
    assert '#include "lsq_hip_linear_half.h"' in text          # LSQ_DTYPE_* are that header's
    # the header that said the fold was impossible now points here
    assert 'lsq_hip_conv_act_bn_half.h' in open(os.path.join(ROOT, 'include', 'lsq_hip_conv_act_half.h')).read()


def test_the_table_row_and_its_prototype():
    row = _sublibs.BY_DIR['conv_act_bn_half']
    assert (row.header, row.version_symbol, row.version) == ('lsq_hip_conv_act_bn_half.h', 'lsq_conv_act_bn_half_abi_version', 1)
    assert row.pattern == PATTERN and _sublibs.soname(row) == 'liblsq_hip_conv_act_bn_half.so'
    assert sorted(row.prototypes) == ENTRY_POINTS
    restype, argtypes = row.prototypes['lsq_act_quant_bn_half']
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert restype is i32 and len(argtypes) == 14
    assert argtypes == [vp, i32, vp, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp]
    # lsq_act_quant_half's prototype with the two arrays in front of `forced`
    base = _sublibs.BY_DIR['conv_act_half'].prototypes['lsq_act_quant_half'][1]
    assert argtypes == base[:7] + [vp, vp] + base[7:]


def test_the_library_is_a_sublib_of_the_build():
    import __graft_entry__
    row = [s for s in __graft_entry__.SUBLIBS if s[0] == 'conv_act_bn_half']
    assert len(row) == 1
    assert row[0][1:3] == ('conv_act_bn_half_lib', 'lsq_hip_conv_act_bn_half.h') and row[0][5] == 'CONV_ACT_BN_HALF_ABI_VERSION'
    assert row[0][3] == PATTERN
    assert sorted(row[0][4]) == ENTRY_POINTS
    assert sorted(set(re.findall(r'\b(' + row[0][3] + r')\s*\(', open(HEADER).read()))) == ENTRY_POINTS
    assert os.path.exists(os.path.join(ROOT, 'ml-quant_amd', 'csrc', 'conv_act_bn_half', 'Makefile'))
    # no other row's regex claims the new symbols, and the new row claims none of theirs
    for other in __graft_entry__.SUBLIBS:
        if other[0] != 'conv_act_bn_half':
            assert not any(re.fullmatch(other[3], name) for name in ENTRY_POINTS), other[0]
            assert not any(re.fullmatch(row[0][3], name) for name in other[4]), other[0]


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.conv_act_bn_half_library_path())
    assert hip.conv_act_bn_half_lib().lsq_conv_act_bn_half_abi_version() == hip.CONV_ACT_BN_HALF_ABI_VERSION == 1


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm') or shutil.which('llvm-nm') or '/opt/rocm/llvm/bin/llvm-nm'
    out = subprocess.run([nm, '-D', '--defined-only', hip.conv_act_bn_half_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def test_argument_errors_return_before_a_launch(hip):
    """Host buffers filled with a sentinel stand in for planes, scales and status: a refused call never dereferences a
    pointer (x, pre_scale and pre_shift are garbage) and leaves every byte as it was.  Every refusal of lsq_act_quant_half,
    with both pre-arrays and with neither; one pre-array alone is LSQ_E_NULL."""
    n = 4
    planes = np.full((8 * n * 2 * 9 * 9,), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    scales = np.full((8, n), 12345.0, dtype=np.float32)
    status = np.full((n,), -77, dtype=np.int32)
    forced = np.full((8, n), 0.5, dtype=np.float32)
    keep = planes.copy(), scales.copy(), status.copy()
    fn = hip.conv_act_bn_half_lib().lsq_act_quant_bn_half
    garbage = (3 << 20, 5 << 20)

    def geom(N=n, C=100, H=7, W=7, groups=1):
        return hip.make_geom(N, C, H, W, 64, 3, 3, (1, 1), (1, 1), (1, 1), groups)

    def call(x=1 << 20, xdt=BF16, g=None, scheme=LS1, k=1, skip=3, alpha=2.0, pre=garbage, f=None, p=planes.ctypes.data,
             s=scales.ctypes.data, t=status.ctypes.data, no_geom=False):
        gp = None if no_geom else ctypes.byref(g if g is not None else geom())
        return fn(x, xdt, gp, scheme, k, skip, alpha, pre[0], pre[1], f, p, s, t, None)

    good_k = {LS1: 1, LS2: 2, LST: 2, GF: 3}
    for pre in (garbage, (None, None)):
        for xdt in (BF16, F16):
            for scheme, k in good_k.items():
                for given in (None, forced.ctypes.data):
                    kw = dict(xdt=xdt, scheme=scheme, k=k, f=given, pre=pre)
                    for name in ('x', 'p', 's'):
                        assert call(**kw, **{name: None}) == E_NULL, name
                    assert call(**kw, no_geom=True) == E_NULL
                    for g in (geom(N=0), geom(C=0), geom(H=-1), geom(W=0), geom(groups=0), geom(C=100, groups=3)):
                        assert call(**kw, g=g) == E_SHAPE
                    for skip in (0, -3):
                        assert call(**kw, skip=skip) == E_SHAPE, skip
                    # M >= 2^31
                    assert call(**kw, g=geom(N=1, C=1 << 11, H=1 << 10, W=1 << 10)) == E_UNSUPPORTED
            for scheme, k in ((0, 1), (5, 1), (-1, 1), (LS1, 2), (LS1, 0), (LS2, 1), (LS2, 3), (LST, 1), (GF, 0), (GF, 9), (GF, -1)):
                assert call(xdt=xdt, scheme=scheme, k=k, pre=pre) == E_SCHEME, (scheme, k)
        for xdt in (F32, 3, -1):
            assert call(xdt=xdt, pre=pre) == E_UNSUPPORTED and call(xdt=xdt, scheme=LST, k=2, t=None, pre=pre) == E_UNSUPPORTED, xdt
    # exactly one of the two arrays: refused whatever the rest of the call is
    for pre in ((garbage[0], None), (None, garbage[1])):
        for xdt in (BF16, F16):
            for scheme, k in good_k.items():
                for given in (None, forced.ctypes.data):
                    assert call(xdt=xdt, scheme=scheme, k=k, f=given, pre=pre) == E_NULL
        assert call(pre=pre, xdt=F32) == E_NULL and call(pre=pre, skip=0) == E_NULL      # (whatever else is wrong with the call)
    assert all(np.array_equal(a, b) for a, b in zip(keep, (planes, scales, status)))


def test_python_wrapper_checks_operands_on_the_host(hip):
    n, c, h, w = 4, 100, 5, 6
    geom = hip.make_geom(n, c, h, w, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    words = n * 2 * 7 * 8
    q = hip.act_quant_bn_half
    pre = (torch.ones(c), torch.zeros(c))
    for dtype in (torch.bfloat16, torch.float16):
        x = torch.zeros((n, c, h, w), dtype=dtype)
        planes = torch.zeros((2 * words,), dtype=torch.int64)
        scales = torch.zeros((2, n), dtype=torch.float32)
        status = torch.zeros((n,), dtype=torch.int32)
        for bad in (x.float(), x.double(), x.to(torch.int16)):
            with pytest.raises(TypeError, match='bfloat16 or float16'):
                q(bad, geom, LS2, 2, 3, 2.0, planes, scales, None, pre)
        with pytest.raises(TypeError, match='planes must be'):
            q(x, geom, LS2, 2, 3, 2.0, planes.int(), scales, None, pre)
        with pytest.raises(TypeError, match='scales must be'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales.to(dtype), None, pre)
        with pytest.raises(TypeError, match='forced must be'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, scales.double(), pre)
        with pytest.raises(TypeError, match='pre_scale must be'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, None, (pre[0].to(dtype), pre[1]))
        with pytest.raises(TypeError, match='pre_shift must be'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, None, (pre[0], pre[1].double()))
        with pytest.raises(TypeError, match='status must be'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, None, pre, status.long())
        with pytest.raises(ValueError, match='contiguous'):
            q(x.to(memory_format=torch.channels_last), geom, LS2, 2, 3, 2.0, planes, scales, None, pre)
        with pytest.raises(ValueError, match='contiguous'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, None, (torch.ones(2 * c)[::2], pre[1]))
        with pytest.raises(ValueError, match='bad sizes'):
            q(x.view(n, -1), geom, LS2, 2, 3, 2.0, planes, scales, None, pre)
        with pytest.raises(ValueError, match='bad sizes'):
            q(x, geom, LST, 2, 0, 2.0, planes, scales, None, pre)
        with pytest.raises(ValueError, match='do not match'):
            q(x[:, :50].contiguous(), geom, LS2, 2, 3, 2.0, planes, scales, None, pre)
        with pytest.raises(ValueError, match='do not match'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, None, (pre[0][:c - 1], pre[1]))
        with pytest.raises(ValueError, match='do not match'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, None, (pre[0], torch.zeros(c + 1)))
        with pytest.raises(ValueError, match='do not match'):
            q(x, geom, LS2, 2, 3, 2.0, planes[:2 * words - 1], scales, None, pre)
        with pytest.raises(ValueError, match='do not match'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales[:1], None, pre)
        with pytest.raises(ValueError, match='do not match'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, scales[:1], pre)
        with pytest.raises(ValueError, match='do not match'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, None, pre, status[:n - 1])
        for t in (None, status):                                  # CPU tensors: the kernel reads device memory only
            with pytest.raises(ValueError, match='cuda device'):
                q(x, geom, LST, 2, 3, 2.0, planes, scales, None, pre, t)


@pytest.mark.parametrize('dt', B.DTYPES)
def test_the_parameter_sets_are_what_they_say(dt):
    """Mixed signs and ranges; the identity; the edge set's constant channel and its channel of subnormals with one exact
    zero; fp16's overflow channel gives +-inf, and nothing else does."""
    dtype = B.DTYPES[dt]
    for gi in (3, 4, 5):
        c = B.GEOMS[gi][0]
        x = B.batch(gi, dt)
        s, b = B.params(gi, dt, 'mixed')
        assert s.shape == b.shape == (c,) and s.dtype == b.dtype == torch.float32
        assert (s > 0).any() and (s < 0).any() and (s.abs() >= 0.25).all() and (s.abs() <= 2).all() and (b.abs() <= 1).all()
        assert torch.isfinite(B.folded_batch(gi, dt, 'mixed').float()).all()
        one, zero = B.params(gi, dt, 'identity')
        assert torch.equal(B.folded(x, one, zero).view(torch.int16), (x.float() + 0.0).to(dtype).view(torch.int16))
        s, b = B.params(gi, dt, 'edges')
        t = B.folded_batch(gi, dt, 'edges')
        assert s[0] == 0 and (t[:, 0].float() == b[0].to(dtype).float()).all()
        sub = t[:, 1].float().abs()
        assert t[0, 1, 0, 0] == 0 and (sub < torch.finfo(dtype).tiny).all() and (sub > 0).sum() > sub.numel() // 2
        if dt == 'fp16':
            t = B.folded_batch(gi, dt, 'overflow').float()
            assert torch.isinf(t[:, -1]).any() and torch.isfinite(t[:, :-1]).all() and not torch.isnan(t).any()
            assert (t[:, -1] == float('inf')).any() and (t[:, -1] == float('-inf')).any()


def _conv(xq, **kw):
    return QuantConv2d(xq, 'ls-1', 64, 64, 3, {'kind': 'symmetric', 'alpha': 2}, padding=1, **kw).eval()


def test_the_fold_is_off_by_default_and_never_taken_on_the_cpu():
    assert QuantConv2d.act_half_bn_fold is False
    bn = torch.nn.BatchNorm2d(64).eval()
    for dtype in (torch.bfloat16, torch.float16):
        x = torch.zeros((2, 64, 8, 8), dtype=dtype)
        for xq in ('ls-1', 'ls-2', 'fp'):
            m = _conv(xq)
            assert not m._folds_half_bn(x, bn)
            m.act_half = m.xnor_half = m.act_half_bn_fold = True
            assert not m._folds_half_bn(x, bn)                     # a CPU tensor never reaches the kernel
    assert QuantConv2d.act_half_bn_fold is False
