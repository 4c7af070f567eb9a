"""The C ABI of liblsq_hip_conv_act_half.so on the host (no GPU): header, exports, argument errors returned before any launch,
the Python wrapper's operand checks, the CPU packer of the GPU tests against the layout definition, and QuantConv2d's
``act_half`` switch in the dispatch."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import conv_act_half_cases as C
from quant.binary.binary_conv import QuantConv2d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_conv_act_half.h')
E_NULL, E_SHAPE, E_SCHEME, E_UNSUPPORTED = -1, -2, -3, -6
F32, BF16, F16 = 0, 1, 2
LS1, LS2, LST, GF = 1, 2, 3, 4
ENTRY_POINTS = ['lsq_act_quant_half', 'lsq_conv_act_half_abi_version']


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.conv_act_half_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def test_header_declares_exactly_the_two_entry_points():
    assert declared_functions() == ENTRY_POINTS
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_CONV_ACT_HALF_ABI_VERSION\s+1\b', text)
    assert '#include "lsq_hip.h"' in text
    assert '#include "lsq_hip_linear_half.h"' in text          # LSQ_DTYPE_* are that header's


def test_the_library_is_a_sublib_of_the_build():
    import __graft_entry__
    row = [s for s in __graft_entry__.SUBLIBS if s[0] == 'conv_act_half']
    assert len(row) == 1
    assert row[0][1:3] == ('conv_act_half_lib', 'lsq_hip_conv_act_half.h') and row[0][5] == 'CONV_ACT_HALF_ABI_VERSION'
    assert row[0][3] == r'lsq_conv_act_half_[a-z0-9_]+|lsq_act_quant_half[a-z0-9_]*'
    assert sorted(row[0][4]) == ENTRY_POINTS
    assert sorted(set(re.findall(r'\b(' + row[0][3] + r')\s*\(', open(HEADER).read()))) == ENTRY_POINTS
    assert os.path.exists(os.path.join(ROOT, 'ml-quant_amd', 'csrc', 'conv_act_half', 'Makefile'))
    # no other row's regex claims the new symbols, and the new row claims none of theirs
    for other in __graft_entry__.SUBLIBS:
        if other[0] != 'conv_act_half':
            assert not any(re.fullmatch(other[3], name) for name in ENTRY_POINTS), other[0]
            assert not any(re.fullmatch(row[0][3], name) for name in other[4]), other[0]


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.conv_act_half_library_path())
    assert hip.conv_act_half_lib().lsq_conv_act_half_abi_version() == hip.CONV_ACT_HALF_ABI_VERSION == 1


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm') or shutil.which('llvm-nm') or '/opt/rocm/llvm/bin/llvm-nm'
    out = subprocess.run([nm, '-D', '--defined-only', hip.conv_act_half_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def test_argument_errors_return_before_a_launch(hip):
    """Host buffers filled with a sentinel stand in for planes, scales and status: a refused call never dereferences a
    pointer (x is garbage) and leaves every byte as it was."""
    n = 4
    planes = np.full((8 * n * 2 * 9 * 9,), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    scales = np.full((8, n), 12345.0, dtype=np.float32)
    status = np.full((n,), -77, dtype=np.int32)
    forced = np.full((8, n), 0.5, dtype=np.float32)
    keep = planes.copy(), scales.copy(), status.copy()
    fn = hip.conv_act_half_lib().lsq_act_quant_half

    def geom(N=n, C=100, H=7, W=7, groups=1):
        return hip.make_geom(N, C, H, W, 64, 3, 3, (1, 1), (1, 1), (1, 1), groups)

    def call(x=1 << 20, xdt=BF16, g=None, scheme=LS1, k=1, skip=3, alpha=2.0, f=None, p=planes.ctypes.data,
             s=scales.ctypes.data, t=status.ctypes.data, no_geom=False):
        gp = None if no_geom else ctypes.byref(g if g is not None else geom())
        return fn(x, xdt, gp, scheme, k, skip, alpha, f, p, s, t, None)

    good_k = {LS1: 1, LS2: 2, LST: 2, GF: 3}
    for xdt in (BF16, F16):
        for scheme, k in good_k.items():
            for given in (None, forced.ctypes.data):
                kw = dict(xdt=xdt, scheme=scheme, k=k, f=given)
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
            assert call(xdt=xdt, scheme=scheme, k=k) == E_SCHEME, (scheme, k)
    for xdt in (F32, 3, -1):
        assert call(xdt=xdt) == E_UNSUPPORTED and call(xdt=xdt, scheme=LST, k=2, t=None) == E_UNSUPPORTED, xdt
    assert hip.E_UNSUPPORTED == E_UNSUPPORTED
    assert all(np.array_equal(a, b) for a, b in zip(keep, (planes, scales, status)))


def test_python_wrapper_checks_operands_on_the_host(hip):
    n, c, h, w = 4, 100, 5, 6
    geom = hip.make_geom(n, c, h, w, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    words = n * 2 * 7 * 8
    q = hip.act_quant_half
    for dtype in (torch.bfloat16, torch.float16):
        x = torch.zeros((n, c, h, w), dtype=dtype)
        planes = torch.zeros((2 * words,), dtype=torch.int64)
        scales = torch.zeros((2, n), dtype=torch.float32)
        status = torch.zeros((n,), dtype=torch.int32)
        for bad in (x.float(), x.double(), x.to(torch.int16)):
            with pytest.raises(TypeError, match='bfloat16 or float16'):
                q(bad, geom, LS2, 2, 3, 2.0, planes, scales)
        with pytest.raises(TypeError, match='planes must be'):
            q(x, geom, LS2, 2, 3, 2.0, planes.int(), scales)
        with pytest.raises(TypeError, match='scales must be'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales.to(dtype))
        with pytest.raises(TypeError, match='forced must be'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, scales.double())
        with pytest.raises(TypeError, match='status must be'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, None, status.long())
        with pytest.raises(ValueError, match='contiguous'):
            q(x.to(memory_format=torch.channels_last), geom, LS2, 2, 3, 2.0, planes, scales)
        with pytest.raises(ValueError, match='bad sizes'):
            q(x.view(n, -1), geom, LS2, 2, 3, 2.0, planes, scales)
        with pytest.raises(ValueError, match='bad sizes'):
            q(x, geom, LST, 2, 0, 2.0, planes, scales)
        with pytest.raises(ValueError, match='do not match'):
            q(x[:, :50].contiguous(), geom, LS2, 2, 3, 2.0, planes, scales)
        with pytest.raises(ValueError, match='do not match'):
            q(x, geom, LS2, 2, 3, 2.0, planes[:2 * words - 1], scales)
        with pytest.raises(ValueError, match='do not match'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales[:1])
        with pytest.raises(ValueError, match='do not match'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, scales[:1])
        with pytest.raises(ValueError, match='do not match'):
            q(x, geom, LS2, 2, 3, 2.0, planes, scales, None, status[:n - 1])
        for t in (None, status):                                  # CPU tensors: the kernel reads device memory only
            with pytest.raises(ValueError, match='cuda device'):
                q(x, geom, LST, 2, 3, 2.0, planes, scales, None, t)


def _pack_ref(bits, groups, pad):
    """The layout definition of include/lsq_hip.h, word by word: bool [N, C, H, W] -> uint64 [N, Gt, H + 2 ph, W + 2 pw]."""
    bits = np.asarray(bits, dtype=bool)
    n, c, h, w = bits.shape
    cg = c // groups
    gg = (cg + 63) // 64
    out = np.zeros((n, groups * gg, h + 2 * pad[0], w + 2 * pad[1]), dtype=np.uint64)
    for grp in range(groups):
        for j in range(gg):
            word = np.zeros((n, h, w), dtype=np.uint64)
            for b in range(min(64, cg - 64 * j)):
                word |= bits[:, grp * cg + 64 * j + b].astype(np.uint64) << np.uint64(b)
            out[:, grp * gg + j, pad[0]:pad[0] + h, pad[1]:pad[1] + w] = word
    return out


@pytest.mark.parametrize('gi', (1, 4, 5, 6))
def test_the_cpu_packer_equals_the_layout_definition(gi):
    """Geometries 2, 5, 6 and 7: a partial word, a second word of one bit, two groups with unequal padding, depthwise."""
    c, h, w, groups, pad = C.GEOMS[gi]
    x = C.batch(gi, 'bf16').float()
    scales = torch.tensor([[0.9], [0.4]]).expand(2, x.shape[0]).contiguous()
    bits, _ = C.chain(x, -1.0, scales)
    got = C.pack(bits.numpy(), groups, pad)
    assert got.shape == (2, x.shape[0], *C.plane_shape(gi, x.shape[0]))
    for q in range(2):
        assert np.array_equal(got[q], _pack_ref(bits[q].numpy(), groups, pad))
    assert 0 < bits.float().mean() < 1


def _conv(xq, wq='ls-1', c=64, o=64, k=3, **kw):
    return QuantConv2d(xq, wq, c, o, k, {'kind': 'symmetric', 'alpha': 2}, padding=1, **kw).eval()


def test_act_half_is_off_by_default_and_switches_the_dispatch():
    assert QuantConv2d.act_half is False and QuantConv2d.act_half_kernel is True and QuantConv2d.act_half_solve is True
    for dtype in (torch.bfloat16, torch.float16):
        x = torch.zeros((2, 64, 8, 8), dtype=dtype)
        for xq in ('ls-1', 'ls-2', 'ls-T', 'gf-3'):
            m = _conv(xq)
            assert not m._hip_supports_uncached(x) and not m._hip_supports(x)
            assert m._hip_supports(x.float())
            m.act_half = True
            assert m._hip_supports_uncached(x) and m._hip_supports(x)     # (the memo follows the switch)
            assert m._hip_supports(x.float())
            assert not m._wants_hip(x)                                    # CPU tensors never reach the kernel
            # every other limit stays: 16-bit weights, fp activations, the plane count, the kernel size, other types
            on = dict(act_half=True)
            half_w = _conv(xq).to(dtype)
            half_w.act_half = True
            assert not half_w._hip_supports_uncached(x)
            big = _conv(xq, k=9)
            big.__dict__.update(on)
            assert not big._hip_supports_uncached(x)
            assert not m._hip_supports_uncached(x.double()) and not m._hip_supports_uncached(x.to(torch.int16))
        fp = _conv('fp')
        fp.act_half = True
        assert not fp._hip_supports_uncached(x) and fp._hip_supports_uncached(x.float())
        many = _conv('gf-9')
        many.act_half = True
        assert not many._hip_supports_uncached(x)
    assert QuantConv2d.act_half is False
