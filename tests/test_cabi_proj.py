"""lsq_xnor_conv2d_proj through the raw C ABI (include/lsq_hip_conv_proj.h, liblsq_hip_conv_proj.so): the library exports
what its header declares, and every documented refusal returns its code before any launch and before any pointer is read --
so the host tests pass made-up addresses; the GPU test repeats them on real buffers and checks that y stays untouched."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch  # noqa: F401  (its HIP runtime must be the one the libraries bind to)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_conv_proj.h')
E_NULL, E_SHAPE, E_SCHEME, E_UNSUPPORTED = -1, -2, -3, -6
FAKE = 0x1000


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not (_hip.available() and os.path.exists(_hip.conv_proj_library_path())):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def test_library_exports_what_the_header_declares(hip):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))
    assert declared == ['lsq_conv_proj_abi_version', 'lsq_xnor_conv2d_proj']
    lib = hip.conv_proj_lib()
    assert lib.lsq_conv_proj_abi_version() == hip.CONV_PROJ_ABI_VERSION == 1
    nm = shutil.which('nm')
    if nm is not None:
        out = subprocess.run([nm, '-D', '--defined-only', hip.conv_proj_library_path()], capture_output=True, text=True, check=True).stdout
        exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
        assert exported == declared


def _call(hip, y=FAKE, ptrs=FAKE, n=2, c=64, hw=(12, 12), stride=2, o=128, kx=2, kw_planes=1, kernel=3, groups=1, res_pre=None,
          res_post=None, proj=True, px=FAKE, pw=FAKE, cp=64, phw=(12, 12), pstride=2, post=1):
    from quant import _sublibs
    g = hip.make_geom(n, c, hw[0], hw[1], o, kernel, kernel, (stride, stride), (kernel // 2, kernel // 2), (1, 1), groups)
    pd = _sublibs.Proj(px, pw, None, cp, phw[0], phw[1], pstride, post)
    return hip.conv_proj_lib().lsq_xnor_conv2d_proj(ptrs, kx, ptrs, ptrs, ptrs, kw_planes, ptrs, None, ctypes.byref(g), 0, None,
                                                    res_pre, res_post, ctypes.byref(pd) if proj else None, y, None)


def _refusals(hip, **kw):
    """Every refusal of the header, with the code it documents."""
    assert _call(hip, proj=False, **kw) == E_NULL
    assert _call(hip, px=None, **kw) == E_NULL and _call(hip, pw=None, **kw) == E_NULL
    assert _call(hip, phw=(13, 12), **kw) == E_SHAPE                  # (13 - 1) / 2 + 1 = 7 != Ho = 6
    assert _call(hip, phw=(12, 10), **kw) == E_SHAPE                  # (10 - 1) / 2 + 1 = 5 != Wo = 6
    assert _call(hip, pstride=1, **kw) == E_SHAPE and _call(hip, pstride=0, **kw) == E_SHAPE
    assert _call(hip, post=1, res_post=FAKE, **kw) == E_SCHEME        # a residual in the slot the projection takes
    assert _call(hip, post=0, res_pre=FAKE, **kw) == E_SCHEME
    assert _call(hip, cp=96, **kw) == E_UNSUPPORTED                   # Cp % 64 != 0
    assert _call(hip, cp=576, **kw) == E_UNSUPPORTED                  # above the LDS the weights may take
    assert _call(hip, n=1024, hw=(64, 64), phw=(64, 64), cp=256, **kw) == E_UNSUPPORTED       # proj_x: 2^30 elements
    assert _call(hip, c=192, **kw) == E_UNSUPPORTED                   # geometries outside the fp4 matrix-core kernel
    assert _call(hip, kernel=5, **kw) == E_UNSUPPORTED
    assert _call(hip, c=128, groups=2, **kw) == E_UNSUPPORTED
    assert _call(hip, o=80, **kw) == E_UNSUPPORTED
    assert _call(hip, kw_planes=2, **kw) == E_UNSUPPORTED             # more than one weight-plane pass
    assert _call(hip, kx=4, **kw) == E_UNSUPPORTED and _call(hip, kx=1, **kw) == E_UNSUPPORTED
    assert _call(hip, post=1, res_pre=FAKE, **kw) == E_UNSUPPORTED    # one residual array in registers
    for impl in (1, 2):                                               # the popcount / int8 debug implementations
        with hip.debug_switches(xnor_popcount=impl):
            assert _call(hip, **kw) == E_UNSUPPORTED


def test_refusals_come_before_any_pointer_is_read(hip):
    _refusals(hip)


@pytest.mark.gpu
def test_a_refused_call_leaves_y_untouched(hip):
    y = torch.full((2, 128, 6, 6), -7.5, device='cuda:0')
    buf = torch.zeros((1 << 16,), dtype=torch.int64, device='cuda:0')
    _refusals(hip, y=y.data_ptr(), ptrs=buf.data_ptr())
    torch.cuda.synchronize()
    assert bool((y == -7.5).all())
