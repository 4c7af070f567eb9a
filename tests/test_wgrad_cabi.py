"""The training library (liblsq_hip_train.so, include/lsq_hip_train.h) builds for gfx950, loads, exports exactly what its
header declares, and returns every argument error before a launch (no GPU needed: nothing here reaches a kernel)."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch  # noqa: F401  (its HIP runtime must be the one the library binds to)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_train.h')
E_NULL, E_SHAPE, E_SCHEME, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -3, -5, -6


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.train_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.train_library_path())
    assert hip.train_lib().lsq_train_abi_version() == hip.TRAIN_ABI_VERSION == 1


def test_header_declares_exactly_the_train_entry_points():
    assert declared_functions() == ['lsq_train_abi_version', 'lsq_train_wgrad', 'lsq_train_wgrad_workspace_bytes']


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('no nm on this machine')
    out = subprocess.run([nm, '-D', '--defined-only', hip.train_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == declared_functions()


def _call(hip, geom, kx=2, planes=1 << 20, scales=1 << 20, gy=1 << 20, out=1 << 20, ws=None, ws_bytes=None):
    tl = hip.train_lib()
    need = tl.lsq_train_wgrad_workspace_bytes(ctypes.byref(geom) if geom is not None else None, kx)
    if ws_bytes is None:
        ws_bytes = need
    if ws is None and need:
        ws = 1 << 20
    return tl.lsq_train_wgrad(planes, kx, scales, gy, ctypes.byref(geom) if geom is not None else None, out, ws, ws_bytes,
                              None)


def test_workspace_query(hip):
    tl = hip.train_lib()
    big = hip.make_geom(256, 64, 56, 56, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    assert tl.lsq_train_wgrad_workspace_bytes(ctypes.byref(big), 2) > 0              # K is split over workgroups
    assert tl.lsq_train_wgrad_workspace_bytes(ctypes.byref(big), 2) == tl.lsq_train_wgrad_workspace_bytes(ctypes.byref(big), 8)
    tiny = hip.make_geom(1, 3, 1, 1, 1, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    assert tl.lsq_train_wgrad_workspace_bytes(ctypes.byref(tiny), 1) == 0             # one chunk: no split, no slabs
    bad = hip.make_geom(2, 64, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 2)
    assert tl.lsq_train_wgrad_workspace_bytes(ctypes.byref(bad), 2) == 0
    assert tl.lsq_train_wgrad_workspace_bytes(None, 2) == 0


def test_argument_errors_return_before_a_launch(hip):
    # the pointers are never dereferenced on these paths: every call below must fail its checks first
    g = lambda *a, **k: hip.make_geom(*a, **k)            # noqa: E731
    ok = g(4, 64, 8, 8, 32, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    assert _call(hip, None) == E_NULL
    for name in ('planes', 'scales', 'gy', 'out'):
        assert _call(hip, ok, **{name: None}) == E_NULL, name
    for kx in (0, -1, 9):
        assert _call(hip, ok, kx=kx) == E_SCHEME, kx
    assert _call(hip, g(0, 64, 8, 8, 32, 3, 3, (1, 1), (1, 1), (1, 1), 1)) == E_SHAPE
    assert _call(hip, g(4, 64, 8, 8, 0, 3, 3, (1, 1), (1, 1), (1, 1), 1)) == E_SHAPE
    assert _call(hip, g(4, 64, 1, 1, 32, 3, 3, (1, 1), (0, 0), (1, 1), 1)) == E_SHAPE           # kernel larger than the input
    assert _call(hip, g(4, 64, 8, 8, 32, 3, 3, (1, 1), (-1, 1), (1, 1), 1)) == E_SHAPE
    assert _call(hip, g(4, 64, 8, 8, 30, 3, 3, (1, 1), (1, 1), (1, 1), 4)) == E_SHAPE           # O not divisible by groups
    assert _call(hip, g(4, 64, 8, 8, 32, 3, 3, (1, 1), (1, 1), (1, 1), 2)) == E_UNSUPPORTED     # groups
    assert _call(hip, g(4, 64, 8, 8, 32, 3, 3, (1, 1), (1, 1), (2, 2), 1)) == E_UNSUPPORTED     # dilation
    assert _call(hip, g(4, 64, 8, 8, 32, 3, 3, (3, 3), (1, 1), (1, 1), 1)) == E_UNSUPPORTED     # stride 3
    assert _call(hip, g(4, 64, 8, 8, 32, 3, 3, (1, 2), (1, 1), (1, 1), 1)) == E_UNSUPPORTED     # unequal strides
    assert _call(hip, g(4, 64, 8, 8, 32, 3, 3, (1, 1), (3, 1), (1, 1), 1)) == E_UNSUPPORTED     # pad > k - 1
    assert _call(hip, g(4, 64, 12, 12, 32, 9, 9, (1, 1), (1, 1), (1, 1), 1)) == E_UNSUPPORTED   # kernel > 8
    big = g(256, 64, 56, 56, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    assert _call(hip, big, ws=None, ws_bytes=0) == E_WORKSPACE                                   # workspace too small
    assert _call(hip, big, ws_bytes=1024) == E_WORKSPACE
    need = hip.train_lib().lsq_train_wgrad_workspace_bytes(ctypes.byref(big), 2)
    assert _call(hip, big, ws=(1 << 20) + 4, ws_bytes=need) == E_WORKSPACE                       # misaligned workspace
