"""What lsq_train_wgrad (liblsq_hip_train.so) and lsq_train_wgrad_half (liblsq_hip_train_half.so) take from one header,
csrc/train/lsq_wgrad_core.h, checked on the host through both entry points (no GPU: the workspace queries are plain host
functions and every refusal returns before a launch): the tile and split rule against the independent restatements of
tests/golden/train_wgrad_half_cases.py, where the two reductions have the same chunks, and one table of refused geometries
with one code each for both entries."""

import ctypes
import os

import pytest

import train_wgrad_half_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ml-quant_amd', 'csrc')


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not (os.path.exists(_hip.train_library_path()) and os.path.exists(_hip.train_half_library_path())):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def _geom(hip, c):
    return hip.make_geom(c.N, c.C, c.H, c.W, c.O, c.k[0], c.k[1], (c.stride, c.stride), c.pad, (1, 1), 1)


def test_the_fp32_workspace_is_plan_fp32_on_every_case(hip):
    fp32 = hip.train_lib().lsq_train_wgrad_workspace_bytes
    split = 0
    for c in T.CASES:
        p = T.plan_fp32(c)
        assert fp32(ctypes.byref(_geom(hip, c)), T.kx_of(c)) == p.workspace_bytes, c.id
        assert p.workspace_bytes % 16 == 0 and (p.workspace_bytes == 0) == (p.S == 1), c.id
        assert (p.S - 1) * p.chunks_per_split < p.chunks <= p.S * p.chunks_per_split, c.id       # no empty slice
        split += p.S > 1
    assert split >= 8 and T.plan_fp32(T.BY_ID['one_chunk']).S == 1


def test_whole_k_steps_a_sample_give_both_kernels_the_same_chunks(hip):
    """where Ho Wo is a multiple of 64 the chunks, slices and slab bytes of the 16-bit kernel are exactly the fp32
    kernel's.  (A multiple of 16 is enough: no k-step is padded, so four k-steps are 64 consecutive positions.)  Elsewhere the
    padding makes more chunks."""
    fp32 = hip.train_lib().lsq_train_wgrad_workspace_bytes
    half = hip.train_half_lib().lsq_train_wgrad_half_workspace_bytes
    same = []
    for c in T.CASES:
        p, q = T.plan(c), T.plan_fp32(c)
        assert (p.TT, p.ntc, p.tiles, p.slab_floats) == (q.TT, q.ntc, q.tiles, q.slab_floats), c.id      # one tile rule
        geom = _geom(hip, c)
        if p.howo % 16 == 0:
            same.append(c.id)
            assert (p.chunks, p.S, p.chunks_per_split) == (q.chunks, q.S, q.chunks_per_split), c.id
            assert half(ctypes.byref(geom), T.kx_of(c), 0) == fp32(ctypes.byref(geom), T.kx_of(c)) == q.workspace_bytes, c.id
        else:
            assert p.chunks >= q.chunks and p.ksteps * 16 > c.N * p.howo, c.id
    assert [i for i in same if T.plan(T.BY_ID[i]).howo % 64 == 0] == ['sample_is_chunk', 'r18_64_64_56']
    assert same == ['sample_is_chunk', 'r18_64_64_56', 'r18_64_128_56', 'r18_128_128_28']
    assert T.plan(T.BY_ID['r18_128_128_28']).howo == 28 * 28 and T.plan(T.BY_ID['r18_64_64_56']).howo == 56 * 56


def test_both_entries_refuse_the_same_geometries_with_the_same_code(hip):
    """One table, two entry points.  The pointers are garbage addresses and are never read: every call fails its geometry check
    first; both workspace queries answer 0."""
    fp32, fp32_ws = hip.train_lib().lsq_train_wgrad, hip.train_lib().lsq_train_wgrad_workspace_bytes
    half, half_ws = hip.train_half_lib().lsq_train_wgrad_half, hip.train_half_lib().lsq_train_wgrad_half_workspace_bytes
    mk = lambda **kw: hip.make_geom(*[kw.get(n, v) for n, v in T.REFUSAL_BASE.items()])
    x, xs, gy, out, gb, ws = (i << 20 for i in range(1, 7))
    ok = mk()
    assert fp32_ws(ctypes.byref(ok), 2) > 0 and half_ws(ctypes.byref(ok), 2, 1) > 0          # the base geometry is accepted
    assert {code for _, code in T.REFUSED} == {T.E_SHAPE, T.E_UNSUPPORTED} and len(T.REFUSED) >= 17
    for change, code in T.REFUSED:
        assert set(change) <= set(T.REFUSAL_BASE), change
        bad = mk(**change)
        assert fp32(x, 2, xs, gy, ctypes.byref(bad), out, ws, 1 << 30, None) == code, change
        for dtype in (1, 2):
            assert half(x, 2, xs, gy, dtype, ctypes.byref(bad), out, gb, ws, 1 << 30, None) == code, change
        assert fp32_ws(ctypes.byref(bad), 2) == 0 and half_ws(ctypes.byref(bad), 2, 0) == 0 and half_ws(ctypes.byref(bad), 2, 1) == 0
    # the checks in front of the geometry's, in the same order for both
    for kx in (0, -1, 9):
        assert fp32(x, kx, xs, gy, ctypes.byref(ok), out, ws, 1 << 30, None) == T.E_SCHEME
        assert half(x, kx, xs, gy, 1, ctypes.byref(ok), out, gb, ws, 1 << 30, None) == T.E_SCHEME
        bad = mk(groups=2)                                           # a bad plane count is named before a bad geometry
        assert fp32(x, kx, xs, gy, ctypes.byref(bad), out, ws, 1 << 30, None) == T.E_SCHEME
        assert half(x, kx, xs, gy, 1, ctypes.byref(bad), out, gb, ws, 1 << 30, None) == T.E_SCHEME
    assert fp32(x, 2, xs, gy, None, out, ws, 1 << 30, None) == T.E_NULL
    assert half(x, 2, xs, gy, 1, None, out, gb, ws, 1 << 30, None) == T.E_NULL


def test_the_shared_rules_stand_in_one_file():
    """check_geom, the tile rule, the constants, the workspace check and the reduce kernel are text of lsq_wgrad_core.h alone,
    and both Makefiles rebuild on it."""
    core = open(os.path.join(CSRC, 'train', 'lsq_wgrad_core.h')).read()
    files = [open(os.path.join(CSRC, d, f)).read() for d, f in (('train', 'lsq_wgrad.hip'), ('train_half', 'lsq_wgrad_half.hip'))]
    for once in ('int check_geom(', 'kTargetGroups = 512', 'kTapTile = 9', 'kApitch = ', 'TilePlan tile_plan(', 'WgradGeom fill_geom(',
                 'void wgrad_reduce_kernel(', 'int check_workspace(', 'int launch_wgrad(', 'struct SignSmem', 'struct WgradGeom'):
        assert core.count(once) == 1, once
        assert all(once not in f for f in files), once
    for f in files:
        assert 'lsq_wgrad_core.h"' in f and 'check_geom(g, kx)' in f and 'tile_plan(' in f and 'launch_wgrad(' in f
        assert 'hipLaunchKernelGGL' not in f and 'LSQ_E_WORKSPACE' not in f
    for d in ('train', 'train_half'):
        hdrs = [l for l in open(os.path.join(CSRC, d, 'Makefile')).read().splitlines() if l.startswith('HDRS')]
        assert len(hdrs) == 1 and 'lsq_wgrad_core.h' in hdrs[0] and 'lsq_signw_mma.h' in hdrs[0], d
