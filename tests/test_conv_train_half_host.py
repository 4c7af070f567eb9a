"""The C ABI of liblsq_hip_conv_train_half.so on the host (no GPU): header, exports, ABI version, the SUBLIBS row, the
missing-library error, plan and workspace size against the fp32 library for every case, every refusal returned before a launch
with nothing written, the Python wrapper's operand checks, ``hip_train.supported`` with ``hip_train_half``, and the conditions
the table of tests/golden/conv_train_half_cases.py must meet."""

import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import conv_dgrad_cases as D
import conv_train_half_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_conv_train_half.h')
PATTERN = r'lsq_conv_train_half_[a-z0-9_]+|lsq_signw_conv2d_dgrad_half[a-z0-9_]*'
E_NULL, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5, -6
F32, BF16, F16 = 0, 1, 2
# cases of two or more activation planes whose clamp leaves the second sign no edge (as in the fp32 table: v_1 <= 1 < alpha - v_1)
NO_EDGE = ('k4x3_padfull', 's2_pad0')
ENTRY_POINTS = ['lsq_conv_train_half_abi_version', 'lsq_signw_conv2d_dgrad_half', 'lsq_signw_conv2d_dgrad_half_plan',
                'lsq_signw_conv2d_dgrad_half_workspace_bytes']


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not (os.path.exists(_hip.conv_train_half_library_path()) and os.path.exists(_hip.conv_train_library_path())):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def _geom(hip, c, **changes):
    c = c._replace(**changes) if changes else c
    return hip.make_geom(c.N, c.C, c.H, c.W, c.O, c.KH, c.KW, (c.stride_h, c.stride_w), (c.pad_h, c.pad_w),
                         (c.dil_h, c.dil_w), c.groups)


# ------------------------------------------------------------------------------------------------- header and library
def test_header_declares_exactly_the_four_entry_points():
    assert declared_functions() == ENTRY_POINTS
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_CONV_TRAIN_HALF_ABI_VERSION\s+1\b', text)
    for inc in ('lsq_hip.h', 'lsq_hip_conv_train.h', 'lsq_hip_linear_half.h'):       # geometry, the plan, LSQ_DTYPE_*
        assert f'#include "{inc}"' in text


def test_the_library_is_a_sublib_of_the_build():
    import __graft_entry__
    row = [s for s in __graft_entry__.SUBLIBS if s[0] == 'conv_train_half']
    assert len(row) == 1
    assert row[0][1:3] == ('conv_train_half_lib', 'lsq_hip_conv_train_half.h') and row[0][5] == 'CONV_TRAIN_HALF_ABI_VERSION'
    assert row[0][3] == PATTERN and sorted(row[0][4]) == ENTRY_POINTS
    assert sorted(set(re.findall(r'\b(' + PATTERN + r')\s*\(', open(HEADER).read()))) == ENTRY_POINTS
    assert os.path.exists(os.path.join(ROOT, 'ml-quant_amd', 'csrc', 'conv_train_half', 'Makefile'))
    # the new row claims no other library's symbols, and no other header declares the new ones
    for other in __graft_entry__.SUBLIBS:
        if other[0] != 'conv_train_half':
            assert not any(re.fullmatch(PATTERN, name) for name in other[4]), other[0]
            with open(os.path.join(ROOT, 'include', other[2])) as f:
                assert not re.findall(r'\b(' + PATTERN + r')\s*\(', f.read()), other[2]


def test_the_kernels_are_one_source_for_both_libraries():
    """The kernels live in a header beside the fp32 library's source; both sources include it and hold no kernel of their own."""
    csrc = os.path.join(ROOT, 'ml-quant_amd', 'csrc')
    shared = open(os.path.join(csrc, 'conv_train', 'lsq_conv_dgrad.h')).read()
    for name in ('transpose_planes', 'dgrad_patch', 'dgrad_conv', 'shape_of'):
        assert name in shared
    for path in (('conv_train', 'lsq_conv_train.hip'), ('conv_train_half', 'lsq_conv_train_half.hip')):
        text = open(os.path.join(csrc, *path)).read()
        assert 'lsq_conv_dgrad.h"' in text and '__global__' not in text and 'mfma' not in text, path


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.conv_train_half_library_path())
    assert hip.conv_train_half_lib().lsq_conv_train_half_abi_version() == hip.CONV_TRAIN_HALF_ABI_VERSION == 1
    assert hip.conv_train_lib().lsq_conv_train_abi_version() == hip.CONV_TRAIN_ABI_VERSION == 1      # (unchanged)


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm') or shutil.which('llvm-nm') or '/opt/rocm/llvm/bin/llvm-nm'
    out = subprocess.run([nm, '-D', '--defined-only', hip.conv_train_half_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == ENTRY_POINTS


def test_a_missing_library_is_an_error(hip, monkeypatch, tmp_path):
    monkeypatch.setattr(hip, '_LIB_DIR', str(tmp_path))              # (where the libraries are looked for: none is there)
    monkeypatch.delitem(hip._handles, 'conv_train_half', raising=False)
    assert hip.conv_train_half_library_path() == str(tmp_path / 'liblsq_hip_conv_train_half.so')
    with pytest.raises(hip.LsqHipError, match='csrc/conv_train_half'):
        hip.conv_train_half_lib()
    with pytest.raises(hip.LsqHipError):
        hip.signw_conv2d_dgrad_half_supported(_geom(hip, H.ODD))


# ------------------------------------------------------------------------------------------- plan and workspace size
PLAN_FIELDS = ('kernel', 'classes', 'dead_classes', 'tap_steps')
REFUSED_GEOMETRIES = (dict(N=0), dict(groups=5), dict(H=1, pad_h=0), dict(N=1 << 20, H=64, W=64), dict(stride_h=256, stride_w=256),
                      dict(groups=1, C=1 << 24, H=1, W=1, pad_h=1, pad_w=1, N=1))


@pytest.mark.parametrize('case', H.CASES, ids=lambda c: c.id)
def test_plan_and_workspace_equal_the_fp32_library(hip, case):
    f32, half = hip.conv_train_lib(), hip.conv_train_half_lib()
    g = _geom(hip, case)
    a, b = hip.signw_conv2d_dgrad_plan(g), hip.signw_conv2d_dgrad_half_plan(g)
    assert a is not None and b is not None and hip.signw_conv2d_dgrad_half_supported(g)
    assert [getattr(a, f) for f in PLAN_FIELDS] == [getattr(b, f) for f in PLAN_FIELDS]
    assert b.kernel == (2 if H.wide(case) else 1) | (4 if H.patch_positions(case) is not None else 0)
    for kw in (0, 1, 2, 3, 8, 9):
        need = int(half.lsq_signw_conv2d_dgrad_half_workspace_bytes(ctypes.byref(g), kw))
        assert need == int(f32.lsq_signw_conv2d_dgrad_workspace_bytes(ctypes.byref(g), kw)), kw
        assert (need > 0) == (1 <= kw <= 8)
    for bad in REFUSED_GEOMETRIES:
        gb = _geom(hip, case, **bad)
        pa, pb = hip.ConvDgradPlan(), hip.ConvDgradPlan()
        ea = f32.lsq_signw_conv2d_dgrad_plan(ctypes.byref(gb), ctypes.byref(pa))
        eb = half.lsq_signw_conv2d_dgrad_half_plan(ctypes.byref(gb), ctypes.byref(pb))
        assert ea == eb, bad
        if ea == 0:                                   # (a change that this case's other sizes make harmless)
            assert [getattr(pa, f) for f in PLAN_FIELDS] == [getattr(pb, f) for f in PLAN_FIELDS]
        assert (int(half.lsq_signw_conv2d_dgrad_half_workspace_bytes(ctypes.byref(gb), 1))
                == int(f32.lsq_signw_conv2d_dgrad_workspace_bytes(ctypes.byref(gb), 1)))


def test_every_kernel_is_reached(hip):
    assert {hip.signw_conv2d_dgrad_half_plan(_geom(hip, c)).kernel for c in H.CASES} == {1, 2, 5, 6}
    assert hip.signw_conv2d_dgrad_half_plan(_geom(hip, H.ODD)).kernel == 5
    lib = hip.conv_train_half_lib()
    assert lib.lsq_signw_conv2d_dgrad_half_plan(None, ctypes.byref(hip.ConvDgradPlan())) == E_NULL
    assert lib.lsq_signw_conv2d_dgrad_half_plan(ctypes.byref(_geom(hip, H.ODD)), None) == E_NULL
    assert int(lib.lsq_signw_conv2d_dgrad_half_workspace_bytes(None, 1)) == 0


# ----------------------------------------------------------------------------------------------------- argument errors
class _Host:
    """Host buffers filled with sentinels stand in for grad_x and the workspace: a refused call never dereferences a pointer
    (the other operands are garbage addresses) and leaves every byte as it was."""

    def __init__(self):
        self.gx = np.full((1 << 16,), 12345.0, dtype=np.float32)
        self.ws = np.full((1 << 16,), -77.0, dtype=np.float32)
        self.keep = self.gx.copy(), self.ws.copy()

    def untouched(self):
        return np.array_equal(self.gx, self.keep[0]) and np.array_equal(self.ws, self.keep[1])


GARBAGE = 1 << 20


def _call(hip, host, c, gy=GARBAGE, gy_dtype=BF16, wbits=GARBAGE, kw=1, wscales=GARBAGE, x=None, kx=0, xscales=None, alpha=-1.0,
          gx=True, gx_dtype=None, ws=True, ws_bytes=None, ws_shift=0, geom=True, **changes):
    g = ctypes.byref(_geom(hip, c, **changes)) if geom else None
    gx_ptr = host.gx.ctypes.data if gx is True else gx
    ws_ptr = host.ws.ctypes.data + ws_shift if ws is True else ws
    ws_bytes = host.ws.nbytes if ws_bytes is None else ws_bytes
    return hip.conv_train_half_lib().lsq_signw_conv2d_dgrad_half(
        gy, gy_dtype, wbits, kw, wscales, g, x, kx, xscales, alpha, gx_ptr, gy_dtype if gx_dtype is None else gx_dtype, ws_ptr,
        ws_bytes, None)


def test_every_refusal_returns_before_a_launch_and_writes_nothing(hip):
    host = _Host()
    c = D.BY_ID['g2_tails']
    need = int(hip.conv_train_half_lib().lsq_signw_conv2d_dgrad_half_workspace_bytes(ctypes.byref(_geom(hip, c)), 1))
    assert 0 < 2 * need <= host.ws.nbytes
    # those of lsq_signw_conv2d_dgrad
    for name in ('gy', 'wbits', 'wscales', 'gx'):
        assert _call(hip, host, c, **{name: None}) == E_NULL, name
    assert _call(hip, host, c, geom=False) == E_NULL
    for bad in (dict(N=0), dict(C=-8), dict(KH=0), dict(stride_w=0), dict(dil_h=0), dict(pad_w=-1), dict(groups=0),
                dict(groups=5), dict(H=1, pad_h=0), dict(W=2, dil_w=3, pad_w=0)):
        assert _call(hip, host, c, **bad) == E_SHAPE, bad
    for bad in (dict(kw=0), dict(kw=9), dict(kw=-1), dict(N=1 << 20, H=64, W=64), dict(stride_h=256, stride_w=256),
                dict(groups=1, C=1 << 24, H=1, W=1, pad_h=1, pad_w=1, N=1)):
        assert _call(hip, host, c, **bad) == E_UNSUPPORTED, bad
    assert _call(hip, host, c, ws_bytes=need - 1) == E_WORKSPACE
    assert _call(hip, host, c, ws_bytes=0) == E_WORKSPACE
    assert _call(hip, host, c, ws=None) == E_WORKSPACE
    assert _call(hip, host, c, ws_shift=4) == E_WORKSPACE          # misaligned
    assert _call(hip, host, c, kw=2, ws_bytes=need) == E_WORKSPACE       # two planes need twice the image
    # the new ones: types
    for dt in (F32, 3, -1, 7):
        assert _call(hip, host, c, gy_dtype=dt, gx_dtype=F32) == E_UNSUPPORTED, dt
    assert _call(hip, host, c, gy_dtype=BF16, gx_dtype=F16) == E_UNSUPPORTED
    assert _call(hip, host, c, gy_dtype=F16, gx_dtype=BF16) == E_UNSUPPORTED
    assert _call(hip, host, c, gy_dtype=F16, gx_dtype=3) == E_UNSUPPORTED
    # activation planes
    for kx in (-1, 9, 100):
        assert _call(hip, host, c, x=GARBAGE, kx=kx, xscales=GARBAGE) == E_UNSUPPORTED, kx
        assert _call(hip, host, c, kx=kx) == E_UNSUPPORTED, kx             # (checked without x too)
    assert _call(hip, host, c, x=GARBAGE, kx=2, xscales=None) == E_NULL
    assert _call(hip, host, c, x=GARBAGE, kx=8, xscales=None) == E_NULL
    # the sample limit of lsq_ste_backward, with x only: without x the same geometry passes every check up to the workspace
    big = dict(N=65536, C=2, O=2, groups=1, H=3, W=3)
    assert _call(hip, host, c, x=GARBAGE, kx=1, xscales=GARBAGE, **big) == E_UNSUPPORTED
    assert _call(hip, host, c, x=GARBAGE, kx=0, **big) == E_UNSUPPORTED
    assert _call(hip, host, c, ws_bytes=0, **big) == E_WORKSPACE
    assert _call(hip, host, c, x=GARBAGE, kx=1, xscales=GARBAGE, ws_bytes=0, **dict(big, N=65535)) == E_WORKSPACE
    # operands not aligned to their element
    assert _call(hip, host, c, gy=GARBAGE + 1) == E_UNSUPPORTED
    assert _call(hip, host, c, x=GARBAGE + 1) == E_UNSUPPORTED
    assert _call(hip, host, c, gx=host.gx.ctypes.data + 1) == E_UNSUPPORTED
    assert _call(hip, host, c, gx=host.gx.ctypes.data + 2, gx_dtype=F32) == E_UNSUPPORTED
    assert host.untouched()


def test_python_wrapper_checks_operands_on_the_host(hip):
    c = D.BY_ID['g2_tails']
    geom = _geom(hip, c)
    ho, wo = D.out_hw(c)
    gy = torch.zeros((c.N, c.O, ho, wo), dtype=torch.bfloat16)
    x = torch.zeros((c.N, c.C, c.H, c.W), dtype=torch.bfloat16)
    words = 9 * 1 * 2 * 32
    wbits = torch.zeros((2 * words,), dtype=torch.int64)
    wsc = torch.ones((2, c.O), dtype=torch.float32)
    xsc = torch.ones((1, c.N), dtype=torch.float32)
    f = hip.signw_conv2d_dgrad_half
    with pytest.raises(TypeError, match='bfloat16 or float16'):
        f(gy.float(), wbits, wsc, geom)
    with pytest.raises(TypeError, match='out_dtype'):
        f(gy, wbits, wsc, geom, out_dtype=torch.float16)
    with pytest.raises(TypeError, match="gy's type"):
        f(gy, wbits, wsc, geom, x.half(), xsc)
    with pytest.raises(TypeError, match='float32'):
        f(gy, wbits, wsc.half(), geom)
    with pytest.raises(TypeError, match='float32'):
        f(gy, wbits, wsc, geom, x, xsc.double())
    with pytest.raises(TypeError, match='int64'):
        f(gy, wbits.int(), wsc, geom)
    with pytest.raises(ValueError, match='xscales without x'):
        f(gy, wbits, wsc, geom, None, xsc)
    with pytest.raises(ValueError, match='cuda device'):          # CPU tensors: the kernel reads device memory only
        f(gy, wbits, wsc, geom, x, xsc)
    with pytest.raises(ValueError, match='contiguous'):
        f(torch.zeros((c.N, c.O, ho, 2 * wo), dtype=torch.bfloat16)[..., ::2], wbits, wsc, geom)
    with pytest.raises(ValueError, match='contiguous'):
        f(gy, wbits, wsc, geom, torch.zeros((c.N, c.C, c.H, 2 * c.W), dtype=torch.bfloat16)[..., ::2], xsc)
    with pytest.raises(ValueError, match='do not match'):         # a gradient of another geometry
        f(gy, wbits, wsc, _geom(hip, c, stride_h=2))
    with pytest.raises(ValueError, match='do not match'):         # planes of another plane count
        f(gy, wbits, torch.ones((1, c.O)), geom)
    with pytest.raises(ValueError, match='do not match'):
        f(gy, wbits, wsc, geom, x[:, :-1].contiguous(), xsc)
    with pytest.raises(ValueError, match='do not match'):
        f(gy, wbits, wsc, geom, x, torch.ones((1, c.N + 1)))
    with pytest.raises(ValueError, match='bad sizes'):
        f(gy[0], wbits, wsc, geom)
    with pytest.raises(ValueError, match='bad sizes'):
        f(gy, wbits, wsc, geom, x, torch.ones((9, c.N)))


# ------------------------------------------------------------------------------------------------- hip_train.supported
class _DeviceTensor:
    """What ``supported`` reads of its input, claiming to live on a GPU: the clauses can be reached on the host."""
    is_cuda = True

    def __init__(self, shape, dtype):
        self.shape, self.dtype = torch.Size(shape), dtype

    def dim(self):
        return len(self.shape)


def test_the_switch_is_off_by_default_and_a_class_attribute():
    from quant.binary.binary_conv import QuantConv2d
    assert QuantConv2d.hip_train_half is False and 'hip_train_half' in vars(QuantConv2d)
    assert QuantConv2d.act_half is False and QuantConv2d.fp_half is False


@pytest.mark.parametrize('dtype', H.DTYPES, ids=lambda t: H.DTYPE_NAMES[t])
def test_supported_takes_16_bit_inputs_with_the_switch_only(hip, monkeypatch, dtype):
    from quant.binary import hip_train
    for on in (False, True):                          # DGRAD_KERNEL does not matter for a 16-bit input
        monkeypatch.setattr(hip_train, 'DGRAD_KERNEL', on)
        for c in H.CASES:
            conv, x = H.make_module(c), _DeviceTensor((c.N, c.C, c.H, c.W), dtype)
            assert not conv.act_half and not conv.fp_half
            assert not hip_train.supported(conv, x), c.id
            conv.hip_train_half = True
            assert hip_train.supported(conv, x), c.id                     # independent of act_half / fp_half
            assert not hip_train.supported(conv, H.inputs(c.id, dtype)['x']), c.id      # a CPU tensor
            conv.act_half = conv.fp_half = True
            assert hip_train.supported(conv, x), c.id
            conv.hip_train_half = False
            assert not hip_train.supported(conv, x), c.id


def test_what_stays_refused_with_the_switch_on(hip):
    from quant.binary import hip_train
    from quant.binary.binary_conv import QuantConv2d

    def conv(xs='ls-1', ws='ls-1', **kw):
        kw.setdefault('padding', 1)
        m = QuantConv2d(xs, ws, 8, 16, 3, dict(D.SYM2), **kw).train()
        m.hip_train_half = True
        return m
    x = _DeviceTensor((2, 8, 9, 8), torch.bfloat16)
    assert hip_train.supported(conv(), x) and hip_train.supported(conv('fp'), x)
    assert not hip_train.supported(conv(ws='fp'), x)
    assert not hip_train.supported(conv(padding_mode='reflect'), x)
    assert not hip_train.supported(conv(padding='same'), x)
    assert not hip_train.supported(conv(dilation=5), x)                               # an empty output: the plan refuses
    assert not hip_train.supported(conv().half(), x)                                  # 16-bit weights
    assert not hip_train.supported(conv(), _DeviceTensor((2, 8, 9, 8), torch.float64))
    assert not hip_train.supported(conv(), _DeviceTensor((8, 9, 8), torch.bfloat16))
    assert not hip_train.supported(conv(), _DeviceTensor((65536, 8, 9, 8), torch.bfloat16))        # lsq_ste_backward's limit
    assert not hip_train.supported(QuantConv2d('ls-1', 'ls-1', 8, 16, 9, dict(D.SYM2), padding=4).train(), x)
    big = QuantConv2d('ls-1', 'ls-1', 8, 16, 9, dict(D.SYM2), padding=4).train()      # 9 x 9: past the XNOR forward's kernels
    big.hip_train_half = True
    assert not hip_train.supported(big, _DeviceTensor((2, 8, 12, 12), torch.bfloat16))
    # (the autocast rule needs a GPU to be switched on: tests/test_gpu_conv_train_half.py)
    # the fp32 step's rule is what it was
    assert hip_train.supported(conv(), _DeviceTensor((2, 8, 9, 8), torch.float32))
    off = conv()
    off.hip_train_half = False
    assert hip_train.supported(off, _DeviceTensor((2, 8, 9, 8), torch.float32)) and not hip_train.supported(off, x)


# ------------------------------------------------------------------------------------------------------ the table
def test_the_table_holds_the_31_cases_and_the_odd_one():
    assert [c.id for c in H.CASES[:31]] == [c.id for c in D.CASES] and len(D.CASES) == 31 and len(H.CASES) == 32
    assert len(H.PAIRS) == 64 and len({H.pair_id(p) for p in H.PAIRS}) == 64
    o = H.ODD
    assert (o.KH, o.KW, o.stride_h, o.stride_w, o.N, o.C, o.H, o.W) == (3, 3, 1, 1, 3, 5, 5, 7)
    assert (o.H * o.W) % 2 == 1 and (o.C * o.H * o.W) % 2 == 1 and (o.O * H.out_hw(o)[0] * H.out_hw(o)[1]) % 2 == 1
    for c in H.CASES:
        assert c.N <= 3 and c.O * (c.C // c.groups) * c.KH * c.KW <= 160_000, c.id


@pytest.mark.parametrize('pair', H.PAIRS, ids=H.pair_id)
def test_inputs_are_values_of_the_type_with_the_special_values_in_place(pair):
    c, dtype = pair
    d = H.inputs(c.id, dtype)
    base = H._fp32_inputs(c)
    x, gy, alpha = d['x'], d['gy'], d['alpha']
    assert x.dtype == dtype and gy.dtype == dtype and d['w'].dtype == torch.float32
    assert tuple(x.shape) == (c.N, c.C, c.H, c.W) and tuple(gy.shape) == (c.N, c.O) + H.out_hw(c)
    assert torch.equal(gy, base['gy'].to(dtype)) and torch.equal(d['w'], base['w'])
    assert alpha == D.alpha_of(c.clamp) and len(d['xscales']) == H.planes(c.xs)
    flat = x.view(-1).float()
    if flat.numel() < 64:
        return
    assert bool((flat[::11][1:] == 0).any()) and bool(torch.signbit(flat[flat == 0]).any()) and bool((flat == 1).any())
    assert bool((flat == -1).any())
    if alpha >= 0:                                    # each clamped case holds elements exactly at +-alpha
        assert bool((flat == alpha).any()) and bool((flat == -alpha).any())
        assert bool((flat.abs() > alpha).any())       # ... and some the clamp cuts off
    xs = d['xscales']
    ref = D.step64(c, x.float(), d['w'], d['b'], gy.float(), xs, list(H.weight_scales(c.id)))
    m = ref['m_x']
    if xs or alpha >= 0:                              # where an estimator or a clamp exists: neither all-open nor all-closed
        assert bool((m == 0).any()) and bool((m != 0).any()), c.id
    else:
        assert bool((m == 1).all())
    if len(xs) >= 2 and c.id not in NO_EDGE:          # an element on each side of the second sign's edge, one step of the type apart
        v1 = float(xs[0][0])
        e = H.edge_of(c, v1, dtype)
        assert e > 0, (c.id, v1)
        lo, hi = H.edge_pair(c, v1, dtype)
        assert lo <= e <= hi and (alpha < 0 or hi <= alpha)
        row0 = x[0].view(-1).float()
        assert bool((row0 == lo).any()) and bool((row0 == hi).any()) and bool((row0 == -lo).any()) and bool((row0 == -hi).any())
        d1 = (row0.clamp(-alpha, alpha) if alpha >= 0 else row0) - v1 * torch.where(row0 >= 0, 1.0, -1.0)
        is_open = d1.abs() <= 1
        placed = torch.zeros_like(is_open)
        placed[d['edge_idx']] = True
        assert len(d['edge_idx']) >= 4
        assert bool(is_open[placed].any()) and bool((~is_open[placed]).any()), (c.id, v1, e, lo, hi)
    elif len(xs) >= 2:                                # no edge inside the clamp: 1 + v_1 is beyond it and v_1 <= 1
        v1 = float(xs[0][0])
        assert H.edge_of(c, v1, dtype) <= 0 and alpha >= 0 and 1 + v1 > alpha - 2 * H.UNIT[dtype] * alpha and d['edge_idx'] == []


def test_shifted_views_start_one_element_into_their_buffers():
    t = H.inputs('odd_planes', torch.bfloat16)['x']
    buf, view = H.shifted(t)
    assert view.data_ptr() == buf.data_ptr() + 2 and view.is_contiguous() and torch.equal(view, t)
    assert float(buf[0]) == -7.25 and bool((buf[1 + t.numel():] == -7.25).all())


def test_step64_is_the_fp32_tables_reference_on_the_rounded_values():
    c, dtype = H.ODD, torch.float16
    d = H.inputs(c.id, dtype)
    ws = list(H.weight_scales(c.id))
    a = H.step64(c, dtype, d['xscales'], ws)
    b = D.step64(c, d['x'].float(), d['w'], d['b'], d['gy'].float(), d['xscales'], ws)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # the reference of the new case against fp32 autograd through the torch formulation on the same values
    conv = H.make_module(c)
    x = d['x'].float().requires_grad_()
    y = conv._forward_torch(x)
    y.backward(d['gy'].float())
    for name, t in (('y', y), ('gx', x.grad), ('gw', conv.weight.grad), ('gb', conv.bias.grad)):
        err = float((t.detach().double() - a[name]).abs().max() / a[name].abs().max())
        assert err <= 1e-5, (name, err)
