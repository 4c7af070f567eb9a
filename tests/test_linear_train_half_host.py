"""The C ABI of liblsq_hip_linear_train_half.so on the host (no GPU): header, exports, ABI version, the SUBLIBS row, the
missing-library error, the workspace size against the fp32 library, every refusal returned before a launch with nothing
written, the Python wrapper's operand checks, ``hip_train_linear.supported`` with ``hip_train_half``, and the conditions the
table of tests/golden/linear_train_half_cases.py must meet."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import linear_train_half_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_linear_train_half.h')
PATTERN = r'lsq_linear_train_half_[a-z0-9_]+|lsq_linear_signw_dgrad_half[a-z0-9_]*'
E_NULL, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5, -6
F32, BF16, F16 = 0, 1, 2
ENTRY_POINTS = ['lsq_linear_signw_dgrad_half', 'lsq_linear_signw_dgrad_half_workspace_bytes', 'lsq_linear_train_half_abi_version']


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not (os.path.exists(_hip.linear_train_half_library_path()) and os.path.exists(_hip.linear_train_library_path())):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


# ------------------------------------------------------------------------------------------------- header and library
def test_header_declares_exactly_the_three_entry_points():
    assert declared_functions() == ENTRY_POINTS
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_LINEAR_TRAIN_HALF_ABI_VERSION\s+1\b', text)
    for inc in ('lsq_hip.h', 'lsq_hip_linear_half.h'):       # the error codes and LSQ_MAX_PLANES, LSQ_DTYPE_*
        assert f'#include "{inc}"' in text


def test_the_library_is_a_row_of_the_table():
    from quant import _sublibs
    row = _sublibs.BY_DIR['linear_train_half']
    assert (row.header, row.version_symbol, row.version) == ('lsq_hip_linear_train_half.h', 'lsq_linear_train_half_abi_version', 1)
    assert row.pattern == PATTERN and sorted(row.prototypes) == ENTRY_POINTS
    assert os.path.exists(os.path.join(ROOT, 'ml-quant_amd', 'csrc', 'linear_train_half', 'Makefile'))
    # the new row claims no other library's symbols, and no other header declares the new ones
    for other in _sublibs.SUBLIBS:
        if other.dir != 'linear_train_half':
            assert not any(re.fullmatch(PATTERN, name) for name in other.prototypes), other.dir
            assert not set(declared_functions(os.path.join(ROOT, 'include', other.header))) & set(ENTRY_POINTS), other.header


def test_the_kernels_are_one_source_for_both_libraries():
    """The kernels live in a header beside the fp32 library's source; both sources include it and hold no kernel of their own."""
    csrc = os.path.join(ROOT, 'ml-quant_amd', 'csrc')
    shared = open(os.path.join(csrc, 'linear_train', 'lsq_linear_dgrad.h')).read()
    for name in ('transpose_planes', 'dgrad_tiled', 'dgrad_split', 'launch_dgrad', 'tile_rule('):
        assert name in shared
    for path in (('linear_train', 'lsq_linear_train.hip'), ('linear_train_half', 'lsq_linear_train_half.hip')):
        text = open(os.path.join(csrc, *path)).read()
        assert 'lsq_linear_dgrad.h"' in text and '__global__' not in text and 'mfma' not in text, path


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.linear_train_half_library_path())
    assert hip.linear_train_half_lib().lsq_linear_train_half_abi_version() == hip.LINEAR_TRAIN_HALF_ABI_VERSION == 1
    assert hip.linear_train_lib().lsq_linear_train_abi_version() == hip.LINEAR_TRAIN_ABI_VERSION == 1      # (unchanged)


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm') or shutil.which('llvm-nm') or '/opt/rocm/llvm/bin/llvm-nm'
    out = subprocess.run([nm, '-D', '--defined-only', hip.linear_train_half_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == ENTRY_POINTS


def test_a_missing_library_is_an_error(hip, monkeypatch, tmp_path):
    monkeypatch.setattr(hip, '_LIB_DIR', str(tmp_path))              # (where the libraries are looked for: none is there)
    monkeypatch.delitem(hip._handles, 'linear_train_half', raising=False)
    assert hip.linear_train_half_library_path() == str(tmp_path / 'liblsq_hip_linear_train_half.so')
    with pytest.raises(hip.LsqHipError, match='csrc/linear_train_half'):
        hip.linear_train_half_lib()
    # the switch asked for the kernel: supported() raises too, where the input reaches that clause
    from quant.binary import hip_train_linear
    lin = L.make_module(L.BY_ID['ragged'])
    lin.hip_train_half = True
    lin.weight = _OnDevice(lin.weight)
    with pytest.raises(hip.LsqHipError):
        hip_train_linear.supported(lin, _DeviceTensor((7, 33), torch.bfloat16))


# ----------------------------------------------------------------------------------------------------- workspace size
def test_workspace_size_equals_the_fp32_library(hip):
    f32, half = hip.linear_train_lib(), hip.linear_train_half_lib()
    for kw in (0, 1, 2, 3, 8, 9, -1):
        for f in (1, 15, 16, 17, 63, 64, 65, 800, 4096, (1 << 22) - 1, 1 << 22, 0):
            for o in (1, 63, 64, 65, 130, 4096, (1 << 21) - 1, 1 << 21, 0):
                a = int(f32.lsq_linear_signw_dgrad_workspace_bytes(kw, f, o))
                b = int(half.lsq_linear_signw_dgrad_half_workspace_bytes(kw, f, o))
                assert a == b, (kw, f, o)
                ok = 1 <= kw <= 8 and 0 < f < 1 << 22 and 0 < o < 1 << 21
                assert (b > 0) == ok and (not ok or b == kw * ((o + 63) // 64) * ((f + 15) // 16 * 16) * 8), (kw, f, o)


# ----------------------------------------------------------------------------------------------------- argument errors
class _Host:
    """Host buffers filled with sentinels stand in for gx and the workspace: a refused call never dereferences a pointer (the
    other operands are garbage addresses) and leaves every byte as it was."""

    def __init__(self):
        self.gx = np.full((1 << 16,), 12345.0, dtype=np.float32)
        self.ws = np.full((1 << 16,), -77.0, dtype=np.float32)
        self.keep = self.gx.copy(), self.ws.copy()

    def untouched(self):
        return np.array_equal(self.gx, self.keep[0]) and np.array_equal(self.ws, self.keep[1])


GARBAGE = 1 << 20


def _call(hip, host, gy=GARBAGE, gy_dtype=BF16, wbits=GARBAGE, kw=1, wscales=GARBAGE, M=12, F=40, O=70, x=None, T=1, kx=0,
          xscales=None, alpha=-1.0, gx=True, gx_dtype=None, ws=True, ws_bytes=None, ws_shift=0):
    gx_ptr = host.gx.ctypes.data if gx is True else gx
    ws_ptr = host.ws.ctypes.data + ws_shift if ws is True else ws
    ws_bytes = host.ws.nbytes if ws_bytes is None else ws_bytes
    return hip.linear_train_half_lib().lsq_linear_signw_dgrad_half(
        gy, gy_dtype, wbits, kw, wscales, M, F, O, x, T, kx, xscales, alpha, gx_ptr, gy_dtype if gx_dtype is None else gx_dtype,
        ws_ptr, ws_bytes, None)


def test_every_refusal_returns_before_a_launch_and_writes_nothing(hip):
    host = _Host()
    need = int(hip.linear_train_half_lib().lsq_linear_signw_dgrad_half_workspace_bytes(1, 40, 70))
    assert 0 < 2 * need <= host.ws.nbytes
    # those of lsq_linear_signw_dgrad
    for name in ('gy', 'wbits', 'wscales', 'gx'):
        assert _call(hip, host, **{name: None}) == E_NULL, name
    for bad in (dict(M=0), dict(M=-3), dict(F=0), dict(O=0), dict(O=-1)):
        assert _call(hip, host, **bad) == E_SHAPE, bad
    for bad in (dict(kw=0), dict(kw=9), dict(kw=-1), dict(F=1 << 22), dict(O=1 << 21), dict(M=1 << 31)):
        assert _call(hip, host, **bad) == E_UNSUPPORTED, bad
    assert _call(hip, host, ws_bytes=need - 1) == E_WORKSPACE
    assert _call(hip, host, ws_bytes=0) == E_WORKSPACE
    assert _call(hip, host, ws=None) == E_WORKSPACE
    assert _call(hip, host, ws_shift=4) == E_WORKSPACE             # misaligned
    assert _call(hip, host, kw=2, ws_bytes=need) == E_WORKSPACE    # two planes need twice the image
    # the new ones: types
    for dt in (F32, 3, -1, 7):
        assert _call(hip, host, gy_dtype=dt, gx_dtype=F32) == E_UNSUPPORTED, dt
    assert _call(hip, host, gy_dtype=BF16, gx_dtype=F16) == E_UNSUPPORTED
    assert _call(hip, host, gy_dtype=F16, gx_dtype=BF16) == E_UNSUPPORTED
    assert _call(hip, host, gy_dtype=F16, gx_dtype=3) == E_UNSUPPORTED
    # activation planes
    for kx in (-1, 9, 100):
        assert _call(hip, host, x=GARBAGE, kx=kx, xscales=GARBAGE) == E_UNSUPPORTED, kx
        assert _call(hip, host, kx=kx) == E_UNSUPPORTED, kx             # (checked without x too)
    assert _call(hip, host, x=GARBAGE, kx=2, xscales=None) == E_NULL
    assert _call(hip, host, x=GARBAGE, kx=8, xscales=None) == E_NULL
    # rows per sample, with x only
    for t in (0, -1, 5, 7, 24):
        assert _call(hip, host, x=GARBAGE, T=t) == E_SHAPE, t
        assert _call(hip, host, T=t, ws_bytes=0) == E_WORKSPACE, t      # (without x: T is ignored, the call goes on to the workspace)
    # the sample limit of lsq_ste_backward, with x only: without x the same shape passes every check up to the workspace
    big = dict(M=65536 * 2, F=2, O=2)
    assert _call(hip, host, x=GARBAGE, kx=1, xscales=GARBAGE, T=1, **big) == E_UNSUPPORTED
    assert _call(hip, host, x=GARBAGE, kx=0, T=1, **big) == E_UNSUPPORTED
    assert _call(hip, host, x=GARBAGE, kx=0, T=2, **big) == E_UNSUPPORTED          # 65536 samples
    assert _call(hip, host, ws_bytes=0, **big) == E_WORKSPACE
    assert _call(hip, host, x=GARBAGE, kx=1, xscales=GARBAGE, T=4, ws_bytes=0, **big) == E_WORKSPACE       # 32768 samples
    assert _call(hip, host, x=GARBAGE, kx=1, xscales=GARBAGE, T=2, ws_bytes=0, M=65535 * 2, F=2, O=2) == E_WORKSPACE
    # operands not aligned to their element
    assert _call(hip, host, gy=GARBAGE + 1) == E_UNSUPPORTED
    assert _call(hip, host, x=GARBAGE + 1) == E_UNSUPPORTED
    assert _call(hip, host, gx=host.gx.ctypes.data + 1) == E_UNSUPPORTED
    assert _call(hip, host, gx=host.gx.ctypes.data + 2, gx_dtype=F32) == E_UNSUPPORTED
    assert host.untouched()


def test_python_wrapper_checks_operands_on_the_host(hip):
    m, f, o, t = 12, 40, 70, 3
    gy = torch.zeros((m, o), dtype=torch.bfloat16)
    x = torch.zeros((m, f), dtype=torch.bfloat16)
    wbits = torch.zeros((2 * 1 * 80,), dtype=torch.int64)           # [kw = 2][ceil(40 / 64)][ceil16(70)]
    wsc = torch.ones((2, o), dtype=torch.float32)
    xsc = torch.ones((1, m // t), dtype=torch.float32)
    fn = hip.linear_signw_dgrad_half
    with pytest.raises(TypeError, match='bfloat16 or float16'):
        fn(gy.float(), wbits, wsc, m, f, o)
    with pytest.raises(TypeError, match='out_dtype'):
        fn(gy, wbits, wsc, m, f, o, out_dtype=torch.float16)
    with pytest.raises(TypeError, match="gy's type"):
        fn(gy, wbits, wsc, m, f, o, x.half(), xsc, T=t)
    with pytest.raises(TypeError, match='float32'):
        fn(gy, wbits, wsc.half(), m, f, o)
    with pytest.raises(TypeError, match='float32'):
        fn(gy, wbits, wsc, m, f, o, x, xsc.double(), T=t)
    with pytest.raises(TypeError, match='int64'):
        fn(gy, wbits.int(), wsc, m, f, o)
    with pytest.raises(ValueError, match='xscales without x'):
        fn(gy, wbits, wsc, m, f, o, None, xsc)
    with pytest.raises(ValueError, match='cuda device'):          # CPU tensors: the kernel reads device memory only
        fn(gy, wbits, wsc, m, f, o, x, xsc, T=t)
    with pytest.raises(ValueError, match='contiguous'):
        fn(gy, wbits, torch.ones((2, 2 * o))[:, ::2], m, f, o)
    with pytest.raises(ValueError, match='bad sizes'):
        fn(gy, wbits, wsc, m + 1, f, o)
    with pytest.raises(ValueError, match='bad sizes'):
        fn(gy, wbits, wsc, m, f, o, x[:-1], xsc, T=t)
    with pytest.raises(ValueError, match='bad sizes'):              # M % T != 0
        fn(gy, wbits, wsc, m, f, o, x, xsc, T=5)
    with pytest.raises(ValueError, match='bad sizes'):
        fn(gy, wbits, wsc, m, f, o, x, xsc, T=0)
    with pytest.raises(ValueError, match='do not match'):         # planes of another plane count
        fn(gy, wbits, torch.ones((1, o)), m, f, o)
    with pytest.raises(ValueError, match='do not match'):         # scales of another sample count
        fn(gy, wbits, wsc, m, f, o, x, torch.ones((1, m)), T=t)
    with pytest.raises(ValueError, match='do not match'):
        fn(gy, wbits, wsc, m, f, o, x, torch.ones((9, m // t)), T=t)
    n = hip.LINEAR_DGRAD_HALF_MAX_SAMPLES + 1
    with pytest.raises(ValueError, match='do not match'):         # lsq_ste_backward's limit
        fn(torch.zeros((n, 1), dtype=torch.bfloat16), torch.zeros((16,), dtype=torch.int64), torch.ones((1, 1)), n, 1, 1,
           torch.zeros((n, 1), dtype=torch.bfloat16))


# ---------------------------------------------------------------------------------------- hip_train_linear.supported
class _DeviceTensor:
    """What ``supported`` reads of its input, claiming to live on a GPU: the clauses can be reached on the host."""
    is_cuda = True

    def __init__(self, shape, dtype):
        self.shape, self.dtype = torch.Size(shape), dtype

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))


class _OnDevice(torch.nn.Parameter):
    """A CPU parameter that claims to live on a GPU (``supported`` asks the weight too)."""
    is_cuda = True

    def __new__(cls, p):
        return torch.nn.Parameter.__new__(cls, p.data, p.requires_grad)


def _module(c, half=True):
    lin = L.make_module(c)
    lin.hip_train_half = half
    lin.weight = _OnDevice(lin.weight)
    return lin


def test_the_switch_is_off_by_default_and_a_class_attribute():
    from quant.binary.binary_linear import QuantLinear
    assert QuantLinear.hip_train_half is False and 'hip_train_half' in vars(QuantLinear)
    assert QuantLinear.hip_train is False and QuantLinear.act_half_solve is False


@pytest.mark.parametrize('dtype', L.DTYPES, ids=lambda t: L.DTYPE_NAMES[t])
def test_supported_takes_16_bit_inputs_with_the_switch_only(hip, dtype):
    from quant.binary import hip_train_linear
    for c in L.CASES:
        lin, x = _module(c, half=False), _DeviceTensor(L.x_shape(c), dtype)
        assert not hip_train_linear.supported(lin, x), c.id
        lin.hip_train = True                          # (fp32 inputs' switch: it does not bring the 16-bit step)
        assert not hip_train_linear.supported(lin, x), c.id
        lin.hip_train = False
        lin.hip_train_half = True                     # free-running ls-2 / ls-T included: act_half_solve is an eval switch
        assert not lin.act_half_solve and hip_train_linear.supported(lin, x), c.id
        assert not hip_train_linear.supported(lin, L.inputs(c.id, dtype)['x']), c.id      # a CPU tensor


def test_what_stays_refused_with_the_switch_on(hip):
    from quant.binary import hip_train_linear
    from quant.binary.binary_linear import QuantLinear

    def lin(xs='ls-1', ws='ls-1', f=64, **kw):
        m = QuantLinear(xs, ws, f, 16, dict(L.SYM2), **kw).train()
        m.hip_train_half = True
        m.weight = _OnDevice(m.weight)
        return m
    x = _DeviceTensor((4, 3, 64), torch.bfloat16)
    assert hip_train_linear.supported(lin(), x) and hip_train_linear.supported(lin('fp'), x)
    assert hip_train_linear.supported(lin('ls-2'), x) and hip_train_linear.supported(lin('ls-T'), x)
    assert not hip_train_linear.supported(lin(ws='fp'), x)
    assert not hip_train_linear.supported(lin(ws='gf-9'), x) and not hip_train_linear.supported(lin('gf-9'), x)
    half = lin()
    half.weight = _OnDevice(torch.nn.Parameter(half.weight.data.half()))
    assert not hip_train_linear.supported(half, x)                                     # 16-bit weights
    assert not hip_train_linear.supported(lin(), _DeviceTensor((4, 3, 64), torch.float64))
    assert not hip_train_linear.supported(lin(), _DeviceTensor((64,), torch.bfloat16))
    assert not hip_train_linear.supported(lin(), _DeviceTensor((4, 3, 32), torch.bfloat16))
    assert not hip_train_linear.supported(lin(f=96), _DeviceTensor((4, 3, 96), torch.bfloat16))     # T > 1, F % 64 != 0
    assert hip_train_linear.supported(lin('fp', f=96), _DeviceTensor((4, 3, 96), torch.bfloat16))
    # lsq_ste_backward's limit: N = 65536 samples are refused, binary and fp activations alike, on the host
    assert hip_train_linear.supported(lin(), _DeviceTensor((65535, 64), torch.bfloat16))
    assert not hip_train_linear.supported(lin(), _DeviceTensor((65536, 64), torch.bfloat16))
    assert not hip_train_linear.supported(lin('fp'), _DeviceTensor((65536, 64), torch.float16))
    # (the autocast rule needs a GPU to be switched on: tests/test_gpu_linear_train_half.py)
    # the fp32 step's rule is what it was
    off = lin()
    off.hip_train_half = False
    assert hip_train_linear.supported(off, _DeviceTensor((4, 3, 64), torch.float32)) and not hip_train_linear.supported(off, x)


@pytest.mark.parametrize('xs', ['ls-2', 'fp'])
def test_a_cpu_train_step_stays_the_torch_formulation(xs):
    from quant.binary.binary_linear import QuantLinear
    lin = QuantLinear(xs, 'ls-1', 64, 16, dict(L.SYM2)).train()
    lin.hip_train_half = True
    x = torch.randn(4, 3, 64, generator=torch.Generator().manual_seed(3)).requires_grad_()
    y = lin(x)
    assert type(y.grad_fn).__name__ not in ('_QuantLinearStepBackward', '_QuantLinearStepHalfBackward')
    assert torch.equal(y, lin._forward_torch(x))
    y.sum().backward()
    assert x.grad is not None and lin.weight.grad is not None


# ------------------------------------------------------------------------------------------------------ the table
def test_the_table_reaches_every_kernel_and_scheme():
    assert [c.id for c in L.CASES] == ['one_product', 'ragged', 'odd_rows', 'lenet_fc1', 'rows_per_sample', 'tiles64_ragged',
                                       'tiles64_t4', 'tiles128']
    for c in L.CASES:
        assert L.tile_class(c) == c.kernel, c.id
        assert c.T == 1 or c.xs == 'fp' or c.F % 64 == 0, c.id
    assert [(c.N, c.T, c.F, c.O) for c in L.CASES] == [(1, 1, 1, 1), (7, 1, 33, 65), (3, 1, 35, 63), (64, 1, 800, 10),
                                                       (3, 5, 64, 130), (1000, 1, 1033, 65), (250, 4, 1024, 64),
                                                       (2100, 1, 2000, 130)]
    assert {c.kernel for c in L.CASES} == {'split', 'small', 'big'}
    assert {c.xs for c in L.CASES} == {'fp', 'ls-1', 'ls-2', 'ls-T', 'gf-3'}
    assert {c.ws for c in L.CASES} == {'ls-1', 'ls-2', 'gf-3', 'gf-8'}
    assert any(L.alpha_of(c.clamp) < 0 for c in L.CASES) and any(not c.bias for c in L.CASES)
    odd = L.BY_ID['odd_rows']
    assert odd.F % 2 == 1 and odd.O % 2 == 1
    rows = L.BY_ID['rows_per_sample']
    assert rows.T > 1 and 32 % rows.T != 0 and rows.N * rows.T < 32                  # sample boundaries inside one 32-row tile
    assert len(L.PAIRS) == 16 and len({L.pair_id(p) for p in L.PAIRS}) == 16


@pytest.mark.parametrize('pair', L.PAIRS, ids=L.pair_id)
def test_inputs_are_values_of_the_type_with_the_special_values_in_place(pair):
    c, dtype = pair
    d = L.inputs(c.id, dtype)
    x, gy, alpha = d['x'], d['gy'], d['alpha']
    assert x.dtype == dtype and gy.dtype == dtype and d['w'].dtype == torch.float32
    assert tuple(x.shape) == L.x_shape(c) and tuple(gy.shape) == L.gy_shape(c) and tuple(d['w'].shape) == (c.O, c.F)
    assert alpha == L.alpha_of(c.clamp) and len(d['xscales']) == L.planes(c.xs)
    assert all(tuple(v.shape) == (c.N,) for v in d['xscales'])
    assert tuple(L.weight_scales(c.id).shape) == (L.planes(c.ws), c.O)
    flat = x.view(-1).float()
    if flat.numel() < 64:
        return
    assert bool((flat == 0).any()) and bool(torch.signbit(flat[flat == 0]).any()) and bool((flat == 1).any())
    assert bool((flat == -1).any())
    if alpha >= 0:                                    # each clamped case holds elements exactly at +-alpha
        assert bool((flat == alpha).any()) and bool((flat == -alpha).any())
        assert bool((flat.abs() > alpha).any())       # ... and some the clamp cuts off
    xs = d['xscales']
    m = L.step64(c, dtype, xs, list(L.weight_scales(c.id)))['m_x']
    if xs or alpha >= 0:                              # where an estimator or a clamp exists: neither all-open nor all-closed
        assert bool((m == 0).any()) and bool((m != 0).any()), c.id
    else:
        assert bool((m == 1).all())
    if len(xs) >= 2:                                  # an element on each side of the second sign's edge, one step of the type apart
        v1 = float(xs[0][0])
        e = L.edge_of(c, v1, dtype)
        assert e > 0, (c.id, v1)
        lo, hi = L.edge_pair(c, v1, dtype)
        assert lo <= e <= hi and (alpha < 0 or hi <= alpha)
        row0 = x[0].reshape(-1).float()
        assert bool((row0 == lo).any()) and bool((row0 == hi).any()) and bool((row0 == -lo).any()) and bool((row0 == -hi).any())
        assert len(d['edge_idx']) >= 4 and all(i % 3 for i in d['edge_idx'])          # the act_skip = 3 sub-sample does not read them
        d1 = (row0.clamp(-alpha, alpha) if alpha >= 0 else row0) - v1 * torch.where(row0 >= 0, 1.0, -1.0)
        is_open = d1.abs() <= 1
        placed = torch.zeros_like(is_open)
        placed[d['edge_idx']] = True
        assert bool(is_open[placed].any()) and bool((~is_open[placed]).any()), (c.id, v1, e, lo, hi)


def test_shifted_views_start_one_element_into_their_buffers():
    t = L.inputs('odd_rows', torch.bfloat16)['x']
    buf, view = L.shifted(t)
    assert view.data_ptr() == buf.data_ptr() + 2 and view.is_contiguous() and torch.equal(view, t)


@pytest.mark.parametrize('cid', ['ragged', 'rows_per_sample'])
def test_step64_agrees_with_fp64_autograd_of_the_torch_formulation(cid):
    """The reference against autograd through the torch formulation in fp64 on the same (rounded) values: the module's own
    scales, fp64 throughout."""
    c, dtype = L.BY_ID[cid], torch.float16
    d = L.inputs(c.id, dtype)
    lin = L.make_module(c).double()
    x = d['x'].double().requires_grad_()
    y = lin._forward_torch(x)
    y.backward(d['gy'].double())
    wsc = lin.w_approximate.plane_scales().detach().float()
    xsc = [v.float() for v in L.act_scales_cpu(c, d['x'].float())]
    ref = L.step64(c, dtype, xsc, list(wsc))
    for name, t in (('y', y), ('gx', x.grad), ('gw', lin.weight.grad), ('gb', lin.bias.grad)):
        err = float((t.detach().double() - ref[name]).abs().max() / ref[name].abs().max())
        assert err <= 1e-5, (name, err)
    assert torch.allclose(ref['gx'], ref['m_x'] * ref['gxq'], rtol=1e-12, atol=0)     # the estimator is a multiplier (fp64 rounding apart)
