"""The C ABI of liblsq_hip_linear_wgrad_half.so on the host (no GPU): header, exports, ABI version, the SUBLIBS row, the
workspace size against the fp32 library, every refusal returned before a launch with nothing written, the Python wrapper's
operand checks, the WGRAD_HALF_KERNEL switch, the table of tests/golden/linear_wgrad_half_cases.py, the kernel's prescribed
arithmetic emulated on the CPU at every case (which is what fixes that file's seeds), and the shared headers as prerequisites
of the objects that include them."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import linear_wgrad_half_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ml-quant_amd', 'csrc')
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_linear_wgrad_half.h')
PATTERN = r'lsq_linear_wgrad_half_[a-z0-9_]+|lsq_linear_signx_wgrad_half[a-z0-9_]*'
E_NULL, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5, -6
F32, BF16, F16 = 0, 1, 2
ENTRY_POINTS = ['lsq_linear_signx_wgrad_half', 'lsq_linear_signx_wgrad_half_workspace_bytes', 'lsq_linear_wgrad_half_abi_version']


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not (os.path.exists(_hip.linear_wgrad_half_library_path()) and os.path.exists(_hip.linear_wgrad_library_path())
            and os.path.exists(_hip.linear_train_half_library_path())):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


# ------------------------------------------------------------------------------------------------- header and library
def test_header_declares_exactly_the_three_entry_points():
    assert declared_functions() == ENTRY_POINTS
    text = open(HEADER).read()
    assert re.search(r'#define\s+LSQ_LINEAR_WGRAD_HALF_ABI_VERSION\s+1\b', text)
    for inc in ('lsq_hip.h', 'lsq_hip_linear_half.h'):       # the error codes and LSQ_MAX_PLANES, LSQ_DTYPE_*
        assert f'#include "{inc}"' in text
    assert '(A)' in text and '(B)' in text                   # the two equalities are stated


def test_the_library_is_a_row_of_the_table():
    from quant import _hip, _sublibs
    row = _sublibs.BY_DIR['linear_wgrad_half']
    assert (row.header, row.version_symbol, row.version) == ('lsq_hip_linear_wgrad_half.h', 'lsq_linear_wgrad_half_abi_version', 1)
    assert row.pattern == PATTERN and sorted(row.prototypes) == ENTRY_POINTS
    assert os.path.exists(os.path.join(CSRC, 'linear_wgrad_half', 'Makefile'))
    assert _hip.LINEAR_WGRAD_HALF_ABI_VERSION == 1
    assert _hip.linear_wgrad_half_library_path().endswith(os.path.join('lib', 'liblsq_hip_linear_wgrad_half.so'))
    # the new row claims no other library's symbols, and no other header declares the new ones
    for other in _sublibs.SUBLIBS:
        if other.dir != 'linear_wgrad_half':
            assert not any(re.fullmatch(PATTERN, name) for name in other.prototypes), other.dir
            assert not set(declared_functions(os.path.join(ROOT, 'include', other.header))) & set(ENTRY_POINTS), other.header


def test_the_kernels_are_one_source_for_both_libraries():
    """The kernels live in a header beside the fp32 library's source; both sources include it and hold no kernel of their own;
    ste_one is written once for the libraries beside liblsq_hip.so that this change touches."""
    shared = open(os.path.join(CSRC, 'linear_wgrad', 'lsq_linear_wgrad_core.h')).read()
    for name in ('sign_image', 'wgrad_tiled', 'wgrad_split', 'struct Args', 'launch(', 'in_limits(', 'tile_rule('):
        assert name in shared, name
    assert 'atomic' not in shared.lower()
    for path in (('linear_wgrad', 'lsq_linear_wgrad.hip'), ('linear_wgrad_half', 'lsq_linear_wgrad_half.hip')):
        text = open(os.path.join(CSRC, *path)).read()
        assert 'lsq_linear_wgrad_core.h"' in text and '__global__' not in text and 'mfma(' not in text, path
        assert 'atomic' not in text.lower()
    ste = re.compile(r'float\s+ste_one\s*\(')
    assert len(ste.findall(open(os.path.join(CSRC, 'lsq_ste_one.h')).read())) == 1
    for path in (('linear_wgrad_half', 'lsq_linear_wgrad_half.hip'), ('linear_train_half', 'lsq_linear_train_half.hip')):
        text = open(os.path.join(CSRC, *path)).read()
        assert 'lsq_ste_one.h"' in text and not ste.search(text), path


def test_the_library_builds_and_loads(hip):
    assert os.path.exists(hip.linear_wgrad_half_library_path())
    assert hip.linear_wgrad_half_lib().lsq_linear_wgrad_half_abi_version() == hip.LINEAR_WGRAD_HALF_ABI_VERSION == 1
    assert hip.linear_wgrad_lib().lsq_linear_wgrad_abi_version() == hip.LINEAR_WGRAD_ABI_VERSION == 1      # (unchanged)


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm') or shutil.which('llvm-nm') or '/opt/rocm/llvm/bin/llvm-nm'
    for path, want in ((hip.linear_wgrad_half_library_path(), ENTRY_POINTS),
                       (hip.linear_wgrad_library_path(), ['lsq_linear_signx_wgrad', 'lsq_linear_signx_wgrad_workspace_bytes',
                                                          'lsq_linear_wgrad_abi_version'])):
        out = subprocess.run([nm, '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
        exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
        assert exported == want, path


def test_a_missing_library_is_an_error(hip, monkeypatch, tmp_path):
    monkeypatch.setattr(hip, '_LIB_DIR', str(tmp_path))              # (where the libraries are looked for: none is there)
    monkeypatch.delitem(hip._handles, 'linear_wgrad_half', raising=False)
    assert hip.linear_wgrad_half_library_path() == str(tmp_path / 'liblsq_hip_linear_wgrad_half.so')
    with pytest.raises(hip.LsqHipError, match='csrc/linear_wgrad_half'):
        hip.linear_wgrad_half_lib()


# ----------------------------------------------------------------------------------------------------- workspace size
def _refused(kx, n, t, f, o):
    return not (1 <= kx <= 8 and 0 < n <= 65535 and t > 0 and f > 0 and o > 0 and n * t < 1 << 31 and f < 1 << 22 and o < 1 << 21)


def test_workspace_size_equals_the_fp32_library(hip):
    f32, half = hip.linear_wgrad_lib(), hip.linear_wgrad_half_lib()
    args = [(H.planes(c.xs), c.N, c.T, c.F, c.O) for c in H.CASES]
    for kx in (0, 1, 2, 8, 9, -1):
        for n, t in ((1, 1), (64, 1), (65, 3), (65535, 1), (65536, 1), (65535, 1 << 16), (0, 1), (4, 0), (-1, 1)):
            for f in (1, 15, 17, 800, (1 << 22) - 1, 1 << 22, 0):
                for o in (1, 65, (1 << 21) - 1, 1 << 21, 0, -3):
                    args.append((kx, n, t, f, o))
    for a in args:
        got = int(half.lsq_linear_signx_wgrad_half_workspace_bytes(*a))
        assert got == int(f32.lsq_linear_signx_wgrad_workspace_bytes(*a)), a
        kx, n, t, f, o = a
        assert got == (0 if _refused(*a) else kx * ((n * t + 63) // 64) * ((f + 15) // 16 * 16) * 8), a
    for c in H.CASES:
        assert int(half.lsq_linear_signx_wgrad_half_workspace_bytes(H.planes(c.xs), c.N, c.T, c.F, c.O)) > 0, c.id


# ----------------------------------------------------------------------------------------------------- argument errors
class _Host:
    """Host buffers filled with sentinels stand in for out and the workspace: a refused call never dereferences a pointer (the
    other operands are garbage addresses) and leaves every byte as it was."""

    def __init__(self):
        self.out = np.full((1 << 16,), 12345.0, dtype=np.float32)
        self.ws = np.full((1 << 16,), -77.0, dtype=np.float32)
        self.keep = self.out.copy(), self.ws.copy()

    def untouched(self):
        return np.array_equal(self.out, self.keep[0]) and np.array_equal(self.ws, self.keep[1])


GARBAGE = 1 << 20


def _call(hip, host, gy=GARBAGE, x=GARBAGE, dtype=BF16, kx=1, xscales=GARBAGE, alpha=2.0, N=12, T=1, F=40, O=70, w=None, kw=0,
          wscales=None, out=True, ws=True, ws_bytes=None, ws_shift=0):
    out_ptr = host.out.ctypes.data if out is True else out
    ws_ptr = host.ws.ctypes.data + ws_shift if ws is True else ws
    ws_bytes = host.ws.nbytes if ws_bytes is None else ws_bytes
    return hip.linear_wgrad_half_lib().lsq_linear_signx_wgrad_half(gy, x, dtype, kx, xscales, alpha, N, T, F, O, w, kw, wscales,
                                                                   out_ptr, ws_ptr, ws_bytes, None)


def test_every_refusal_returns_before_a_launch_and_writes_nothing(hip):
    host = _Host()
    need = int(hip.linear_wgrad_half_lib().lsq_linear_signx_wgrad_half_workspace_bytes(1, 12, 1, 40, 70))
    assert 0 < 2 * need <= host.ws.nbytes
    with_w = dict(w=GARBAGE, kw=2, wscales=GARBAGE)
    for extra in ({}, with_w):
        for name in ('gy', 'x', 'xscales', 'out'):
            assert _call(hip, host, **dict(extra, **{name: None})) == E_NULL, name
        # those of lsq_linear_signx_wgrad
        for bad in (dict(N=0), dict(T=0), dict(F=0), dict(O=0), dict(N=-1), dict(F=-64), dict(O=-3)):
            assert _call(hip, host, **dict(extra, **bad)) == E_SHAPE, bad
        for bad in (dict(kx=0), dict(kx=9), dict(kx=-1), dict(N=65536), dict(F=1 << 22), dict(O=1 << 21),
                    dict(N=65535, T=1 << 16)):                    # (the last: M = N * T >= 2^31)
            assert _call(hip, host, **dict(extra, **bad)) == E_UNSUPPORTED, bad
        assert _call(hip, host, ws_bytes=need - 1, **extra) == E_WORKSPACE
        assert _call(hip, host, ws_bytes=0, **extra) == E_WORKSPACE
        assert _call(hip, host, ws=None, **extra) == E_WORKSPACE
        assert _call(hip, host, ws_shift=4, **extra) == E_WORKSPACE             # misaligned
        assert _call(hip, host, kx=2, ws_bytes=need, **extra) == E_WORKSPACE    # two planes need twice the image
        # the new ones: the type, operands not aligned to their element
        for dt in (F32, 3, -1, 7):
            assert _call(hip, host, dtype=dt, **extra) == E_UNSUPPORTED, dt
        assert _call(hip, host, gy=GARBAGE + 1, **extra) == E_UNSUPPORTED
        assert _call(hip, host, x=GARBAGE + 1, **extra) == E_UNSUPPORTED
        assert _call(hip, host, out=host.out.ctypes.data + 2, **extra) == E_UNSUPPORTED
        assert _call(hip, host, out=host.out.ctypes.data + 1, **extra) == E_UNSUPPORTED
    # the weight side
    assert _call(hip, host, w=GARBAGE, kw=1, wscales=None) == E_NULL
    for kw in (0, 9, -1, 100):
        assert _call(hip, host, w=GARBAGE, kw=kw, wscales=GARBAGE) == E_UNSUPPORTED, kw
        assert _call(hip, host, kw=kw, ws_bytes=0) == E_WORKSPACE, kw           # (without w: kw is ignored, the call goes on)
    assert _call(hip, host, w=GARBAGE + 2, kw=1, wscales=GARBAGE) == E_UNSUPPORTED
    assert _call(hip, host, w=GARBAGE, kw=1, wscales=GARBAGE + 2) == E_UNSUPPORTED
    assert _call(hip, host, wscales=GARBAGE + 2, ws_bytes=0) == E_WORKSPACE     # (ignored without w)
    assert host.untouched()


def test_python_wrapper_checks_operands_on_the_host(hip, monkeypatch):
    def no_library(*a):
        raise AssertionError('the library was touched before the operand checks')
    monkeypatch.setattr(hip, 'linear_wgrad_half_lib', no_library)
    n, t, f, o = 4, 3, 40, 6
    m = n * t
    gy = torch.zeros((m, o), dtype=torch.bfloat16)
    x = torch.zeros((m, f), dtype=torch.bfloat16)
    xs = torch.ones((2, n), dtype=torch.float32)
    w = torch.zeros((o, f), dtype=torch.float32)
    wsc = torch.ones((2, o), dtype=torch.float32)
    fn = hip.linear_signx_wgrad_half
    with pytest.raises(TypeError, match='bfloat16 or float16'):
        fn(gy.float(), x.float(), xs, 2.0, n, t, f, o)
    with pytest.raises(TypeError, match="gy's type"):
        fn(gy, x.half(), xs, 2.0, n, t, f, o)
    with pytest.raises(TypeError, match="gy's type"):
        fn(gy, x.float(), xs, 2.0, n, t, f, o)
    with pytest.raises(TypeError, match='float32'):
        fn(gy, x, xs.double(), 2.0, n, t, f, o)
    with pytest.raises(TypeError, match='float32'):
        fn(gy, x, xs, 2.0, n, t, f, o, w.bfloat16(), wsc)
    with pytest.raises(TypeError, match='float32'):
        fn(gy, x, xs, 2.0, n, t, f, o, w, wsc.half())
    with pytest.raises(ValueError, match='go together'):
        fn(gy, x, xs, 2.0, n, t, f, o, w)
    for weight in ((), (w, wsc)):
        with pytest.raises(ValueError, match='cuda device'):          # CPU tensors: the kernel reads device memory only
            fn(gy, x, xs, 2.0, n, t, f, o, *weight)
        with pytest.raises(ValueError, match='contiguous'):
            fn(torch.zeros((m, 2 * o), dtype=torch.bfloat16)[:, ::2], x, xs, 2.0, n, t, f, o, *weight)
        with pytest.raises(ValueError, match='contiguous'):
            fn(gy, torch.zeros((m, 2 * f), dtype=torch.bfloat16)[:, ::2], xs, 2.0, n, t, f, o, *weight)
        with pytest.raises(ValueError, match='bad sizes'):
            fn(gy, x, xs, 2.0, n + 1, t, f, o, *weight)
        with pytest.raises(ValueError, match='bad sizes'):
            fn(gy, x, xs, 2.0, n, t, f + 1, o, *weight)
        with pytest.raises(ValueError, match='bad sizes'):
            fn(gy, x, xs, 2.0, n, 0, f, o, *weight)
        with pytest.raises(ValueError, match='do not match'):         # per-row scales where the rows share a sample's
            fn(gy, x, torch.ones((2, m)), 2.0, n, t, f, o, *weight)
        with pytest.raises(ValueError, match='do not match'):
            fn(gy, x, torch.ones((n,)), 2.0, n, t, f, o, *weight)
    with pytest.raises(ValueError, match='contiguous'):
        fn(gy, x, xs, 2.0, n, t, f, o, torch.zeros((o, 2 * f))[:, ::2], wsc)
    with pytest.raises(ValueError, match='bad sizes'):
        fn(gy, x, xs, 2.0, n, t, f, o, torch.zeros((o + 1, f)), wsc)
    with pytest.raises(ValueError, match='do not match'):             # scales of another output count / plane count
        fn(gy, x, xs, 2.0, n, t, f, o, w, torch.ones((2, o + 1)))
    with pytest.raises(ValueError, match='do not match'):
        fn(gy, x, xs, 2.0, n, t, f, o, w, torch.ones((9, o)))
    with pytest.raises(TypeError):                                    # the fp32 wrapper stays fp32-only
        hip.linear_signx_wgrad(gy.float(), x, xs, 2.0, n, t, f, o)


def test_the_switch_is_off_by_default():
    from quant.binary import hip_train_linear
    assert hip_train_linear.WGRAD_HALF_KERNEL is False and hip_train_linear.WGRAD_KERNEL is False


# ------------------------------------------------------------------------------------------------------ the table
def test_the_table_is_the_stated_one_and_reaches_every_kernel_class():
    assert [(c.N, c.T, c.F, c.O, c.xs) for c in H.CASES] == H.SHAPES
    assert len(H.PAIRS) == 24 and len({H.pair_id(p) for p in H.PAIRS}) == 24
    for c in H.CASES:
        assert H.tile_class(c) == c.kernel, c.id
        rows, cols = c.O, c.F                          # tile_rule(O, F) of csrc/linear/lsq_signw_mma.h, written out
        split = ((rows + 63) // 64) * ((cols + 63) // 64) < 256
        big = ((rows + 127) // 128) * ((cols + 127) // 128) >= 256
        assert ('split' if split else 'big' if big else 'small') == c.kernel, c.id
    assert [c.kernel for c in H.CASES] == ['split'] * 7 + ['small'] * 3 + ['big'] * 2
    assert [c.ws for c in H.CASES] == ['ls-1', 'ls-2', 'ls-T', 'gf-3'] * 3
    assert {c.xs for c in H.CASES} == {'ls-1', 'ls-2', 'ls-T', 'gf-2', 'gf-3', 'gf-8'}
    odd = H.BY_ID['odd_rows']
    assert odd.F % 2 == 1 and odd.O % 2 == 1
    rows = H.BY_ID['rows_per_sample']
    assert rows.T > 1 and 16 % rows.T != 0                           # sample boundaries inside a 16-row step
    long_m = H.BY_ID['long_m']
    assert ((long_m.N + 63) // 64) * 4 == 260 and long_m.N % 64 == 4
    for cid, vec in (('tiles64_vec', True), ('tiles64_ragged', False), ('tiles128', True), ('tiles128_ragged', False)):
        assert (H.BY_ID[cid].O % 4 == 0) == vec


@pytest.mark.parametrize('pair', H.PAIRS, ids=H.pair_id)
def test_inputs_are_values_of_the_type_with_the_special_values_in_place(pair):
    c, dtype = pair
    d = H.inputs(c.id, dtype)
    m = c.N * c.T
    assert d['gy'].dtype == dtype and d['x'].dtype == dtype and d['w'].dtype == d['ws'].dtype == d['xs'].dtype == torch.float32
    assert tuple(d['gy'].shape) == (m, c.O) and tuple(d['x'].shape) == (m, c.F) and tuple(d['w'].shape) == (c.O, c.F)
    assert tuple(d['xs'].shape) == (H.planes(c.xs), c.N) and tuple(d['ws'].shape) == (H.planes(c.ws), c.O)
    assert bool((d['xs'] > 0).all()) and bool((d['ws'] >= 0).all()) and float(d['ws'].max()) > 0
    flat = d['x'].reshape(-1).float()
    if flat.numel() < 64:
        return
    assert bool((flat == 0).any()) and bool(torch.signbit(flat[flat == 0]).any()) and not bool(torch.signbit(flat[flat == 0]).all())
    for v in (1.0, -1.0, H.ALPHA, -H.ALPHA):
        assert bool((flat == v).any()), v
    assert bool((flat > H.ALPHA).any()) and bool((flat < -H.ALPHA).any())
    if H.planes(c.xs) >= 2:                           # an element on each side of the second sign's edge, one step of the type apart
        v1 = float(d['xs'][0][0])
        lo, hi = H.L.edge_pair(c, v1, dtype)
        row0 = d['x'].reshape(c.N, -1)[0].float()
        assert len(d['edge_idx']) >= 4
        for v in (lo, hi, -lo, -hi):
            assert bool((row0 == v).any()), (c.id, v)


# ------------------------------------------------------------------------------------------- the prescribed arithmetic
def test_prescribed_arithmetic_stays_inside_half_the_bound():
    """For every (case, type): the signs of the fp32 chain on float(x), the 16-bit gy widened exactly, a = fl32(gy xs),
    hi = bf16(a), lo = bf16(a - hi) -- the kernel's operands -- summed EXACTLY (fp64) against the fp64 reference.  What the split
    alone costs has to stay within half of the bound the kernel is held to, so that the GPU test measures the kernel and not a
    draw in which max |ref| cancels; SEED_BASE is the first of 0, 1000, 2000, ... for which that holds everywhere (measured
    here: worst 3.7e-6 of max |ref|)."""
    assert H.SEED_BASE % 1000 == 0 and H.BOUND == 1e-5
    worst = 0.0
    for c, dtype in H.PAIRS:
        d = H.inputs(c.id, dtype)
        ref = H.ref_a(c, d)
        scale = ref.abs().max().item()
        assert scale > 0
        err = (H.emulated64(c, d) - ref).abs().max().item()
        worst = max(worst, err / scale)
        assert err <= 0.5 * H.BOUND * scale, (H.pair_id((c, dtype)), err / scale)
    print(f'prescribed arithmetic, worst case: {worst:.3e} of max |ref|')


def test_the_estimator_reference_is_the_fp64_autograd_of_the_weight_chain():
    """ref_b against autograd through the weight quantizer's chain written in fp64 torch (sign through a straight-through
    estimator with |d| <= 1), on one case with two planes."""
    c = H.BY_ID['ragged']
    d = H.inputs(c.id, torch.float16)
    a = H.ref_a(c, d)
    w = d['w'].double().requires_grad_()
    r = torch.zeros_like(w)
    for v in d['ws'].double():
        dd = w - r
        is_open = (dd.detach().abs() <= 1).double()
        sign = torch.where(dd.detach() >= 0, 1.0, -1.0).double()
        r = r + v.view(-1, 1) * (sign + dd * is_open - (dd * is_open).detach())        # value: the sign; gradient: [|d| <= 1]
    r.backward(a)
    want = H.ref_b(d, a)
    assert float((w.grad - want).abs().max()) <= 1e-9 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------ the Makefiles
def _compile_lines(sub, header):
    subprocess.run(['make', '-C', os.path.join(CSRC, sub)], check=True, capture_output=True)     # (nothing to do after build())
    out = subprocess.run(['make', '-n', '-W', header, '-C', os.path.join(CSRC, sub)], check=True, capture_output=True,
                         text=True).stdout
    return [line for line in out.splitlines() if ' -c ' in line]


def test_the_shared_headers_are_prerequisites_of_the_objects_that_include_them(hip):
    core = os.path.join(CSRC, 'linear_wgrad', 'lsq_linear_wgrad_core.h')
    ste = os.path.join(CSRC, 'lsq_ste_one.h')
    mma = os.path.join(CSRC, 'linear', 'lsq_signw_mma.h')
    assert os.path.exists(core) and os.path.exists(ste)
    for header, subs in ((core, ('linear_wgrad', 'linear_wgrad_half')), (ste, ('linear_wgrad_half', 'linear_train_half')),
                         (mma, ('linear_wgrad', 'linear_wgrad_half'))):
        for sub in subs:
            lines = _compile_lines(sub, header)
            assert len(lines) == 1 and f'lsq_{sub}.hip' in lines[0] and f'{sub}_lsq_{sub}.o' in lines[0], (header, sub, lines)
    assert _compile_lines('linear_wgrad', ste) == [] and _compile_lines('linear_train', core) == []
    assert _compile_lines('train', core) == []
