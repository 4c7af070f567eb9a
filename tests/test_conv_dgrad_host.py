"""The C ABI of liblsq_hip_conv_train.so on the host (no GPU): header, exports, the plan of every case of
tests/golden/conv_dgrad_cases.py, the workspace formula, argument errors returned before any launch, the Python wrapper's
operand checks, the missing-library error, ``hip_train.supported`` under both settings of DGRAD_KERNEL, the conditions the
table must meet, and the fp64 reference of the new cases against fp32 autograd through the torch formulation."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import conv_dgrad_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'lsq_hip_conv_train.h')
E_NULL, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5, -6
NARROW, WIDE, PATCH = 1, 2, 4
TOL = 1e-5            # fp32 reassociation only: the figure of tests/test_train_step_cases_host.py
ENTRY_POINTS = ['lsq_conv_train_abi_version', 'lsq_signw_conv2d_dgrad', 'lsq_signw_conv2d_dgrad_plan',
                'lsq_signw_conv2d_dgrad_workspace_bytes']
NEW = [D.BY_ID[i] for i in D.NEW_IDS]


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', open(header).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.conv_train_library_path()):
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
    assert re.search(r'#define\s+LSQ_CONV_TRAIN_ABI_VERSION\s+1\b', text)


def test_the_library_builds_and_loads(hip):
    import __graft_entry__
    assert 'conv_train' in [s[0] for s in __graft_entry__.SUBLIBS]
    assert os.path.exists(hip.conv_train_library_path())
    assert hip.conv_train_lib().lsq_conv_train_abi_version() == hip.CONV_TRAIN_ABI_VERSION == 1


def test_library_exports_exactly_the_declared_entry_points(hip):
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('no nm on this machine')
    out = subprocess.run([nm, '-D', '--defined-only', hip.conv_train_library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({line.split()[-1] for line in out.splitlines() if ' T ' in line and line.split()[-1].startswith('lsq_')})
    assert exported == ENTRY_POINTS


# ---------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize('case', D.CASES, ids=lambda c: c.id)
def test_plan_of_every_case(hip, case):
    plan = hip.signw_conv2d_dgrad_plan(_geom(hip, case))
    assert plan is not None and hip.signw_conv2d_dgrad_supported(_geom(hip, case))
    cl = D.classes(case)
    assert plan.tap_steps == case.KH * case.KW == sum(cl.values())
    assert plan.classes == case.stride_h * case.stride_w == len(cl)
    assert plan.dead_classes == sum(1 for n in cl.values() if n == 0)
    assert plan.kernel == (WIDE if D.wide(case) else NARROW) | (PATCH if D.patch_positions(case) is not None else 0)


def test_every_kernel_is_reached_and_the_dead_classes_are_the_expected_ones(hip):
    reached = {hip.signw_conv2d_dgrad_plan(_geom(hip, c)).kernel for c in D.CASES}
    assert reached == {NARROW, WIDE, NARROW | PATCH, WIDE | PATCH}
    kernel = {c.id: hip.signw_conv2d_dgrad_plan(_geom(hip, c)).kernel for c in D.CASES}
    assert kernel['base3x3'] == NARROW | PATCH and kernel['c130_gf3'] == WIDE | PATCH
    assert kernel['k5_many'] == NARROW and kernel['k8x8'] == WIDE          # 12 x 20 and 15 x 23 positions at the least
    dead = {c.id: hip.signw_conv2d_dgrad_plan(_geom(hip, c)).dead_classes for c in D.CASES}
    assert dead['s3_2x2'] == 5 and dead['s3_3x3'] == 0 and dead['dil2x1_s2'] == 2 and dead['o520_proj'] == 3
    assert dead['h1_s2'] == 2 and dead['base3x3'] == 0


def _need(hip, c, kw, **changes):
    return int(hip.conv_train_lib().lsq_signw_conv2d_dgrad_workspace_bytes(ctypes.byref(_geom(hip, c, **changes)), kw))


def test_workspace_size(hip):
    # the transposed plane image: kw * taps * groups * ceil(og / 64) * ceil16(cg) words
    for c in D.CASES:
        cg, og = c.C // c.groups, c.O // c.groups
        for kw in (1, D.planes(c.ws)):
            assert _need(hip, c, kw) == kw * c.KH * c.KW * c.groups * ((og + 63) // 64) * ((cg + 15) // 16 * 16) * 8, c.id
    c = D.BY_ID['g2_tails']
    assert _need(hip, c, 2) == 2 * 9 * 2 * 1 * 48 * 8
    assert _need(hip, c, 0) == 0 and _need(hip, c, 9) == 0 and _need(hip, c, 1, groups=5) == 0


# ----------------------------------------------------------------------------------------------------- argument errors
def _call(hip, c, gy=1 << 20, wbits=1 << 20, kw=1, wscales=1 << 20, gx=1 << 20, ws=1 << 20, ws_bytes=None, geom=True, **changes):
    if ws_bytes is None:
        ws_bytes = 1 << 40                        # (never touched: every call below fails its checks first)
    g = ctypes.byref(_geom(hip, c, **changes)) if geom else None
    return hip.conv_train_lib().lsq_signw_conv2d_dgrad(gy, wbits, kw, wscales, g, gx, ws, ws_bytes, None)


def test_argument_errors_return_before_a_launch(hip):
    # the pointers are never dereferenced on these paths: every call below must fail its checks first
    c = D.BY_ID['g2_tails']
    for name in ('gy', 'wbits', 'wscales', 'gx'):
        assert _call(hip, c, **{name: None}) == E_NULL, name
    assert _call(hip, c, geom=False) == E_NULL
    for bad in (dict(N=0), dict(C=-8), dict(KH=0), dict(stride_w=0), dict(dil_h=0), dict(pad_w=-1), dict(groups=0),
                dict(groups=5), dict(H=1, pad_h=0), dict(W=2, dil_w=3, pad_w=0)):
        assert _call(hip, c, **bad) == E_SHAPE, bad
        plan = hip.ConvDgradPlan()
        assert hip.conv_train_lib().lsq_signw_conv2d_dgrad_plan(ctypes.byref(_geom(hip, c, **bad)), ctypes.byref(plan)) == E_SHAPE
    for bad in (dict(kw=0), dict(kw=9), dict(kw=-1), dict(N=1 << 20, H=64, W=64), dict(stride_h=256, stride_w=256),
                dict(groups=1, C=1 << 24, H=1, W=1, pad_h=1, pad_w=1, N=1)):
        assert _call(hip, c, **bad) == E_UNSUPPORTED, bad
    lib = hip.conv_train_lib()
    assert lib.lsq_signw_conv2d_dgrad_plan(None, ctypes.byref(hip.ConvDgradPlan())) == E_NULL
    assert lib.lsq_signw_conv2d_dgrad_plan(ctypes.byref(_geom(hip, c)), None) == E_NULL
    need = _need(hip, c, 1)
    assert need > 0
    assert _call(hip, c, ws_bytes=need - 1) == E_WORKSPACE
    assert _call(hip, c, ws_bytes=0) == E_WORKSPACE
    assert _call(hip, c, ws=None) == E_WORKSPACE
    assert _call(hip, c, ws=(1 << 20) + 4) == E_WORKSPACE          # misaligned
    assert _call(hip, c, kw=2, ws_bytes=need) == E_WORKSPACE       # two planes need twice the image


def test_python_wrapper_checks_operands_on_the_host(hip):
    c = D.BY_ID['g2_tails']
    geom = _geom(hip, c)
    ho, wo = D.out_hw(c)
    gy = torch.zeros((c.N, c.O, ho, wo), dtype=torch.float32)
    words = 9 * 1 * 2 * 32
    wbits = torch.zeros((2 * words,), dtype=torch.int64)
    wsc = torch.ones((2, c.O), dtype=torch.float32)
    with pytest.raises(TypeError):
        hip.signw_conv2d_dgrad(gy.double(), wbits, wsc, geom)
    with pytest.raises(TypeError):
        hip.signw_conv2d_dgrad(gy, wbits.int(), wsc, geom)
    with pytest.raises(TypeError):
        hip.signw_conv2d_dgrad(gy, wbits, wsc.half(), geom)
    with pytest.raises(ValueError, match='cuda device'):          # CPU tensors: the kernel reads device memory only
        hip.signw_conv2d_dgrad(gy, wbits, wsc, geom)
    with pytest.raises(ValueError, match='contiguous'):
        hip.signw_conv2d_dgrad(torch.zeros((c.N, c.O, ho, 2 * wo))[..., ::2], wbits, wsc, geom)
    with pytest.raises(ValueError, match='do not match'):         # a gradient of another geometry
        hip.signw_conv2d_dgrad(gy, wbits, wsc, _geom(hip, c, stride_h=2))
    with pytest.raises(ValueError, match='do not match'):         # planes of another plane count
        hip.signw_conv2d_dgrad(gy, wbits, torch.ones((1, c.O)), geom)
    with pytest.raises(ValueError, match='do not match'):
        hip.signw_conv2d_dgrad(gy, wbits, torch.ones((2, c.O + 1)), geom)
    with pytest.raises(ValueError, match='do not match'):         # planes packed for groups 1
        hip.signw_conv2d_dgrad(gy, torch.zeros((2 * 9 * 2 * 48,), dtype=torch.int64), wsc, geom)
    with pytest.raises(ValueError, match='bad sizes'):
        hip.signw_conv2d_dgrad(gy[0], wbits, wsc, geom)
    with pytest.raises(ValueError, match='bad sizes'):
        hip.signw_conv2d_dgrad(gy, wbits, torch.ones((9, c.O)), geom)


def test_a_missing_library_is_an_error(hip, monkeypatch, tmp_path):
    monkeypatch.setattr(hip, '_LIB_DIR', str(tmp_path))              # (where the libraries are looked for: none is there)
    monkeypatch.delitem(hip._handles, 'conv_train', raising=False)
    assert hip.conv_train_library_path() == str(tmp_path / 'liblsq_hip_conv_train.so')
    with pytest.raises(hip.LsqHipError, match='csrc/conv_train'):
        hip.conv_train_lib()
    with pytest.raises(hip.LsqHipError):
        hip.signw_conv2d_dgrad_supported(_geom(hip, D.BY_ID['g2_tails']))


# ------------------------------------------------------------------------------------------------- hip_train.supported
class _DeviceTensor:
    """What ``supported`` reads of its input, claiming to live on a GPU: the geometry clauses can be reached on the host."""
    is_cuda, dtype = True, torch.float32

    def __init__(self, shape):
        self.shape = torch.Size(shape)

    def dim(self):
        return len(self.shape)


def test_the_switch_is_off_by_default():
    from quant.binary import hip_train
    assert hip_train.DGRAD_KERNEL is False and hip_train.WGRAD_KERNEL is False


@pytest.mark.parametrize('on', [False, True], ids=['off', 'on'])
def test_supported_is_false_on_the_cpu(hip, monkeypatch, on):
    from quant.binary import hip_train
    monkeypatch.setattr(hip_train, 'DGRAD_KERNEL', on)
    for c in D.CASES:
        assert not hip_train.supported(D.make_module(c), D.inputs(c.id)['x']), c.id


WIDENED = ('g2_tails', 'depthwise', 'g3_wide_s2', 'dil2', 'dil2x1_s2', 's3_3x3', 's3_2x2', 's2x1', 's1x2', 'pad3x1', 'pad0x3')


def test_the_widened_geometries_need_the_switch(hip, monkeypatch):
    from quant.binary import hip_train
    assert set(WIDENED) <= set(D.NEW_IDS)
    for c in D.CASES:
        conv, x = D.make_module(c), _DeviceTensor((c.N, c.C, c.H, c.W))
        monkeypatch.setattr(hip_train, 'DGRAD_KERNEL', False)
        assert hip_train.supported(conv, x) == (c.id not in WIDENED), c.id
        monkeypatch.setattr(hip_train, 'DGRAD_KERNEL', True)
        assert hip_train.supported(conv, x), c.id


def test_what_stays_refused_with_the_switch_on(hip, monkeypatch):
    from quant.binary import hip_train
    from quant.binary.binary_conv import QuantConv2d
    monkeypatch.setattr(hip_train, 'DGRAD_KERNEL', True)
    x = _DeviceTensor((2, 8, 9, 8))
    plain = dict(padding=1)
    assert hip_train.supported(QuantConv2d('ls-1', 'ls-1', 8, 16, 3, dict(D.SYM2), **plain).train(), x)
    assert not hip_train.supported(QuantConv2d('ls-1', 'fp', 8, 16, 3, dict(D.SYM2), **plain).train(), x)
    assert not hip_train.supported(QuantConv2d('ls-1', 'ls-1', 8, 16, 3, dict(D.SYM2), padding=1, padding_mode='reflect').train(), x)
    assert not hip_train.supported(QuantConv2d('ls-1', 'ls-1', 8, 16, 3, dict(D.SYM2), padding='same').train(), x)
    half = _DeviceTensor((2, 8, 9, 8))
    half.dtype = torch.float16
    assert not hip_train.supported(QuantConv2d('ls-1', 'ls-1', 8, 16, 3, dict(D.SYM2), **plain).train(), half)
    assert not hip_train.supported(QuantConv2d('ls-1', 'ls-1', 8, 16, 3, dict(D.SYM2), **plain).train(), torch.zeros(2, 8, 9, 8))
    # an empty output is the plan's to refuse
    assert not hip_train.supported(QuantConv2d('ls-1', 'ls-1', 8, 16, 3, dict(D.SYM2), dilation=5).train(), x)


# ------------------------------------------------------------------------------------------------------ the table
def test_the_table_is_what_the_gpu_tests_need():
    import train_step_cases as T
    ids = [c.id for c in D.CASES]
    assert len(set(ids)) == len(ids)
    assert ids[:17] == [c.id for c in T.CASES] and len(T.CASES) == 17
    present = set()
    for c in D.CASES:
        ho, wo = D.out_hw(c)
        assert ho >= 1 and wo >= 1 and c.C % c.groups == 0 and c.O % c.groups == 0, c.id
        assert c.N <= 3 and ((c.H <= 20 and c.W <= 20) or (c.H, c.W) == (3, 260)), c.id
        assert c.O * (c.C // c.groups) * c.KH * c.KW <= 160_000, c.id
        present |= D.kinds(c)
    assert sum(1 for c in D.CASES if c.W > 20) == 1
    assert set(D.REQUIRED_KINDS) <= present, set(D.REQUIRED_KINDS) - present
    for c in D.LIFTED:                                # a lifted case is the old case: one stride, no dilation, one group
        t = T.BY_ID[c.id]
        assert (c.stride_h, c.stride_w, c.dil_h, c.dil_w, c.groups) == (t.stride, t.stride, 1, 1, 1)
        assert D.out_hw(c) == T.out_hw(t) and D.inputs(c.id) is T.inputs(c.id)
    assert {D.planes(c.ws) for c in NEW} >= {1, 2, 3} and 'ls-T' in {c.ws for c in NEW}
    assert {c.xs for c in NEW} >= {'fp', 'ls-1', 'ls-2', 'ls-T'}


def test_dead_row_class_leaves_exact_zero_rows():
    """dil2x1_s2: rows with (h + pad_h) odd are reached by no tap: the reference and its bound are exactly 0 there."""
    c = D.BY_ID['dil2x1_s2']
    d = D.inputs(c.id)
    conv = D.make_module(c)
    conv(d['x'])
    ref = D.step64(c, d['x'], d['w'], d['b'], d['gy'], [], list(conv.w_approximate.plane_scales()))
    rows = [h for h in range(c.H) if (h + c.pad_h) % 2 == 1]
    assert 2 <= len(rows) < c.H and any(0 < h < c.H - 1 for h in rows)
    assert float(ref['mag_x'][:, :, rows, :].abs().max()) == 0.0 and float(ref['gxq'][:, :, rows, :].abs().max()) == 0.0
    live = [h for h in range(c.H) if h not in rows]
    assert float(ref['mag_x'][:, :, live, :].min()) > 0.0


# --------------------------------------------------------------------------------------------- the reference itself
def _rel(a, b64):
    return float((a.detach().double() - b64).abs().max() / b64.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('case', NEW, ids=lambda c: c.id)
def test_step64_equals_fp32_autograd_through_the_torch_formulation(case):
    d = D.inputs(case.id)
    conv = D.make_module(case)
    x = d['x'].clone().requires_grad_()
    y = conv._forward_torch(x)
    assert tuple(y.shape) == tuple(d['gy'].shape)
    y.backward(d['gy'])
    wscales = list(conv.w_approximate.plane_scales())
    assert len(wscales) == D.planes(case.ws) and float(wscales[0].abs().min()) > 0
    xscales = D.act_scales_cpu(case, d['x'])
    assert len(xscales) == D.planes(case.xs)
    ref = D.step64(case, d['x'], d['w'], d['b'], d['gy'], xscales, wscales)
    got = {'y': y, 'gx': x.grad, 'gw': conv.weight.grad}
    if case.bias:
        got['gb'] = conv.bias.grad
    for name, t in got.items():
        assert t.shape == ref[name].shape, name
        err = _rel(t, ref[name])
        assert err <= TOL, (case.id, name, err)
    assert _rel(ref['m_x'] * ref['gxq'], ref['gx']) <= 1e-14 or float(ref['gx'].abs().max()) == 0.0
    assert bool((ref['gxq'].abs() <= ref['mag_x'] * (1 + 1e-12)).all())


@pytest.mark.parametrize('case', D.LIFTED[:3], ids=lambda c: c.id)
def test_step64_of_a_lifted_case_is_the_old_reference(case):
    import train_step_cases as T
    t = T.BY_ID[case.id]
    d = D.inputs(case.id)
    conv = D.make_module(case)
    conv(d['x'])
    ws, xs = list(conv.w_approximate.plane_scales()), D.act_scales_cpu(case, d['x'])
    a = D.step64(case, d['x'], d['w'], d['b'], d['gy'], xs, ws)
    b = T.step64(d['x'], d['w'], d['b'], d['gy'], xs, ws, T.alpha_of(t.clamp), t.stride, (t.pad_h, t.pad_w))
    for k in a:
        assert torch.equal(a[k], b[k]), k
