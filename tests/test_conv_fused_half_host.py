"""lsq_signw_conv2d_fused_half (liblsq_hip_conv_fused_half.so) without a GPU: the library loads at ABI 1, its plan and
workspace size are lsq_signw_conv2d_half's for every geometry (the folded batch norm cannot change the plan), every refusal
returns its code before anything is dereferenced, the case table of tests/golden/conv_fused_half_cases.py covers every
variant on both kernel kinds, and QuantConv2d selects the new route only with its switches."""

import ctypes
import os

import numpy as np
import pytest
import torch

import conv_fused_half_cases as FC
import conv_half_cases as C
from quant.binary.binary_conv import ProjectionShortcut, QuantConv2d

E_NULL, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5, -6
F32, BF16, F16 = 0, 1, 2


@pytest.fixture(scope='module')
def hip():
    from quant import _hip
    if not os.path.exists(_hip.conv_fused_half_library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _hip


def _geom(hip, c):
    return hip.make_geom(c.N, c.C, c.H, c.W, c.O, c.KH, c.KW, c.stride, c.pad, c.dil, c.groups)


def test_the_library_loads_at_abi_one(hip):
    assert os.path.exists(hip.conv_fused_half_library_path())
    assert hip.conv_fused_half_lib().lsq_conv_fused_half_abi_version() == hip.CONV_FUSED_HALF_ABI_VERSION == 1
    import __graft_entry__
    row = [s for s in __graft_entry__.SUBLIBS if s[0] == 'conv_fused_half']
    assert len(row) == 1 and row[0][1:3] == ('conv_fused_half_lib', 'lsq_hip_conv_fused_half.h')


def test_plan_and_workspace_are_those_of_the_unfused_library(hip):
    fused, plain = hip.conv_fused_half_lib(), hip.conv_half_lib()
    geoms = [_geom(hip, c) for c in C.CASES]
    # 2048 channels a group: past the table of the fp32 patch kernel's folded batch norm (512 / 256 channels)
    geoms.append(hip.make_geom(2, 2048, 9, 9, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1))
    geoms.append(hip.make_geom(2, 4096, 9, 9, 128, 3, 3, (2, 2), (1, 1), (1, 1), 2))
    for c, g in zip(C.CASES, geoms):
        assert fused.lsq_signw_conv2d_fused_half_plan(ctypes.byref(g)) == c.plan, c.id
    for g in geoms:
        plan = fused.lsq_signw_conv2d_fused_half_plan(ctypes.byref(g))
        assert plan == plain.lsq_signw_conv2d_half_plan(ctypes.byref(g)) and plan >= 0
        for kw in (1, 2, 8):
            for ydt in (F32, BF16, F16):
                assert fused.lsq_signw_conv2d_fused_half_workspace_bytes(ctypes.byref(g), kw, ydt) \
                    == plain.lsq_signw_conv2d_half_workspace_bytes(ctypes.byref(g), kw, ydt)
    assert fused.lsq_signw_conv2d_fused_half_plan(ctypes.byref(geoms[-2])) & C.PATCH          # the fold would not fit a table
    assert fused.lsq_signw_conv2d_fused_half_plan(None) == E_NULL
    bad = hip.make_geom(2, 100, 7, 7, 64, 3, 3, (1, 1), (1, 1), (1, 1), 3)
    assert fused.lsq_signw_conv2d_fused_half_plan(ctypes.byref(bad)) == E_SHAPE
    assert fused.lsq_signw_conv2d_fused_half_workspace_bytes(ctypes.byref(bad), 2, BF16) == 0


def test_refusals_return_before_a_launch(hip):
    """Host buffers filled with a sentinel stand in for y and the workspace, every other pointer is a garbage address: a
    refused call dereferences nothing and leaves every byte as it was."""
    y = np.full((4 * 64 * 7 * 7,), 12345.0, dtype=np.float32)
    ws = np.full((4 * 64 * 7 * 7,), -77.0, dtype=np.float32)
    keep = y.copy(), ws.copy()
    fn = hip.conv_fused_half_lib().lsq_signw_conv2d_fused_half

    def geom(N=4, C=100, H=7, W=7, O=64, K=3, groups=1, pad=1, stride=1, dil=1):
        return hip.make_geom(N, C, H, W, O, K, K, (stride, stride), (pad, pad), (dil, dil), groups)

    def call(x=1 << 20, xdt=BF16, alpha=2.0, ps=None, pb=None, wb=1 << 21, k=1, sc=1 << 22, bias=None, g=None, act=0, slope=None,
             rpre=None, rpost=None, yp=y.ctypes.data, ydt=F32, w=ws.ctypes.data, wbytes=ws.nbytes, no_geom=False):
        gp = None if no_geom else ctypes.byref(g if g is not None else geom())
        return fn(x, xdt, alpha, ps, pb, wb, k, sc, bias, gp, act, slope, rpre, rpost, yp, ydt, w, wbytes, None)

    full = dict(ps=1 << 23, pb=1 << 24, act=3, slope=1 << 25, rpre=1 << 26, rpost=1 << 27)
    for extra in ({}, full):
        for xdt in (BF16, F16):
            kw = dict(xdt=xdt, **extra)
            for name in ('x', 'wb', 'sc', 'yp'):
                assert call(**kw, **{name: None}) == E_NULL, name
            assert call(**kw, no_geom=True) == E_NULL
            for g in (geom(N=0), geom(C=0), geom(K=0), geom(groups=0), geom(stride=0), geom(dil=0), geom(pad=-1),
                      geom(C=100, groups=3), geom(H=2, W=2, K=5, pad=1)):
                assert call(**kw, g=g) == E_SHAPE
            for g in (geom(N=1 << 11, C=1 << 10, H=32, W=32), geom(N=1 << 10, C=1, H=1 << 10, W=1 << 10, O=4, K=1, pad=0),
                      geom(N=1, C=1 << 18, H=1, W=1, O=1 << 16, K=1, pad=0),
                      geom(N=1, C=1 << 16, H=1, W=1, O=1 << 16, K=1, pad=0, groups=1 << 16)):
                assert call(**kw, g=g) == E_UNSUPPORTED
            for k in (0, -1, 9):
                assert call(**kw, k=k) == E_UNSUPPORTED, k
            for ydt in (F16 if xdt == BF16 else BF16, 3, -1):
                assert call(**kw, ydt=ydt) == E_UNSUPPORTED, ydt
            assert call(**kw, k=2, ydt=xdt, w=None) == E_WORKSPACE
            assert call(**kw, k=2, ydt=xdt, w=ws.ctypes.data + 2) == E_WORKSPACE
            assert call(**kw, k=2, ydt=xdt, wbytes=ws.nbytes - 1) == E_WORKSPACE
        for xdt in (F32, 3, -1):
            assert call(xdt=xdt, **extra) == E_UNSUPPORTED
    # the new operands: exactly one of the folded batch norm's arrays, a PReLU without slopes, an unknown act
    assert call(ps=1 << 23) == E_NULL and call(pb=1 << 24) == E_NULL
    assert call(act=2) == E_NULL and call(act=3) == E_NULL
    for act in (-1, 4, 100):
        assert call(act=act, slope=1 << 25) == E_UNSUPPORTED, act
    assert all(np.array_equal(a, b) for a, b in zip(keep, (y, ws)))


def test_case_table_covers_every_variant_on_both_kernel_kinds():
    assert len(FC.VARIANTS) == 6 and [v.id for v in FC.VARIANTS] == ['none', 'relu_pre', 'prelu1_post', 'preluC_both', 'relu_both',
                                                                     'id_pre']
    assert set(FC.VARIANT_OF) == {c.id for c in C.CASES} and len(C.CASES) == 20
    for i, c in enumerate(C.CASES):
        assert FC.VARIANT_OF[c.id] is FC.VARIANTS[i % 6]
    FC.check_coverage()
    # the batch-norm runs: channel index under groups, padded positions
    assert {'groups_dil', 'groups3_patch', 'cg1'} <= set(FC.VARIANT_OF)
    assert sum(1 for c in C.CASES if max(c.pad) > 0) >= 15
    for c in C.CASES:
        s, b = FC.folded_bn(c.id)
        assert s.shape == b.shape == (c.C,) and s.dtype == b.dtype == torch.float32
        assert ((s.abs() >= 0.5) & (s.abs() <= 1.5)).all() and (b != 0).all()
        if c.C > 1:
            assert (s > 0).any() and (s < 0).any()
        for which in ('pre', 'post'):
            for dt in C.DTYPES:
                r = FC.residual(c.id, which, dt)
                assert r.dtype == C.DTYPES[dt] and tuple(r.shape) == FC.out_shape(c.id)
        assert (FC.slopes(c.id, 'channel') < 0).any() and FC.slopes(c.id, 'one').tolist() == [0.25]


def test_compose_is_the_contracts_expression():
    y = torch.tensor([[[[-2.0, 0.5]], [[1.0, -4.0]]]])
    rp, rq = torch.full_like(y, 1.0).bfloat16(), torch.full_like(y, -0.5).bfloat16()
    sl = torch.tensor([0.5, -0.25])
    got = FC.compose(y, FC.VARIANT_BY_ID['preluC_both'], rp, rq, sl)
    assert got.tolist() == [[[[-1.0, 1.0]], [[1.5, 0.25]]]]
    got = FC.compose(y, FC.VARIANT_BY_ID['relu_pre'], rp, None, None)
    assert got.tolist() == [[[[0.0, 1.5]], [[2.0, 0.0]]]]
    x = torch.tensor([[[[1.0]], [[3.0]]]]).half()
    t = FC.folded_input(x, (torch.tensor([2.0, 30000.0]), torch.tensor([-1.0, 0.0])))
    assert t.dtype == torch.float16 and t.flatten().tolist() == [1.0, float('inf')]


# ---------------------------------------------------------------------------------------------------- QuantConv2d
class _Cuda(torch.Tensor):
    """A CPU tensor that says it lives on cuda:0: what the selection predicates read, without a device."""
    is_cuda = True
    device = torch.device('cuda', 0)


def _cuda(t):
    return t.as_subclass(_Cuda)


def _conv(**kw):
    m = QuantConv2d('fp', 'ls-1', 64, 70, 3, {'kind': 'symmetric', 'alpha': 2}, padding=1, **kw).eval()
    m.fp_half = True
    return m


def test_switches_are_off_by_default_and_never_reach_the_binding(hip, monkeypatch):
    assert QuantConv2d.fp_half_fused is False and QuantConv2d.fp_half_bn_fold is False

    def boom(*a, **k):
        raise AssertionError('signw_conv2d_fused_half reached with the switches off')

    monkeypatch.setattr(hip, 'signw_conv2d_fused_half', boom)
    m = _conv()
    x = torch.randn(2, 64, 5, 5).bfloat16()
    bn = torch.nn.BatchNorm2d(64).eval()
    res = torch.randn(2, 70, 5, 5).bfloat16()
    with torch.no_grad(), torch.autocast('cpu', dtype=torch.bfloat16):
        y = m.fused_forward(x, pre_bn=bn, relu=True, res_pre=res)
        ref = torch.relu(m(bn(x)) + res)
    assert torch.equal(y, ref)
    # on: a CPU tensor still takes the composition (the predicate wants a CUDA input)
    m.fp_half_fused = m.fp_half_bn_fold = True
    assert not m._fuses_fp_half(x) and not m._folds_fp_half_bn(x, bn)
    with torch.no_grad(), torch.autocast('cpu', dtype=torch.bfloat16):
        assert torch.equal(m.fused_forward(x, pre_bn=bn, relu=True, res_pre=res), ref)


def test_selection_predicates(monkeypatch):
    monkeypatch.setattr(QuantConv2d, '_wants_hip', lambda self, x: True)
    bf, fp = torch.bfloat16, torch.float16
    m = _conv()
    x = _cuda(torch.zeros(2, 64, 5, 5, dtype=bf))
    assert not m._fuses_fp_half(x)                          # the switch
    m.fp_half_fused = True
    assert m._fuses_fp_half(x)
    assert not m._fuses_fp_half(_cuda(torch.zeros(2, 64, 5, 5)))                 # fp32
    assert not m._fuses_fp_half(torch.zeros(2, 64, 5, 5, dtype=bf))              # not on a GPU
    for attr in ('fp_half', 'fp_half_kernel'):
        setattr(m, attr, False)
        assert not m._fuses_fp_half(x), attr
        setattr(m, attr, True)
    train_bn = torch.nn.BatchNorm2d(64).train()
    assert not m._fuses_fp_half(x, train_bn) and m._fuses_fp_half(x, torch.nn.BatchNorm2d(64).eval())     # a train-mode batch norm
    binary = QuantConv2d('ls-2', 'ls-1', 64, 70, 3, {'kind': 'symmetric', 'alpha': 2}, padding=1).eval()
    binary.fp_half = binary.fp_half_fused = True
    assert not binary._fuses_fp_half(x)
    # the epilogue's operands
    good = _cuda(torch.zeros(2, 70, 5, 5, dtype=bf))
    slopes = _cuda(torch.zeros(70))
    assert m._half_epilogue_fits(x, good, good, slopes) and m._half_epilogue_fits(x, None, None, None)
    assert not m._half_epilogue_fits(x, _cuda(torch.zeros(2, 70, 5, 5, dtype=fp)), None, None)       # another 16-bit type
    assert not m._half_epilogue_fits(x, None, _cuda(torch.zeros(2, 70, 5, 5)), None)                 # fp32
    assert not m._half_epilogue_fits(x, _cuda(torch.zeros(2, 70, 5, 4, dtype=bf)), None, None)       # another shape
    assert not m._half_epilogue_fits(x, torch.zeros(2, 70, 5, 5, dtype=bf), None, None)              # on the CPU
    assert not m._half_epilogue_fits(x, None, None, _cuda(torch.zeros(3)))                           # 3 slopes on 70 channels
    w = torch.zeros(70, 64)
    assert m._half_epilogue_fits(x, ProjectionShortcut(_cuda(torch.zeros(2, 64, 5, 5, dtype=bf)), w, None, 1), None, None)
    assert not m._half_epilogue_fits(x, ProjectionShortcut(_cuda(torch.zeros(2, 64, 5, 5)), w, None, 1), None, None)
    assert not m._half_epilogue_fits(x, ProjectionShortcut(_cuda(torch.zeros(2, 64, 5, 5, dtype=fp)), w, None, 1), None, None)
    # the batch norm: eval mode, running statistics, on x's device, and its own switch
    bn = torch.nn.BatchNorm2d(64).eval()
    bn.running_mean = _cuda(bn.running_mean)
    assert not m._folds_fp_half_bn(x, bn)                   # the switch
    m.fp_half_bn_fold = True
    assert m._folds_fp_half_bn(x, bn)
    assert not m._folds_fp_half_bn(x, torch.nn.BatchNorm2d(64).eval())           # statistics on the CPU
    bn.train()
    assert not m._folds_fp_half_bn(x, bn)
    bn.eval()
    m.fp_half_fused = False
    assert not m._folds_fp_half_bn(x, bn)                   # on top of fp_half_fused only
    assert not m._folds_fp_half_bn(x, torch.nn.BatchNorm2d(64, track_running_stats=False).eval())
