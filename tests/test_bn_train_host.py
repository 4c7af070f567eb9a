"""The train-mode batch-norm fold without a GPU: the header of liblsq_hip_bn_train.so against the table and the bindings, the
rules of ``hip_train.bn_fold_supported`` / ``resnet._bn_conv``, the case table, and the closed form of the backward that the
GPU tests hold the kernels to (``bn_quant_backward64``) against autograd through ``F.batch_norm`` and the torch formulation of
the straight-through estimator, in fp64."""

import os
import re

import pytest
import torch

import bn_train_cases as B
import detgen
import train_step_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {'lsq_bn_train_abi_version', 'lsq_bn_train_workspace_bytes', 'lsq_bn_train_stats', 'lsq_bn_apply',
                'lsq_quant_values_bn', 'lsq_bn_ste_backward_workspace_bytes', 'lsq_bn_ste_backward'}


def bn_quant_backward64(x, gq, scales, alpha, mean, invstd, scale, shift):
    """(grad_x, grad_gamma, grad_beta) of <gq, quantizer(clamp(bn(x)))> in the dtype of ``x`` for a batch norm given as its
    vectors [C]: bn(x) = x scale + shift, x^ = (x - mean) invstd.  g is the straight-through gradient at bn(x) (``T.chain``:
    every sign and mask decided in the dtype of ``x``), then the batch norm's backward in closed form."""
    per_c = lambda v: v.view(1, -1, 1, 1)                                               # noqa: E731
    m = x.numel() // x.shape[1]
    g = T.chain(x * per_c(scale) + per_c(shift), scales, alpha)[1](gq)
    xh = (x - per_c(mean)) * per_c(invstd)
    gbeta, ggamma = g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))
    return per_c(scale) * (g - per_c(gbeta) / m - xh * per_c(ggamma) / m), ggamma, gbeta


# ------------------------------------------------------------------------------------------------- header and bindings
def test_header_table_and_bindings_name_the_same_entry_points():
    from quant import _hip, _sublibs
    row = _sublibs.BY_DIR['bn_train']
    assert row.header == 'lsq_hip_bn_train.h' and _sublibs.soname(row) == 'liblsq_hip_bn_train.so'
    with open(os.path.join(ROOT, 'include', row.header)) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    declared = set(re.findall(r'\b(lsq_[a-z0-9_]+)\s*\(', text))
    assert declared == ENTRY_POINTS == set(row.prototypes)
    assert all(re.fullmatch(row.pattern, s) for s in declared)
    for name in ('bn_train_stats', 'bn_apply', 'quant_values_bn', 'bn_ste_backward', 'bn_train_slabs', 'bn_train_lib'):
        assert callable(getattr(_hip, name)), name
    assert _hip.BN_TRAIN_ABI_VERSION == 1
    with open(os.path.join(ROOT, 'ml-quant_amd', 'csrc', 'bn_train', 'Makefile')) as f:
        make = f.read()
    assert 'include ../sublib.mk' in make and 'LDLIBS' not in make            # it links nothing but the HIP runtime


def test_the_bindings_check_operands_before_any_library_is_loaded():
    from quant import _hip
    x, s = torch.ones((2, 4, 3, 3)), torch.ones((4,))
    with pytest.raises(TypeError):
        _hip.bn_apply(x.double(), s, s)
    with pytest.raises(ValueError, match='contiguous'):
        _hip.bn_apply(x.transpose(2, 3)[:, :, :, :2], s, s)
    with pytest.raises(ValueError, match='C = 4'):
        _hip.bn_train_stats(x, torch.ones((5,)), None, 1e-5, 0.1)
    with pytest.raises(ValueError, match='shape of x'):
        _hip.bn_ste_backward(x, x[:, :, :2].contiguous(), s, s, s, s, None, 2.0)
    with pytest.raises(ValueError, match='plane scales'):
        _hip.quant_values_bn(x, s, s, torch.ones((2, 5)), 2.0)
    with pytest.raises(ValueError, match='cuda device'):
        _hip.bn_apply(x, s, s)


# ------------------------------------------------------------------------------------------------------ the case table
def test_the_case_table_covers_what_it_must():
    assert len({c.id for c in B.CASES}) == len(B.CASES)
    assert {c.scheme for c in B.CASES} == set(B.SCHEMES)
    assert any(c.scheme == 'fp' and c.alpha >= 0 for c in B.CASES)
    assert {c.affine for c in B.CASES} == {True, False} and {c.momentum for c in B.CASES} == {0.1, None}
    shapes = {(c.N, c.C, c.H, c.W) for c in B.CASES}
    assert {(2, 3, 1, 1), (1, 20, 7, 7), (5, 130, 4, 4), (3, 8, 5, 6)} <= shapes
    assert any(c.offset % 4 and (c.H * c.W) % 4 == 0 for c in B.CASES)
    assert any(c.H * c.W // 4 > 256 and (c.H * c.W) % 4 == 0 for c in B.CASES)
    assert all(c.N * c.H * c.W >= 2 and c.N * c.C * c.H * c.W <= 16384 for c in B.CASES)         # quick
    assert 1 <= len(B.MODULE_CASES) <= 6 and all(cid in T.BY_ID for cid in B.MODULE_CASES)
    assert {'fp'} < {T.BY_ID[cid].xs for cid in B.MODULE_CASES}


# ------------------------------------------------------------------------------------------------- the selection rules
def _pair(x_quant='ls-1', w_quant='ls-1', channels=4):
    from quant.binary.binary_conv import QuantConv2d
    conv = QuantConv2d(x_quant, w_quant, channels, 8, 3, dict(T.SYM2), padding=1, bias=True)
    return torch.nn.BatchNorm2d(channels).train(), conv.train()


@pytest.fixture
def fold_on(monkeypatch):
    """The switch set and ``hip_train.supported`` answering True for an fp32 input, as on a GPU host (here: CPU tensors)."""
    from quant.binary import hip_train
    from quant.binary.binary_conv import QuantConv2d
    monkeypatch.setattr(QuantConv2d, 'train_bn_fold', True)
    monkeypatch.setattr(hip_train, 'supported', lambda conv, x: conv.w_quant != 'fp' and x.dtype == torch.float32)
    calls = []
    monkeypatch.setattr(hip_train, 'train_step_forward_bn', lambda conv, bn, x: calls.append((conv, bn)) or conv(bn(x)))
    return calls


def _route(bn, conv, x, calls):
    from quant.models import resnet
    del calls[:]
    resnet._bn_conv(bn, conv, x)
    return len(calls)


def test_the_helper_takes_the_new_step_only_when_every_condition_holds(fold_on, monkeypatch):
    from quant.binary import hip_train
    from quant.binary.binary_conv import QuantConv2d
    x = torch.randn(2, 4, 5, 5)
    bn, conv = _pair()
    assert QuantConv2d.train_bn_fold is True and hip_train.bn_fold_supported(conv, bn, x) and _route(bn, conv, x, fold_on) == 1

    class MyBN(torch.nn.BatchNorm2d):
        pass

    def refusal(runs, bn=None, x_in=x, **pair):
        b, c = _pair(**pair)
        return (b if bn is None else bn, c, x_in, runs)

    # (runs: torch itself accepts the pair on the CPU, so the old route can be watched running)
    refusals = {
        'SyncBatchNorm': refusal(False, bn=torch.nn.SyncBatchNorm(4).train()),
        'a subclass of BatchNorm2d': refusal(True, bn=MyBN(4).train()),
        'fp weights': refusal(True, w_quant='fp'),
        'a bf16 input': refusal(False, x_in=x.bfloat16()),
        'an fp16 input': refusal(False, x_in=x.half()),
        'one value per channel': refusal(False, x_in=x[:1, :, :1, :1]),
        'a 3-d input': refusal(False, x_in=x[0]),
        'fp64 batch-norm parameters': refusal(False, bn=torch.nn.BatchNorm2d(4).double().train()),
    }
    bn, conv = _pair()
    refusals['conv in eval mode'] = (bn, conv.eval(), x, True)
    bn, conv = _pair()
    refusals['bn in eval mode'] = (bn.eval(), conv, x, True)
    bn, conv = _pair()
    conv.hip_train = False
    refusals['hip_train off'] = (bn, conv, x, True)
    for name, (bn, conv, xin, runs) in refusals.items():
        assert not hip_train.bn_fold_supported(conv, bn, xin), name
        if runs:
            assert _route(bn, conv, xin, fold_on) == 0, name                    # ... and the old route runs

    # two values per channel are enough
    bn, conv = _pair()
    assert hip_train.bn_fold_supported(conv, bn, x[:2, :, :1, :1])
    # what ``supported`` refuses is refused
    monkeypatch.setattr(hip_train, 'supported', lambda conv, x: False)
    bn, conv = _pair()
    assert not hip_train.bn_fold_supported(conv, bn, x) and _route(bn, conv, x, fold_on) == 0


def test_with_the_switch_off_nothing_is_asked(monkeypatch):
    from quant.binary import hip_train
    from quant.binary.binary_conv import QuantConv2d
    from quant.models import resnet
    assert QuantConv2d.train_bn_fold is False

    def never(*a, **k):
        raise AssertionError('looked at with the switch off')
    monkeypatch.setattr(hip_train, 'bn_fold_supported', never)
    monkeypatch.setattr(hip_train, 'train_step_forward_bn', never)
    bn, conv = _pair()
    x = torch.randn(2, 4, 5, 5)
    torch.manual_seed(0)
    want = conv(bn(x))
    bn2, conv2 = _pair()
    conv2.load_state_dict(conv.state_dict())
    got = resnet._bn_conv(bn2, conv2, x)
    assert torch.equal(got, want) and torch.equal(bn.running_mean, bn2.running_mean)
    assert int(bn2.num_batches_tracked) == 1


def test_the_block_calls_the_helper_for_both_pairs(fold_on):
    from quant.models.resnet import XnorBasicBlock
    for double in (False, True):
        block = XnorBasicBlock(4, 8, 'ls-1', 'ls-1', ['relu', 'relu'], stride=2, double_shortcut=double, clamp=dict(T.SYM2)).train()
        del fold_on[:]
        block(torch.randn(2, 4, 6, 6))
        assert [(c is block.conv1, b is block.bn1) for c, b in fold_on[:1]] == [(True, True)]
        assert [(c is block.conv2, b is block.bn2) for c, b in fold_on[1:]] == [(True, True)]


# ---------------------------------------------------------------------------------------------------- the closed form
def _torch_quantizer(scheme, xc, scales):
    import quant.binary.quantization as Q
    if scheme == 'fp':
        return xc
    if scheme == 'ls-1':
        return Q.quantizer_ls_1(xc, scales[0])[1]
    if scheme == 'ls-2':
        return Q.quantizer_ls_2(xc, scales[0], scales[1])[2]
    if scheme == 'ls-T':
        return Q.quantizer_ls_ternary(xc, scales[0])[1]
    return Q.quantizer_gf(xc, len(scales), list(scales))[1]


@pytest.mark.parametrize('case', [pytest.param(c, id=c.id) for c in B.CASES])
def test_the_closed_form_is_autograd_through_batch_norm_and_the_estimator(case):
    """fp64 on generic data (no element on a decision's edge): within 1e-12 of the scale of each gradient."""
    k = T.planes(case.scheme)
    shape = (case.N, case.C, case.H, case.W)
    x = (detgen.normal(f'bnh.{case.id}.x', shape, scale=1.3).double() + 0.4).requires_grad_()
    gq = detgen.normal(f'bnh.{case.id}.gq', shape).double()
    gamma = (detgen.uniform(f'bnh.{case.id}.g', (case.C,), 0.5, 1.5).double() if case.affine
             else torch.ones(case.C, dtype=torch.float64)).requires_grad_()
    beta = (detgen.normal(f'bnh.{case.id}.b', (case.C,), scale=0.3).double() if case.affine
            else torch.zeros(case.C, dtype=torch.float64)).requires_grad_()
    base = [0.9, 0.45, 0.2][:k] if case.scheme != 'ls-T' else [0.7, 0.7]
    scales = [v * (1.0 + 0.1 * torch.arange(case.N, dtype=torch.float64)) for v in base]
    eps = 1e-5

    y = torch.nn.functional.batch_norm(x, None, None, gamma, beta, True, 0.1, eps)
    yc = y if case.alpha < 0 else y.clamp(-case.alpha, case.alpha)
    (_torch_quantizer(case.scheme, yc, scales) * gq).sum().backward()

    with torch.no_grad():
        mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
        invstd = 1.0 / torch.sqrt(var + eps)
        scale = gamma * invstd
        gx, gg, gb = bn_quant_backward64(x.detach(), gq, scales, case.alpha, mean, invstd, scale, beta - mean * scale)
    for got, want, name in ((gx, x.grad, 'grad_x'), (gg, gamma.grad, 'grad_gamma'), (gb, beta.grad, 'grad_beta')):
        assert float(want.abs().max()) > 0, name
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (case.id, name)
