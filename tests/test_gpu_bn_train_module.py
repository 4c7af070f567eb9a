"""``QuantConv2d.train_bn_fold`` on the GPU: a bn -> QuantConv2d pair on geometry classes of tests/golden/train_step_cases.py
and one stride-2 ``XnorBasicBlock`` with a projection, each with the switch on and off from equal state.

With the switch on, the step is held to an fp64 restatement that takes the kernels' own decisions: ``step64`` on the tensor
the quantizer saw (lsq_bn_apply with the step's own scale / shift), then the batch norm's backward in closed form.  The bounds
of y, grad_w and grad_b are those of tests/test_gpu_train_geometries.py; grad_x, grad_gamma and grad_beta carry that file's
bound of g = d loss / d bn(x) through the closed form, plus the roundings include/lsq_hip_bn_train.h counts."""

import copy

import pytest
import torch

import bn_train_cases as B
import detgen
import train_step_cases as T
from test_gpu_bn_train import GRAD_X_ROUNDINGS, U24, U53, _within
from test_gpu_train_geometries import BOUND_GB, BOUND_GW_MIOPEN, BOUND_GX, BOUND_Y

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STEP_BN = '_BNQuantConv2dStepBackward'
STEP = '_QuantConv2dStepBackward'
EPS = 1e-5


def _hip():
    from quant import _hip
    return _hip


@pytest.fixture
def switch(monkeypatch):
    from quant.binary.binary_conv import QuantConv2d

    def set_to(on):
        monkeypatch.setattr(QuantConv2d, 'train_bn_fold', on)
    return set_to


def _pair(case, momentum=0.1):
    """(bn, conv) of a case on the device in train mode, deterministic parameters and running statistics."""
    conv = T.make_module(case).to(DEV).train()
    bn = torch.nn.BatchNorm2d(case.C, eps=EPS, momentum=momentum)
    with torch.no_grad():
        bn.weight.copy_(detgen.uniform(f'bnm.{case.id}.gamma', (case.C,), 0.5, 1.5))
        bn.bias.copy_(detgen.normal(f'bnm.{case.id}.beta', (case.C,), scale=0.3))
        bn.running_mean.copy_(detgen.normal(f'bnm.{case.id}.rm', (case.C,), scale=0.2))
        bn.running_var.copy_(detgen.uniform(f'bnm.{case.id}.rv', (case.C,), 0.5, 1.5))
    return bn.to(DEV).train(), conv


def _input(case):
    c = torch.arange(case.C, dtype=torch.float32).view(1, -1, 1, 1)
    return (T.inputs(case.id)['x'] * (0.5 + (c % 3) * 0.4) + (c % 5 - 2.0) * 0.3).to(DEV)


def _run(bn, conv, x0, gy, before_backward=None):
    from quant.models import resnet
    x = x0.clone().requires_grad_()
    y = resnet._bn_conv(bn, conv, x)
    if before_backward is not None:
        before_backward(x, y)                         # (saved tensors are released by backward)
    y.backward(gy)
    return x, y


def _nodes(fn, name, seen=None):
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return []
    seen.add(fn)
    out = [fn] if type(fn).__name__ == name else []
    for nxt, _ in fn.next_functions:
        out += _nodes(nxt, name, seen)
    return out


def _no_copy_of_the_input_is_saved(node, x):
    same_shape = [t for t in node.saved_tensors if t.shape == x.shape]
    assert len(same_shape) == 1 and same_shape[0].data_ptr() == x.data_ptr(), [tuple(t.shape) for t in node.saved_tensors]


def _stats64(x, bn0, momentum):
    """fp64 batch statistics of x, the running buffers torch's update gives from ``bn0``'s, and the bounds of
    include/lsq_hip_bn_train.h for mean-like and variance-like values."""
    x64 = x.detach().cpu().double()
    m = x64.numel() // x64.shape[1]
    b_mean = lambda v: U24 * v.abs() + m * U53 * x64.abs().mean((0, 2, 3))                          # noqa: E731
    b_var = lambda v: U24 * v.abs() + m * U53 * (x64 * x64).mean((0, 2, 3)) * m / (m - 1)         # noqa: E731
    rm, rv = bn0.running_mean.detach().cpu().double(), bn0.running_var.detach().cpu().double()
    torch.nn.functional.batch_norm(x64, rm, rv, None, None, True, momentum, EPS)
    return x64, m, rm, rv, b_mean, b_var


@pytest.mark.parametrize('cid', B.MODULE_CASES)
def test_pair_with_the_switch_on(switch, cid):
    hip = _hip()
    from quant.binary import hip_train
    case = T.BY_ID[cid]
    d = T.inputs(cid)
    gy = d['gy'].to(DEV)
    x0 = _input(case)
    bn, conv = _pair(case)
    bn_off, conv_off = copy.deepcopy(bn), copy.deepcopy(conv)
    bn_start = copy.deepcopy(bn)
    assert hip_train.supported(conv, x0)

    switch(True)
    x, y = _run(bn, conv, x0, gy, lambda x, y: _no_copy_of_the_input_is_saved(y.grad_fn, x))
    assert type(y.grad_fn).__name__ == STEP_BN
    switch(False)
    x_off, y_off = _run(bn_off, conv_off, x0, gy)
    assert type(y_off.grad_fn).__name__ == STEP

    # ---- the batch norm's buffers: fp64 on the same data, and the off route's
    x64, m, rm64, rv64, b_mean, b_var = _stats64(x0, bn_start, 0.1)
    _within(bn.running_mean, rm64, 0.1 * b_mean(x64.mean((0, 2, 3))) + U24 * rm64.abs(), f'{cid} running_mean')
    _within(bn.running_var, rv64, 0.1 * b_var(x64.var((0, 2, 3), unbiased=True)) + U24 * rv64.abs(), f'{cid} running_var')
    assert int(bn.num_batches_tracked) == int(bn_off.num_batches_tracked) == 1
    # torch's own fp32 statistics carry fp32 summation error, at most m 2^-24 of the mean magnitude, on top of the bound above
    fp32_mean = 0.1 * m * U24 * x64.abs().mean((0, 2, 3))
    fp32_var = 0.1 * m * U24 * 3 * (x64 * x64).mean((0, 2, 3)) * m / (m - 1)
    _within(bn.running_mean, bn_off.running_mean.cpu().double(),
            0.1 * b_mean(x64.mean((0, 2, 3))) + 2 * U24 * rm64.abs() + fp32_mean, f'{cid} running_mean against the off route')
    _within(bn.running_var, bn_off.running_var.cpu().double(),
            0.1 * b_var(x64.var((0, 2, 3), unbiased=True)) + 2 * U24 * rv64.abs() + fp32_var, f'{cid} running_var against the off route')

    # ---- y: the quantizer's fold called directly with the step's own scale / shift (the statistics kernel repeats its bits)
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    mean, var, invstd, scale, shift = hip.bn_train_stats(x0, gamma, beta, EPS, 0.1)
    alpha = T.alpha_of(case.clamp)
    geom = conv._geom_of(x0, hip)
    wscales = conv.w_approximate.plane_scales().detach().to(torch.float32).contiguous()
    wbits, wsum = hip.pack_weight(conv.weight.detach(), geom, wscales)
    y_direct = torch.empty_like(y)
    bias = None if conv.bias is None else conv.bias.detach()
    xscales = None
    if case.xs == 'fp':
        hip.signw_conv2d(x0, alpha, wbits, wscales, bias, geom, y_direct, pre=(scale, shift))
    else:
        from quant.binary.hip_module import zero_planes
        k = conv.x_approximate.n_planes
        planes = zero_planes(geom, k, DEV, hip)
        xscales = torch.empty((k, case.N), dtype=torch.float32, device=DEV)
        hip.act_quant(x0, geom, conv.x_approximate.hip_scheme, k, conv.act_skip, alpha, planes, xscales, None, pre=(scale, shift))
        hip.xnor_conv2d(planes, k, xscales, wbits, wsum, wscales, bias, geom, y_direct)
        assert torch.equal(xscales, conv.last_act_scales)
    assert torch.equal(y.detach(), y_direct)

    # ---- the fp64 restatement on what the quantizer saw
    y_bn = hip.bn_apply(x0, scale, shift)
    ref = T.step64(y_bn, conv.weight, conv.bias, gy, None if xscales is None else list(xscales.cpu()), list(wscales.cpu()),
                   alpha, case.stride, (case.pad_h, case.pad_w))
    assert float((y.detach().cpu().double() - ref['y']).abs().max()) <= BOUND_Y * float(ref['y'].abs().max())
    err_w = (conv.weight.grad.cpu().double() - ref['gw']).abs()
    assert float(err_w.max()) <= BOUND_GW_MIOPEN * float(ref['gw'].abs().max())
    if case.bias:
        assert float((conv.bias.grad.cpu().double() - ref['gb']).abs().max()) <= BOUND_GB * float(ref['gb'].abs().max())

    per_c = lambda t: t.view(1, -1, 1, 1)                                              # noqa: E731
    sums = lambda t: t.sum((0, 2, 3))                                                  # noqa: E731
    g, e_g = ref['gx'], BOUND_GX * ref['m_x'].abs() * ref['mag_x']                     # g and the bound of the kernels' g
    xh = (x64 - per_c(mean.cpu().double())) * per_c(invstd.cpu().double())
    s64 = per_c(scale.cpu().double())
    sg, sgx = sums(g), sums(g * xh)
    e_sg = sums(e_g) + U24 * sg.abs() + m * U53 * sums(g.abs())
    e_sgx = sums(e_g * xh.abs()) + U24 * sgx.abs() + m * U53 * sums((g * xh).abs())
    _within(bn.bias.grad, sg, e_sg + 1e-30, f'{cid} grad_beta')
    _within(bn.weight.grad, sgx, e_sgx + 1e-30, f'{cid} grad_gamma')
    want = s64 * (g - per_c(sg) / m - xh * per_c(sgx) / m)
    bound = s64.abs() * (e_g + per_c(e_sg) / m + xh.abs() * per_c(e_sgx) / m) \
        + GRAD_X_ROUNDINGS * U24 * s64.abs() * (g.abs() + per_c(sg).abs() / m + xh.abs() * per_c(sgx).abs() / m)
    _within(x.grad, want, bound + 1e-30, f'{cid} grad_x')
    assert float(x.grad.abs().sum()) > 0 and float(x_off.grad.abs().sum()) > 0


def test_cumulative_average_and_no_running_statistics(switch):
    case = T.BY_ID['base3x3']
    gy, x0 = T.inputs(case.id)['gy'].to(DEV), _input(case)
    switch(True)
    bn, conv = _pair(case, momentum=None)
    start = copy.deepcopy(bn)
    with torch.no_grad():
        bn.num_batches_tracked.fill_(3)
    _, y = _run(bn, conv, x0, gy)
    assert type(y.grad_fn).__name__ == STEP_BN and int(bn.num_batches_tracked) == 4
    x64, m, rm64, rv64, b_mean, b_var = _stats64(x0, start, 0.25)
    _within(bn.running_mean, rm64, 0.25 * b_mean(x64.mean((0, 2, 3))) + U24 * rm64.abs(), 'cumulative running_mean')
    _within(bn.running_var, rv64, 0.25 * b_var(x64.var((0, 2, 3), unbiased=True)) + U24 * rv64.abs(), 'cumulative running_var')

    conv2 = T.make_module(case).to(DEV).train()
    bare = torch.nn.BatchNorm2d(case.C, affine=False, track_running_stats=False).to(DEV).train()
    x, y2 = _run(bare, conv2, x0, gy)
    assert type(y2.grad_fn).__name__ == STEP_BN and bare.running_mean is None and x.grad is not None


def _block():
    from quant.models.resnet import XnorBasicBlock
    block = XnorBasicBlock(8, 16, 'ls-2', 'ls-1', ['relu', 'relu'], stride=2, clamp=dict(T.SYM2))
    detgen.fill_module(block, seed=5)
    return block.to(DEV).train()


def _block_step(block, x0, gy, before_backward=None):
    x = x0.clone().requires_grad_()
    y = block(x)
    if before_backward is not None:
        before_backward(y)
    y.backward(gy)
    return x, y


def _each_fold_saves_one_activation(y):
    folds = _nodes(y.grad_fn, STEP_BN)
    assert len(folds) == 2 and not _nodes(y.grad_fn, STEP)
    for node in folds:
        big = [t for t in node.saved_tensors if t.dim() == 4 and t.shape[0] == 2 and t.shape[2] > 3]
        assert len(big) == 1, [tuple(t.shape) for t in node.saved_tensors]          # its input and nothing else of that shape


def test_block_with_the_switch_on(switch):
    x0 = (detgen.normal('bnm.block.x', (2, 8, 8, 8), scale=1.2) + 0.3).to(DEV)
    gy = detgen.normal('bnm.block.gy', (2, 16, 4, 4)).to(DEV)
    block = _block()
    assert len(block.shortcut) == 2                                   # a projection
    start = copy.deepcopy(block.bn1)
    switch(True)
    x, y = _block_step(block, x0, gy, _each_fold_saves_one_activation)
    x64, m, rm64, rv64, b_mean, b_var = _stats64(x0, start, 0.1)
    _within(block.bn1.running_mean, rm64, 0.1 * b_mean(x64.mean((0, 2, 3))) + U24 * rm64.abs(), 'block bn1 running_mean')
    _within(block.bn1.running_var, rv64, 0.1 * b_var(x64.var((0, 2, 3), unbiased=True)) + U24 * rv64.abs(), 'block bn1 running_var')
    assert [int(b.num_batches_tracked) for b in (block.bn1, block.bn2, block.shortcut[1])] == [1, 1, 1]
    for name, p in block.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert float(block.bn1.weight.grad.abs().sum()) > 0 and float(block.bn2.bias.grad.abs().sum()) > 0
    assert float(x.grad.abs().sum()) > 0


def test_with_the_switch_off_the_helper_changes_nothing(switch, monkeypatch):
    """Pair and block: outputs, gradients and buffers bit for bit those of ``conv(bn(x))`` with the helper bypassed."""
    from quant.models import resnet
    switch(False)
    x0 = (detgen.normal('bnm.block.x', (2, 8, 8, 8), scale=1.2) + 0.3).to(DEV)
    gy = detgen.normal('bnm.block.gy', (2, 16, 4, 4)).to(DEV)
    through = _block()
    bypass = copy.deepcopy(through)
    x1, y1 = _block_step(through, x0, gy)
    assert len(_nodes(y1.grad_fn, STEP)) == 2 and not _nodes(y1.grad_fn, STEP_BN)
    monkeypatch.setattr(resnet, '_bn_conv', lambda bn, conv, x: conv(bn(x)))
    x2, y2 = _block_step(bypass, x0, gy)
    assert torch.equal(y1.detach(), y2.detach()) and torch.equal(x1.grad, x2.grad)
    for (name, p), (_, q) in zip(through.named_parameters(), bypass.named_parameters()):
        assert torch.equal(p.grad, q.grad), name
    for (name, p), (_, q) in zip(through.named_buffers(), bypass.named_buffers()):
        assert torch.equal(p, q), name
    monkeypatch.undo()
    switch(False)

    case = T.BY_ID['s2_3x5']
    gy, xin = T.inputs(case.id)['gy'].to(DEV), _input(case)
    bn, conv = _pair(case)
    bn2, conv2 = copy.deepcopy(bn), copy.deepcopy(conv)
    xa, ya = _run(bn, conv, xin, gy)
    xb = xin.clone().requires_grad_()
    yb = conv2(bn2(xb))
    yb.backward(gy)
    assert type(ya.grad_fn).__name__ == STEP
    assert torch.equal(ya.detach(), yb.detach()) and torch.equal(xa.grad, xb.grad)
    assert torch.equal(conv.weight.grad, conv2.weight.grad) and torch.equal(bn.weight.grad, bn2.weight.grad)
    assert torch.equal(bn.running_var, bn2.running_var)
