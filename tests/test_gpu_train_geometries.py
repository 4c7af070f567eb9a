"""QuantConv2d's train step on the kernels (quant/binary/hip_train.py) across the geometries ``hip_train.supported`` accepts:
(a) every case of tests/golden/train_step_cases.py against the fp64 reference ``step64`` (which tests/test_train_step_cases_host.py
holds to autograd through the torch formulation), (c) the refusal side of ``supported`` and (d) the autograd plumbing.
(b), lsq_train_wgrad alone at non-square geometries, is in tests/test_gpu_wgrad.py."""

import pytest
import torch

import detgen
import train_step_cases as T
from oracle import lsq_exact as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STEP = '_QuantConv2dStepBackward'
BOUND_Y = 1e-5        # of max |y64|: the project's figure for this step and for the bf16 hi + lo GEMMs
BOUND_GX = 1e-5       # per element, of |m_x| mag_x: 2^-18 of the hi + lo split per product, the fp32 rounding of u gy
#                       and fp32 accumulation in another order
BOUND_GW_KERNEL = 2e-6   # per element, of |m_w| mag_w: lsq_train_wgrad's three-term split (BOUND of test_gpu_wgrad.py)
BOUND_GW_MIOPEN = 1e-5   # of max |gw64|: conv2d_weight on MIOpen, whose summation is not ours to bound per element
BOUND_GB = 1e-5       # of max |gb64|


def _hip():
    from quant import _hip
    return _hip


class _Spy:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self.fn(*a, **k)


def _module(case, hip_path, **changes):
    conv = T.make_module(case._replace(**changes) if changes else case)
    conv.hip_train = hip_path
    return conv.to(DEV).train()


def _step(conv, x, gy):
    """One forward and one backward; returns (x leaf, y)."""
    x = x.to(DEV).requires_grad_()
    y = conv(x)
    y.backward(gy.to(DEV))
    return x, y


# ------------------------------------------------------------------------------------------ (a) the step against step64
_TWIN_SCALES, _REFS = {}, {}


def _twin_weight_scales(case):
    """The weight-scale buffers a twin on the torch formulation caches in its step on the same device (once per case)."""
    if case.id not in _TWIN_SCALES:
        d = T.inputs(case.id)
        twin = _module(case, False)
        _, y = _step(twin, d['x'], d['gy'])
        assert type(y.grad_fn).__name__ != STEP
        _TWIN_SCALES[case.id] = {n: b.detach().cpu().clone() for n, b in twin.w_approximate.named_buffers()}
    return _TWIN_SCALES[case.id]


def _reference(case, xscales, wscales):
    """step64 for the scales of the GPU step, computed once per (case, scales) and left unchanged: the two weight-gradient
    routes of a case share it (their scales are the same launches' results)."""
    key = (case.id, None if xscales is None else xscales.numpy().tobytes(), wscales.numpy().tobytes())
    if key not in _REFS:
        d = T.inputs(case.id)
        _REFS[key] = T.step64(d['x'], d['w'], d['b'], d['gy'], None if xscales is None else list(xscales), list(wscales),
                              T.alpha_of(case.clamp), case.stride, (case.pad_h, case.pad_w))
    return _REFS[key]


def _worst(err, bound_unit):
    """max err / bound_unit over the elements whose bound is positive (0 where there is none)."""
    pos = bound_unit > 0
    return float((err[pos] / bound_unit[pos]).max()) if bool(pos.any()) else 0.0


def _step_params():
    out = []
    for c in T.CASES:
        out.append(pytest.param(c, False, id=f'{c.id}-miopen'))
        if c.xs != 'fp':
            out.append(pytest.param(c, True, id=f'{c.id}-wgrad'))
    return out


@pytest.mark.parametrize('case,wgrad', _step_params())
def test_train_step_equals_the_fp64_step(monkeypatch, case, wgrad):
    """Output, the three gradients and the scales of one step on the kernels.  No element and no case is set aside: the
    reference takes the kernels' own fp32 sign decisions, so there are no ties."""
    from quant.binary import hip_train
    hip = _hip()
    monkeypatch.setattr(hip_train, 'WGRAD_KERNEL', wgrad)
    kernel = _Spy(hip.wgrad)
    monkeypatch.setattr(hip, 'wgrad', kernel)
    d = T.inputs(case.id)
    alpha = T.alpha_of(case.clamp)
    conv = _module(case, True)
    assert hip_train.supported(conv, d['x'].to(DEV))
    x, y = _step(conv, d['x'], d['gy'])
    assert type(y.grad_fn).__name__ == STEP
    assert kernel.calls == (1 if wgrad else 0)
    # the scales: cached weight scales bit-equal to the torch formulation's on this device, v1 of the solving schemes bit-equal
    # to the exact oracle
    twin = _twin_weight_scales(case)
    got = dict(conv.w_approximate.named_buffers())
    assert set(got) == set(twin)
    for name, buf in got.items():
        assert torch.equal(buf.cpu(), twin[name]) and float(buf.abs().sum()) > 0, name
    wscales = conv.w_approximate.plane_scales().detach().cpu()
    xscales = None
    if case.xs != 'fp':
        xscales = conv.last_act_scales.detach().cpu()
        assert tuple(xscales.shape) == (T.planes(case.xs), case.N)
    if case.xs in ('ls-2', 'ls-T'):
        xc = d['x'].clamp(-alpha, alpha) if alpha >= 0 else d['x']
        want = E.solve_rows(xc.numpy(), case.xs == 'ls-T', 3)
        assert (xscales[0].numpy() == want).all(), (xscales[0], want)
    ref = _reference(case, xscales, wscales)

    ratios = {}
    err = (y.detach().cpu().double() - ref['y']).abs()
    ratios['y'] = float(err.max() / ref['y'].abs().max()) / BOUND_Y
    unit = ref['m_x'].abs() * ref['mag_x']
    err_x = (x.grad.cpu().double() - ref['gx']).abs()
    ratios['gx'] = _worst(err_x, unit) / BOUND_GX
    unit_w = ref['m_w'].abs() * ref['mag_w']
    err_w = (conv.weight.grad.cpu().double() - ref['gw']).abs()
    if wgrad:
        ratios['gw'] = _worst(err_w, unit_w) / BOUND_GW_KERNEL
    else:
        ratios['gw'] = float(err_w.max() / ref['gw'].abs().max()) / BOUND_GW_MIOPEN
    if case.bias:
        err_b = (conv.bias.grad.cpu().double() - ref['gb']).abs()
        ratios['gb'] = float(err_b.max() / ref['gb'].abs().max()) / BOUND_GB
    print(f'\ntrain-step ratios {case.id} {"wgrad" if wgrad else "miopen"} '
          + ' '.join(f'{k}={v:.4f}' for k, v in ratios.items())
          + f' zero_bound_gx={int((unit == 0).sum())}/{unit.numel()}')

    assert ratios['y'] <= 1.0, (case.id, 'y', ratios)
    # every position the forward never read, or whose straight-through mask is closed, has a bound of exactly 0
    assert bool((err_x <= BOUND_GX * unit + 1e-30).all()), (case.id, 'gx', ratios, float(err_x[unit == 0].max()) if bool((unit == 0).any()) else 0.0)
    if wgrad:
        assert bool((err_w <= BOUND_GW_KERNEL * unit_w + 1e-30).all()), (case.id, 'gw', ratios)
    else:
        assert ratios['gw'] <= 1.0, (case.id, 'gw', ratios)
    if case.bias:
        assert ratios['gb'] <= 1.0, (case.id, 'gb', ratios)
    else:
        assert conv.bias is None


# ----------------------------------------------------------------------------------------------------- (c) refusals
def _plain(device=DEV, dtype=torch.float32, w_quant='ls-1', hip_path=True, **kwargs):
    """ls-1 x ls-1 (or ``w_quant``), 8 -> 16, 3 x 3, padding 1 unless ``kwargs`` say otherwise."""
    from quant.binary.binary_conv import QuantConv2d
    kw = {'padding': 1, 'bias': True}
    kw.update(kwargs)
    conv = QuantConv2d('ls-1', w_quant, 8, 16, 3, dict(T.SYM2), **kw)
    with torch.no_grad():
        conv.weight.copy_(detgen.normal('tgeo.refuse.w', conv.weight.shape, scale=0.2))
        conv.bias.copy_(detgen.normal('tgeo.refuse.b', conv.bias.shape, scale=0.1))
    conv.hip_train = hip_path
    return conv.to(device=device, dtype=dtype).train()


# (what is outside the limits, the same argument put back inside them)
REFUSALS = {
    'groups2': ({'groups': 2}, {'groups': 1}),
    'dilation2': ({'dilation': 2}, {'dilation': 1}),
    'dilation1x2': ({'dilation': (1, 2)}, {'dilation': (1, 1)}),
    'stride3': ({'stride': 3}, {'stride': 2}),
    'stride1x2': ({'stride': (1, 2)}, {'stride': (2, 2)}),
    'pad_k_on_rows': ({'padding': (3, 1)}, {'padding': (2, 1)}),
    'pad_k_on_columns': ({'padding': (0, 3)}, {'padding': (0, 2)}),
    'reflect': ({'padding_mode': 'reflect'}, {'padding_mode': 'zeros'}),
    'same': ({'padding': 'same'}, {'padding': 1}),
    'fp_weights': ({'w_quant': 'fp'}, {'w_quant': 'ls-1'}),
    'half_input': ({'dtype': torch.float16}, {'dtype': torch.float32}),
}


@pytest.mark.parametrize('name', list(REFUSALS))
def test_outside_the_limits_the_module_takes_the_torch_formulation(name):
    """``supported`` is False, the graph is the torch formulation's and the step equals bit for bit the twin's with
    ``hip_train = False`` (the same code path); the accepted neighbour takes the kernels."""
    from quant.binary import hip_train
    bad, good = REFUSALS[name]
    dtype = bad.get('dtype', torch.float32)
    x0 = detgen.normal('tgeo.refuse.x', (2, 8, 9, 8), scale=1.2).to(DEV)
    runs = []
    for hip_path in (True, False):
        conv = _plain(hip_path=hip_path, **bad)
        x = x0.to(dtype).clone().requires_grad_()                      # (a leaf of its own: .to() of the same type is x0 itself)
        if hip_path:
            assert not hip_train.supported(conv, x)
        y = conv(x)
        assert type(y.grad_fn).__name__ != STEP
        y.backward(detgen.normal('tgeo.refuse.gy', y.shape).to(DEV).to(dtype))
        runs.append((y.detach(), x.grad, conv.weight.grad, conv.bias.grad))
    for a, b in zip(*runs):
        assert a is not None and torch.equal(a, b)
    conv = _plain(**good)
    x = x0.clone().requires_grad_()
    assert hip_train.supported(conv, x)
    y = conv(x)
    assert type(y.grad_fn).__name__ == STEP
    y.backward(torch.ones_like(y))
    assert x.grad is not None and conv.weight.grad is not None


# ------------------------------------------------------------------------------------------------------ (d) plumbing
PLUMB = T.BY_ID['s2_3x5']          # 20 -> 50, 3 x 5, stride 2, pad (2, 0), ls-2 activations
_BASE = {}


def _baseline(wgrad):
    """The contiguous run of the plumbing case under the current WGRAD_KERNEL (once per setting): y, gx, gw, gb."""
    if wgrad not in _BASE:
        d = T.inputs(PLUMB.id)
        conv = _module(PLUMB, True)
        x, y = _step(conv, d['x'], d['gy'])
        assert type(y.grad_fn).__name__ == STEP
        _BASE[wgrad] = (y.detach().clone(), x.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())
    return _BASE[wgrad]


@pytest.fixture(params=[False, True], ids=['miopen', 'wgrad'])
def route(request, monkeypatch):
    from quant.binary import hip_train
    monkeypatch.setattr(hip_train, 'WGRAD_KERNEL', request.param)
    return request.param


def _equal_to_baseline(route, y, gx, conv):
    by, bgx, bgw, bgb = _baseline(route)
    assert type(y.grad_fn).__name__ == STEP
    assert torch.equal(y.detach(), by)
    assert torch.equal(gx, bgx)
    assert torch.equal(conv.weight.grad, bgw) and torch.equal(conv.bias.grad, bgb)


@pytest.mark.parametrize('layout', ['channels_last', 'batch_slice'])
def test_non_contiguous_input(route, layout):
    d = T.inputs(PLUMB.id)
    conv = _module(PLUMB, True)
    if layout == 'channels_last':
        x = d['x'].to(DEV).contiguous(memory_format=torch.channels_last)
    else:
        big = detgen.normal('tgeo.plumb.big', (2 * PLUMB.N,) + tuple(d['x'].shape[1:])).to(DEV)
        big[::2] = d['x'].to(DEV)
        x = big[::2].detach()
    assert not x.is_contiguous()
    x.requires_grad_()
    y = conv(x)
    y.backward(d['gy'].to(DEV))
    _equal_to_baseline(route, y, x.grad, conv)


@pytest.mark.parametrize('how', ['expanded', 'permuted'])
def test_non_contiguous_output_gradient(route, how):
    """``y.sum().backward()`` hands backward an expanded gradient (every stride 0), a loss on a permuted copy a permuted one."""
    d = T.inputs(PLUMB.id)
    conv = _module(PLUMB, True)
    x = d['x'].to(DEV).requires_grad_()
    y = conv(x)
    if how == 'expanded':
        y.sum().backward()
        twin = _module(PLUMB, True)
        x2, y2 = _step(twin, d['x'], torch.ones_like(d['gy']))
        assert torch.equal(y.detach(), y2.detach()) and torch.equal(x.grad, x2.grad)
        assert torch.equal(conv.weight.grad, twin.weight.grad) and torch.equal(conv.bias.grad, twin.bias.grad)
    else:
        gperm = d['gy'].to(DEV).permute(0, 2, 3, 1).contiguous()
        (y.permute(0, 2, 3, 1).contiguous() * gperm).sum().backward()
        _equal_to_baseline(route, y, x.grad, conv)


def test_needs_input_grad_subsets(route):
    d = T.inputs(PLUMB.id)
    by, bgx, bgw, bgb = _baseline(route)
    # x without requires_grad
    conv = _module(PLUMB, True)
    x = d['x'].to(DEV)
    y = conv(x)
    y.backward(d['gy'].to(DEV))
    assert type(y.grad_fn).__name__ == STEP and x.grad is None
    assert torch.equal(y.detach(), by) and torch.equal(conv.weight.grad, bgw) and torch.equal(conv.bias.grad, bgb)
    # weight frozen
    conv = _module(PLUMB, True)
    conv.weight.requires_grad_(False)
    x, y = _step(conv, d['x'], d['gy'])
    assert type(y.grad_fn).__name__ == STEP and conv.weight.grad is None
    assert torch.equal(y.detach(), by) and torch.equal(x.grad, bgx) and torch.equal(conv.bias.grad, bgb)
    # bias frozen
    conv = _module(PLUMB, True)
    conv.bias.requires_grad_(False)
    x, y = _step(conv, d['x'], d['gy'])
    assert conv.bias.grad is None and torch.equal(x.grad, bgx) and torch.equal(conv.weight.grad, bgw)


def test_without_a_bias(route):
    """``bias=None``: the gradients are the biased module's bit for bit (neither depends on the bias), the output is the fp64
    step's without it."""
    d = T.inputs(PLUMB.id)
    by, bgx, bgw, _ = _baseline(route)
    conv = _module(PLUMB, True, bias=False)
    assert conv.bias is None
    x, y = _step(conv, d['x'], d['gy'])
    assert type(y.grad_fn).__name__ == STEP
    assert torch.equal(x.grad, bgx) and torch.equal(conv.weight.grad, bgw)
    ref = T.step64(d['x'], d['w'], None, d['gy'], list(conv.last_act_scales.cpu()), list(conv.w_approximate.plane_scales().cpu()),
                   T.alpha_of(PLUMB.clamp), PLUMB.stride, (PLUMB.pad_h, PLUMB.pad_w))
    assert float((y.detach().cpu().double() - ref['y']).abs().max()) <= BOUND_Y * float(ref['y'].abs().max())
    assert not torch.equal(y.detach(), by)


def test_two_forwards_before_one_backward_on_the_miopen_route(monkeypatch):
    """Each step's backward reads its own input and its own saved scales (the module's plane workspace holds the second
    input's planes by then, and with WGRAD_KERNEL off nothing may read them).  The on case is
    test_gpu_wgrad.py::test_backward_reads_the_planes_of_its_own_step."""
    from quant.binary import hip_train
    monkeypatch.setattr(hip_train, 'WGRAD_KERNEL', False)
    d = T.inputs(PLUMB.id)
    x2_cpu = detgen.normal('tgeo.plumb.x2', d['x'].shape, scale=0.6)
    g2 = detgen.normal('tgeo.plumb.g2', d['gy'].shape).to(DEV)
    g1 = d['gy'].to(DEV)
    singles = []
    for xc, g in ((d['x'], g1), (x2_cpu, g2)):
        conv = _module(PLUMB, True)
        x, y = _step(conv, xc, g)
        singles.append((y.detach(), x.grad, conv.weight.grad, conv.bias.grad))
    conv = _module(PLUMB, True)
    xa, xb = d['x'].to(DEV).requires_grad_(), x2_cpu.to(DEV).requires_grad_()
    ya, yb = conv(xa), conv(xb)
    ((ya * g1).sum() + (yb * g2).sum()).backward()
    assert torch.equal(ya.detach(), singles[0][0]) and torch.equal(yb.detach(), singles[1][0])
    assert torch.equal(xa.grad, singles[0][1]) and torch.equal(xb.grad, singles[1][1])
    assert torch.equal(conv.weight.grad, singles[0][2] + singles[1][2])
    assert torch.equal(conv.bias.grad, singles[0][3] + singles[1][3])
