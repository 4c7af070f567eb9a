"""lsq_signw_conv2d_dgrad on the GPU (liblsq_hip_conv_train.so) and QuantConv2d's train step with ``hip_train.DGRAD_KERNEL``:
(a) the kernel alone on every case of tests/golden/conv_dgrad_cases.py against the fp64 reference, (b) the whole step with
the switch on against the same reference, (c) the plumbing: two forwards before one backward, an input without a gradient,
and the switch off."""

import ctypes

import pytest
import torch

import conv_dgrad_cases as D
import detgen

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STEP = '_QuantConv2dStepBackward'
# the bounds of tests/test_gpu_train_geometries.py
BOUND_Y = 1e-5        # of max |y64|
BOUND_GX = 1e-5       # per element, of mag_x (the kernel alone) or |m_x| mag_x (the step): 2^-18 + 2^-24 per product of the
#                       hi + lo split and the rounding of gy * u, the rest is fp32 accumulation in another order
BOUND_GW_MIOPEN = 1e-5   # of max |gw64|
BOUND_GB = 1e-5       # of max |gb64|
SENTINEL = -7.25
PAD = 64              # sentinel floats in front of and behind grad_xq; sentinel bytes 8 * PAD around the workspace


def _hip():
    from quant import _hip
    return _hip


class _Spy:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self.fn(*a, **k)


def _geom(hip, c):
    return hip.make_geom(c.N, c.C, c.H, c.W, c.O, c.KH, c.KW, (c.stride_h, c.stride_w), (c.pad_h, c.pad_w),
                         (c.dil_h, c.dil_w), c.groups)


def _module(case, hip_path):
    conv = D.make_module(case)
    conv.hip_train = hip_path
    return conv.to(DEV).train()


def _step(conv, x, gy):
    x = x.to(DEV).requires_grad_()
    y = conv(x)
    y.backward(gy.to(DEV))
    return x, y


def _worst(err, bound_unit):
    pos = bound_unit > 0
    return float((err[pos] / bound_unit[pos]).max()) if bool(pos.any()) else 0.0


def _of_max(err, ref64):
    """max err as a fraction of max |ref64|; a reference that is 0 everywhere (a straight-through mask closed on every
    element) admits no error at all."""
    top = float(ref64.abs().max())
    if top == 0.0:
        return 0.0 if float(err.max()) == 0.0 else float('inf')
    return float(err.max()) / top


_REFS, _CPU_SCALES = {}, {}


def _cpu_weight_scales(case):
    """The weight plane scales [kw, O] of the torch formulation on the CPU (once per case)."""
    if case.id not in _CPU_SCALES:
        conv = D.make_module(case)
        with torch.no_grad():
            conv.w_approximate(conv.weight)
            _CPU_SCALES[case.id] = conv.w_approximate.plane_scales().detach().float().contiguous().clone()
    return _CPU_SCALES[case.id]


def _reference(case, xscales, wscales):
    """step64 for given scales, computed once per (case, scales) and left unchanged."""
    key = (case.id, None if xscales is None else xscales.numpy().tobytes(), wscales.numpy().tobytes())
    if key not in _REFS:
        d = D.inputs(case.id)
        _REFS[key] = D.step64(case, d['x'], d['w'], d['b'], d['gy'], None if xscales is None else list(xscales), list(wscales))
    return _REFS[key]


# ------------------------------------------------------------------------------------------------- (a) the kernel alone
@pytest.mark.parametrize('case', D.CASES, ids=lambda c: c.id)
def test_kernel_equals_the_fp64_input_gradient(case):
    """|gxq - gxq64| <= 1e-5 mag_x per element, exactly +0 wherever the bound is 0, no case and no element set aside; a second
    call (straight through the C ABI, into a buffer and a workspace between sentinels) gives the same bits and leaves the
    sentinels alone."""
    hip = _hip()
    d = D.inputs(case.id)
    geom = _geom(hip, case)
    wscales = _cpu_weight_scales(case)
    xs = D.act_scales_cpu(case, d['x'])               # (the activation side does not enter gxq; step64 wants scales)
    ref = _reference(case, torch.stack(xs) if xs else None, wscales)
    wsc = wscales.to(DEV)
    wbits, _ = hip.pack_weight(d['w'].to(DEV), geom, wsc)
    gy = d['gy'].to(DEV)
    got = hip.signw_conv2d_dgrad(gy, wbits, wsc, geom)
    assert tuple(got.shape) == (case.N, case.C, case.H, case.W) and got.dtype == torch.float32
    g = got.cpu()
    err = (g.double() - ref['gxq']).abs()
    unit = ref['mag_x']
    ratio = _worst(err, unit) / BOUND_GX
    zero = unit == 0
    print(f'\nconv-dgrad kernel ratio {case.id} {ratio:.4f} zero_bound={int(zero.sum())}/{unit.numel()}')
    assert bool((err <= BOUND_GX * unit).all()), (case.id, ratio)
    assert bool((g[zero] == 0).all()) and not bool(torch.signbit(g[zero]).any()), case.id

    # the second call: the C ABI itself, sentinels around grad_xq and around a workspace of exactly the stated size
    lib = hip.conv_train_lib()
    kw = wsc.shape[0]
    need = int(lib.lsq_signw_conv2d_dgrad_workspace_bytes(ctypes.byref(geom), kw))
    assert need > 0 and need % 8 == 0
    n = got.numel()
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    wsbuf = torch.full((need + 16 * PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    ws_ptr = wsbuf.data_ptr() + 8 * PAD
    assert ws_ptr % 8 == 0
    code = lib.lsq_signw_conv2d_dgrad(gy.data_ptr(), wbits.data_ptr(), kw, wsc.data_ptr(), ctypes.byref(geom),
                                      buf.data_ptr() + 4 * PAD, ws_ptr, need, hip.stream_ptr(DEV))
    assert code == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[PAD:PAD + n].view_as(got), got)
    assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all())
    assert bool((wsbuf[:8 * PAD] == 0xA5).all()) and bool((wsbuf[8 * PAD + need:] == 0xA5).all())


# ------------------------------------------------------------------------------------------ (b) the step, switch on
_TWIN_SCALES = {}


def _twin_weight_scales(case):
    """The weight-scale buffers a twin on the torch formulation caches in its step on the same device (once per case)."""
    if case.id not in _TWIN_SCALES:
        d = D.inputs(case.id)
        twin = _module(case, False)
        _, y = _step(twin, d['x'], d['gy'])
        assert type(y.grad_fn).__name__ != STEP
        _TWIN_SCALES[case.id] = {n: b.detach().cpu().clone() for n, b in twin.w_approximate.named_buffers()}
    return _TWIN_SCALES[case.id]


@pytest.mark.parametrize('case', D.CASES, ids=lambda c: c.id)
def test_train_step_with_the_kernel_equals_the_fp64_step(monkeypatch, case):
    from quant.binary import hip_train
    hip = _hip()
    monkeypatch.setattr(hip_train, 'DGRAD_KERNEL', True)
    dgrad, pack = _Spy(hip.signw_conv2d_dgrad), _Spy(hip.pack_weight)
    monkeypatch.setattr(hip, 'signw_conv2d_dgrad', dgrad)
    monkeypatch.setattr(hip, 'pack_weight', pack)
    d = D.inputs(case.id)
    conv = _module(case, True)
    x = d['x'].to(DEV).requires_grad_()
    assert hip_train.supported(conv, x)
    y = conv(x)
    assert type(y.grad_fn).__name__ == STEP
    assert (dgrad.calls, pack.calls) == (0, 1)
    y.backward(d['gy'].to(DEV))
    assert (dgrad.calls, pack.calls) == (1, 1)        # one kernel call, nothing packed in backward

    twin = _twin_weight_scales(case)
    got = dict(conv.w_approximate.named_buffers())
    assert set(got) == set(twin)
    for name, buf in got.items():
        assert torch.equal(buf.cpu(), twin[name]) and float(buf.abs().sum()) > 0, name
    wscales = conv.w_approximate.plane_scales().detach().float().cpu()
    xscales = None
    if case.xs != 'fp':
        xscales = conv.last_act_scales.detach().cpu()
        assert tuple(xscales.shape) == (D.planes(case.xs), case.N)
    ref = _reference(case, xscales, wscales)

    ratios = {}
    err = (y.detach().cpu().double() - ref['y']).abs()
    ratios['y'] = _of_max(err, ref['y']) / BOUND_Y
    unit = ref['m_x'].abs() * ref['mag_x']
    err_x = (x.grad.cpu().double() - ref['gx']).abs()
    ratios['gx'] = _worst(err_x, unit) / BOUND_GX
    err_w = (conv.weight.grad.cpu().double() - ref['gw']).abs()
    ratios['gw'] = _of_max(err_w, ref['gw']) / BOUND_GW_MIOPEN
    if case.bias:
        err_b = (conv.bias.grad.cpu().double() - ref['gb']).abs()
        ratios['gb'] = _of_max(err_b, ref['gb']) / BOUND_GB
    print(f'\nconv-dgrad step ratios {case.id} ' + ' '.join(f'{k}={v:.4f}' for k, v in ratios.items())
          + f' zero_bound_gx={int((unit == 0).sum())}/{unit.numel()}')
    assert ratios['y'] <= 1.0, (case.id, 'y', ratios)
    assert bool((err_x <= BOUND_GX * unit + 1e-30).all()), (case.id, 'gx', ratios)
    assert ratios['gw'] <= 1.0, (case.id, 'gw', ratios)
    if case.bias:
        assert ratios['gb'] <= 1.0, (case.id, 'gb', ratios)
    else:
        assert conv.bias is None


# ------------------------------------------------------------------------------------------------------ (c) plumbing
PLUMB = D.BY_ID['s2_3x5']          # 20 -> 50, 3 x 5, stride 2, pad (2, 0), ls-2 activations
WBITS = 5                          # position of the step's weight planes among the saved tensors


def _grads(conv, x, y):
    return (y.detach().clone(), None if x.grad is None else x.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())


def test_two_forwards_of_one_module_before_one_backward(monkeypatch):
    """Each backward reads the weight planes, the input and the scales its own forward saved."""
    from quant.binary import hip_train
    monkeypatch.setattr(hip_train, 'DGRAD_KERNEL', True)
    d = D.inputs(PLUMB.id)
    x2_cpu = detgen.normal('cdgrad.plumb.x2', d['x'].shape, scale=0.6)
    g1, g2 = d['gy'].to(DEV), detgen.normal('cdgrad.plumb.g2', d['gy'].shape).to(DEV)
    singles = []
    for xc, g in ((d['x'], g1), (x2_cpu, g2)):
        conv = _module(PLUMB, True)
        x, y = _step(conv, xc, g)
        singles.append(_grads(conv, x, y))
    conv = _module(PLUMB, True)
    xa, xb = d['x'].to(DEV).requires_grad_(), x2_cpu.to(DEV).requires_grad_()
    ya, yb = conv(xa), conv(xb)
    wa, wb = ya.grad_fn.saved_tensors[WBITS], yb.grad_fn.saved_tensors[WBITS]
    assert wa.dtype == torch.int64 and wa.numel() > 0 and wa.data_ptr() != wb.data_ptr() and torch.equal(wa, wb)
    ((ya * g1).sum() + (yb * g2).sum()).backward()
    assert torch.equal(ya.detach(), singles[0][0]) and torch.equal(yb.detach(), singles[1][0])
    assert torch.equal(xa.grad, singles[0][1]) and torch.equal(xb.grad, singles[1][1])
    assert torch.equal(conv.weight.grad, singles[0][2] + singles[1][2])
    assert torch.equal(conv.bias.grad, singles[0][3] + singles[1][3])


def test_input_without_a_gradient_saves_and_launches_nothing(monkeypatch):
    from quant.binary import hip_train
    hip = _hip()
    monkeypatch.setattr(hip_train, 'DGRAD_KERNEL', True)
    d = D.inputs(PLUMB.id)
    conv = _module(PLUMB, True)
    xg, yg = _step(conv, d['x'], d['gy'])
    base = _grads(conv, xg, yg)
    dgrad = _Spy(hip.signw_conv2d_dgrad)
    monkeypatch.setattr(hip, 'signw_conv2d_dgrad', dgrad)
    conv = _module(PLUMB, True)
    x = d['x'].to(DEV)
    y = conv(x)
    assert type(y.grad_fn).__name__ == STEP and y.grad_fn.saved_tensors[WBITS].numel() == 0
    y.backward(d['gy'].to(DEV))
    assert dgrad.calls == 0 and x.grad is None
    assert torch.equal(y.detach(), base[0]) and torch.equal(conv.weight.grad, base[2]) and torch.equal(conv.bias.grad, base[3])


def test_with_the_switch_off_the_step_is_the_old_route_bit_for_bit(monkeypatch):
    from quant.binary import hip_train
    hip = _hip()
    assert hip_train.DGRAD_KERNEL is False
    d = D.inputs(PLUMB.id)
    conv = _module(PLUMB, True)
    x, y = _step(conv, d['x'], d['gy'])
    before = _grads(conv, x, y)                       # (made before the switch is touched)
    monkeypatch.setattr(hip_train, 'DGRAD_KERNEL', True)
    conv = _module(PLUMB, True)
    x, y = _step(conv, d['x'], d['gy'])
    on = _grads(conv, x, y)
    assert torch.equal(on[0], before[0]) and torch.equal(on[2], before[2]) and torch.equal(on[3], before[3])
    monkeypatch.setattr(hip_train, 'DGRAD_KERNEL', False)
    dgrad, pack = _Spy(hip.signw_conv2d_dgrad), _Spy(hip.pack_weight)
    monkeypatch.setattr(hip, 'signw_conv2d_dgrad', dgrad)
    monkeypatch.setattr(hip, 'pack_weight', pack)
    conv = _module(PLUMB, True)
    x = d['x'].to(DEV).requires_grad_()
    y = conv(x)
    assert y.grad_fn.saved_tensors[WBITS].numel() == 0
    y.backward(d['gy'].to(DEV))
    assert (dgrad.calls, pack.calls) == (0, 1 + D.planes(PLUMB.ws))      # the old route packs one plane set per weight plane
    after = _grads(conv, x, y)
    for a, b in zip(after, before):
        assert torch.equal(a, b)
    # widened geometries fall back to the torch formulation again
    wide = D.BY_ID['dil2']
    twin = _module(wide, True)
    xw, yw = _step(twin, D.inputs(wide.id)['x'], D.inputs(wide.id)['gy'])
    assert type(yw.grad_fn).__name__ != STEP
