"""lsq_signw_conv2d_dgrad_half on the GPU (liblsq_hip_conv_train_half.so) and QuantConv2d's 16-bit train step
(``hip_train_half``): (a) the kernel's three contracts bit for bit against the composition of the existing kernels on
``gy.float()`` / ``x.float()``, on every case of tests/golden/conv_train_half_cases.py in both types, from offset views too,
and against the fp64 reference; (b) the whole step against the same reference; (c) the plumbing.

No case is routed to another instantiation (every instantiation builds without scratch), so bit equality holds on all."""

import ctypes

import pytest
import torch

import conv_train_half_cases as H
import detgen

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STEP, STEP_HALF = '_QuantConv2dStepBackward', '_QuantConv2dStepHalfBackward'
# the bounds of tests/test_gpu_conv_dgrad.py, plus one rounding into the type (u = H.UNIT, fp16: + 2^-25, half its smallest subnormal)
BOUND_Y = 1e-5        # of max |y64|
BOUND_GX = 1e-5       # per element, of |m_x| mag_x
BOUND_GW_MIOPEN = 1e-5   # of max |gw64|
BOUND_GB = 1e-5       # of max |gb64|
SENTINEL = -7.25      # (a value of both types)
PAD = 64
DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
WORST = {}            # (what, type) -> worst ratio seen so far, printed as it grows


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


def _bits(t):
    """The tensor's bit patterns (so that -0 and +0 differ)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _note(what, dtype, ratio):
    key = (what, H.DTYPE_NAMES[dtype])
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    return f'worst so far {key[0]} {key[1]} {WORST[key]:.4f}'


def _worst(err, bound):
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def _of_max(err, ref64):
    top = float(ref64.abs().max())
    if top == 0.0:
        return 0.0 if float(err.max()) == 0.0 else float('inf')
    return float(err.max()) / top


_REFS = {}


def _reference(case, dtype, xscales, wscales):
    """step64 for given scales, computed once per (case, type, scales) and left unchanged."""
    key = (case.id, dtype, None if xscales is None else xscales.numpy().tobytes(), wscales.numpy().tobytes())
    if key not in _REFS:
        _REFS[key] = H.step64(case, dtype, None if xscales is None else list(xscales), list(wscales))
    return _REFS[key]


def _gx_bound(ref, dtype):
    """(bound, unit): unit = 1e-5 |m_x| mag_x, the fp32 kernels' bound; bound = (1 + u) unit + u |gx64| (+ 2^-25 for fp16)."""
    u = H.UNIT[dtype]
    unit = BOUND_GX * ref['m_x'].abs() * ref['mag_x']
    return (1 + u) * unit + u * ref['gx'].abs() + H.TINY[dtype], unit


# ------------------------------------------------------------------------------------------------- (a) the kernel alone
def _operands(hip, case, dtype):
    d = H.inputs(case.id, dtype)
    geom = _geom(hip, case)
    wsc_cpu = H.weight_scales(case.id)
    wsc = wsc_cpu.to(DEV)
    wbits, _ = hip.pack_weight(d['w'].to(DEV), geom, wsc)
    xs_cpu = torch.stack(d['xscales']) if d['xscales'] else None
    xs = None if xs_cpu is None else xs_cpu.to(DEV)
    return d, geom, wsc_cpu, wsc, wbits, xs_cpu, xs


@pytest.mark.parametrize('pair', H.PAIRS, ids=H.pair_id)
def test_kernel_contracts_hold_bit_for_bit(pair):
    """(A) x = NULL, fp32 out = lsq_signw_conv2d_dgrad(gy.float()); (B) x = NULL, 16-bit out = (A).to(dtype); (C) x given =
    lsq_ste_backward(x.float(), (A)).to(dtype) (and unrounded with an fp32 out).  Then straight through the C ABI with gy, x and
    grad_x as views one element into their buffers and a workspace of exactly the stated size between sentinels: the same
    bits, twice, and every sentinel intact."""
    case, dtype = pair
    hip = _hip()
    d, geom, _, wsc, wbits, _, xs = _operands(hip, case, dtype)
    gy, x, alpha = d['gy'].to(DEV), d['x'].to(DEV), d['alpha']
    a_ref = hip.signw_conv2d_dgrad(gy.float(), wbits, wsc, geom)
    c_ref = hip.ste_backward(x.float(), a_ref, xs, alpha)
    got_a = hip.signw_conv2d_dgrad_half(gy, wbits, wsc, geom, out_dtype=torch.float32)
    got_b = hip.signw_conv2d_dgrad_half(gy, wbits, wsc, geom)
    got_c = hip.signw_conv2d_dgrad_half(gy, wbits, wsc, geom, x, xs, alpha)
    got_c32 = hip.signw_conv2d_dgrad_half(gy, wbits, wsc, geom, x, xs, alpha, out_dtype=torch.float32)
    assert _same_bits(got_a, a_ref), 'A'
    assert _same_bits(got_b, a_ref.to(dtype)), 'B'
    assert _same_bits(got_c, c_ref.to(dtype)), 'C'
    assert _same_bits(got_c32, c_ref), 'C fp32'
    assert tuple(got_c.shape) == (case.N, case.C, case.H, case.W)

    lib = hip.conv_train_half_lib()
    kw, kx = wsc.shape[0], 0 if xs is None else xs.shape[0]
    need = int(lib.lsq_signw_conv2d_dgrad_half_workspace_bytes(ctypes.byref(geom), kw))
    assert need > 0 and need % 8 == 0
    (gy_buf, gy_v), (x_buf, x_v) = H.shifted(gy), H.shifted(x)
    assert gy_v.data_ptr() % 4 == 2 and x_v.data_ptr() % 4 == 2
    n = got_c.numel()
    wsbuf = torch.full((need + 16 * PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    ws_ptr = wsbuf.data_ptr() + 8 * PAD
    assert ws_ptr % 8 == 0
    for with_x, want in ((True, got_c), (False, got_b), (True, got_c)):
        out = torch.full((n + 1 + PAD,), SENTINEL, dtype=dtype, device=DEV)
        assert (out.data_ptr() + 2) % 4 == 2
        code = lib.lsq_signw_conv2d_dgrad_half(
            gy_v.data_ptr(), DT[dtype], wbits.data_ptr(), kw, wsc.data_ptr(), ctypes.byref(geom),
            x_v.data_ptr() if with_x else None, kx, None if xs is None else xs.data_ptr(), alpha, out.data_ptr() + 2, DT[dtype],
            ws_ptr, need, hip.stream_ptr(DEV))
        assert code == 0
        torch.cuda.synchronize()
        assert _same_bits(out[1:1 + n].view_as(want), want), with_x
        assert float(out[0]) == SENTINEL and bool((out[1 + n:] == SENTINEL).all())
        assert bool((wsbuf[:8 * PAD] == 0xA5).all()) and bool((wsbuf[8 * PAD + need:] == 0xA5).all())
    assert torch.equal(gy_v, gy) and torch.equal(x_v, x) and float(gy_buf[0]) == SENTINEL and float(x_buf[0]) == SENTINEL


@pytest.mark.parametrize('pair', H.PAIRS, ids=H.pair_id)
def test_kernel_with_the_estimator_equals_the_fp64_input_gradient(pair):
    """(C) against step64: |gx - gx64| <= (1 + u) 1e-5 |m_x| mag_x + u |gx64| per element, exactly +0 wherever that is 0, no
    case and no element set aside."""
    case, dtype = pair
    hip = _hip()
    d, geom, wsc_cpu, wsc, wbits, xs_cpu, xs = _operands(hip, case, dtype)
    ref = _reference(case, dtype, xs_cpu, wsc_cpu)
    got = hip.signw_conv2d_dgrad_half(d['gy'].to(DEV), wbits, wsc, geom, d['x'].to(DEV), xs, d['alpha'])
    assert got.dtype == dtype
    g = got.cpu()
    err = (g.double() - ref['gx']).abs()
    bound, unit = _gx_bound(ref, dtype)
    ratio = _worst(err, bound)
    zero = (unit == 0) & (ref['gx'] == 0)
    print(f'\nconv-train-half kernel ratio {H.pair_id(pair)} {ratio:.4f} zero_bound={int(zero.sum())}/{unit.numel()} '
          + _note('kernel gx', dtype, ratio))
    assert bool((err <= bound).all()), (H.pair_id(pair), ratio)
    assert bool((g[zero] == 0).all()) and not bool(torch.signbit(g[zero]).any()), H.pair_id(pair)


# ------------------------------------------------------------------------------------------ (b) the step, switch on
def _module(case, half=True):
    conv = H.make_module(case)
    conv.hip_train_half = half
    return conv.to(DEV).train()


@pytest.mark.parametrize('pair', H.PAIRS, ids=H.pair_id)
def test_train_step_equals_the_fp64_step(monkeypatch, pair):
    case, dtype = pair
    from quant.binary import hip_train
    hip = _hip()
    names = ('signw_conv2d_dgrad_half', 'act_quant_half', 'signw_conv2d_half', 'act_quant', 'signw_conv2d', 'signw_conv2d_dgrad',
             'pack_weight', 'xnor_conv2d')
    spy = {n: _Spy(getattr(hip, n)) for n in names}
    for n, s in spy.items():
        monkeypatch.setattr(hip, n, s)
    d = H.inputs(case.id, dtype)
    conv = _module(case)
    x = d['x'].to(DEV).requires_grad_()
    assert hip_train.supported(conv, x) and not conv.act_half and not conv.fp_half
    y = conv(x)
    assert type(y.grad_fn).__name__ == STEP_HALF and y.dtype == dtype
    fp = case.xs == 'fp'
    calls = {n: s.calls for n, s in spy.items()}
    assert calls == dict(signw_conv2d_dgrad_half=0, act_quant_half=0 if fp else 1, signw_conv2d_half=1 if fp else 0, act_quant=0,
                         signw_conv2d=0, signw_conv2d_dgrad=0, pack_weight=1, xnor_conv2d=0 if fp else 1), calls
    y.backward(d['gy'].to(DEV))
    calls = {n: s.calls for n, s in spy.items()}
    assert calls == dict(signw_conv2d_dgrad_half=1, act_quant_half=0 if fp else 1, signw_conv2d_half=1 if fp else 0, act_quant=0,
                         signw_conv2d=0, signw_conv2d_dgrad=0, pack_weight=1, xnor_conv2d=0 if fp else 1), calls
    assert x.grad.dtype == dtype and conv.weight.grad.dtype == torch.float32
    assert conv.bias is None or conv.bias.grad.dtype == torch.float32

    wscales = conv.w_approximate.plane_scales().detach().float().cpu()
    xscales = None
    if not fp:
        xscales = conv.last_act_scales.detach().cpu()
        assert tuple(xscales.shape) == (H.planes(case.xs), case.N)
    ref = _reference(case, dtype, xscales, wscales)
    u = H.UNIT[dtype]
    ratios = {}
    err_y = (y.detach().cpu().double() - ref['y']).abs()
    bound_y = (1 + u) * BOUND_Y * float(ref['y'].abs().max()) + u * ref['y'].abs() + H.TINY[dtype]
    ratios['y'] = _worst(err_y, bound_y)
    err_x = (x.grad.cpu().double() - ref['gx']).abs()
    bound_x, unit = _gx_bound(ref, dtype)
    ratios['gx'] = _worst(err_x, bound_x)
    err_w = (conv.weight.grad.cpu().double() - ref['gw']).abs()
    ratios['gw'] = _of_max(err_w, ref['gw']) / BOUND_GW_MIOPEN
    if case.bias:
        err_b = (conv.bias.grad.cpu().double() - ref['gb']).abs()
        ratios['gb'] = _of_max(err_b, ref['gb']) / BOUND_GB
    print(f'\nconv-train-half step ratios {H.pair_id(pair)} ' + ' '.join(f'{k}={v:.4f}' for k, v in ratios.items()) + ' '
          + _note('step y', dtype, ratios['y']) + ' ' + _note('step gx', dtype, ratios['gx']))
    assert bool((err_y <= bound_y).all()), (H.pair_id(pair), 'y', ratios)
    assert bool((err_x <= bound_x).all()), (H.pair_id(pair), 'gx', ratios)
    zero = (unit == 0) & (ref['gx'] == 0)
    gx = x.grad.cpu()
    assert bool((gx[zero] == 0).all()) and not bool(torch.signbit(gx[zero]).any())
    assert ratios['gw'] <= 1.0, (H.pair_id(pair), 'gw', ratios)
    if case.bias:
        assert ratios['gb'] <= 1.0, (H.pair_id(pair), 'gb', ratios)


@pytest.mark.parametrize('dtype', H.DTYPES, ids=lambda t: H.DTYPE_NAMES[t])
def test_train_step_with_the_weight_gradient_kernel(monkeypatch, dtype):
    """WGRAD_KERNEL: the step keeps its activation planes and grad_w takes lsq_train_wgrad on gy.float()."""
    from quant.binary import hip_train
    hip = _hip()
    case = H.BY_ID['s2_3x5']
    monkeypatch.setattr(hip_train, 'WGRAD_KERNEL', True)
    wgrad = _Spy(hip.wgrad)
    monkeypatch.setattr(hip, 'wgrad', wgrad)
    d = H.inputs(case.id, dtype)
    conv = _module(case)
    x = d['x'].to(DEV).requires_grad_()
    y = conv(x)
    assert type(y.grad_fn).__name__ == STEP_HALF and y.grad_fn.saved_tensors[4].numel() > 0
    y.backward(d['gy'].to(DEV))
    assert wgrad.calls == 1
    ref = _reference(case, dtype, conv.last_act_scales.detach().cpu(), conv.w_approximate.plane_scales().detach().float().cpu())
    err_w = (conv.weight.grad.cpu().double() - ref['gw']).abs()
    # BOUND_GW_KERNEL of tests/test_gpu_train_geometries.py: 2e-6 of |m_w| mag_w per element (gy.float() is exact)
    assert bool((err_w <= 2e-6 * ref['m_w'].abs() * ref['mag_w'] + 1e-30).all())


# ------------------------------------------------------------------------------------------------------ (c) plumbing
PLUMB = H.BY_ID['s2_3x5']          # 20 -> 50, 3 x 5, stride 2, pad (2, 0), ls-2 activations
WBITS = 5                          # position of the step's weight planes among the saved tensors
BF = torch.bfloat16


def _step(conv, x, gy):
    x = x.to(DEV).requires_grad_()
    y = conv(x)
    y.backward(gy.to(DEV))
    return x, y


def _grads(conv, x, y):
    return (y.detach().clone(), None if x.grad is None else x.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())


def test_two_forwards_of_one_module_before_one_backward():
    """Each backward reads the weight planes, the input and the scales its own forward saved."""
    d = H.inputs(PLUMB.id, BF)
    x2_cpu = detgen.normal('cthalf.plumb.x2', d['x'].shape, scale=0.6).to(BF)
    g1, g2 = d['gy'].to(DEV), detgen.normal('cthalf.plumb.g2', d['gy'].shape).to(BF).to(DEV)
    singles = []
    for xc, g in ((d['x'], g1), (x2_cpu, g2)):
        conv = _module(PLUMB)
        x, y = _step(conv, xc, g)
        singles.append(_grads(conv, x, y))
    conv = _module(PLUMB)
    xa, xb = d['x'].to(DEV).requires_grad_(), x2_cpu.to(DEV).requires_grad_()
    ya, yb = conv(xa), conv(xb)
    assert type(ya.grad_fn).__name__ == STEP_HALF
    wa, wb = ya.grad_fn.saved_tensors[WBITS], yb.grad_fn.saved_tensors[WBITS]
    assert wa.dtype == torch.int64 and wa.numel() > 0 and wa.data_ptr() != wb.data_ptr() and torch.equal(wa, wb)
    torch.autograd.backward([ya, yb], [g1, g2])
    assert _same_bits(ya.detach(), singles[0][0]) and _same_bits(yb.detach(), singles[1][0])
    assert _same_bits(xa.grad, singles[0][1]) and _same_bits(xb.grad, singles[1][1])
    assert torch.equal(conv.weight.grad, singles[0][2] + singles[1][2])
    assert torch.equal(conv.bias.grad, singles[0][3] + singles[1][3])


def test_input_without_a_gradient_saves_and_launches_nothing(monkeypatch):
    hip = _hip()
    d = H.inputs(PLUMB.id, BF)
    conv = _module(PLUMB)
    xg, yg = _step(conv, d['x'], d['gy'])
    base = _grads(conv, xg, yg)
    dgrad = _Spy(hip.signw_conv2d_dgrad_half)
    monkeypatch.setattr(hip, 'signw_conv2d_dgrad_half', dgrad)
    conv = _module(PLUMB)
    x = d['x'].to(DEV)
    y = conv(x)
    assert type(y.grad_fn).__name__ == STEP_HALF and y.grad_fn.saved_tensors[WBITS].numel() == 0
    y.backward(d['gy'].to(DEV))
    assert dgrad.calls == 0 and x.grad is None
    assert _same_bits(y.detach(), base[0]) and torch.equal(conv.weight.grad, base[2]) and torch.equal(conv.bias.grad, base[3])


def test_with_the_switch_off_a_16_bit_input_takes_the_torch_formulation(monkeypatch):
    from quant.binary import hip_train
    from quant.binary.binary_conv import QuantConv2d
    hip = _hip()
    assert QuantConv2d.hip_train_half is False
    dgrad = _Spy(hip.signw_conv2d_dgrad_half)
    monkeypatch.setattr(hip, 'signw_conv2d_dgrad_half', dgrad)
    d = H.inputs(PLUMB.id, BF)
    for eval_switches in (False, True):               # act_half / fp_half are eval switches: they do not bring the step
        conv = _module(PLUMB, half=False)
        conv.act_half = conv.fp_half = eval_switches
        x = d['x'].to(DEV).requires_grad_()
        assert not hip_train.supported(conv, x)
        with torch.autocast('cuda', BF):              # (fp32 weights against a bf16 input: torch needs autocast to decide the types)
            y = conv(x)
        assert type(y.grad_fn).__name__ not in (STEP, STEP_HALF)
        y.backward(d['gy'].to(DEV).to(y.dtype))
        assert dgrad.calls == 0 and x.grad is not None


def test_the_fp32_step_is_unchanged_by_the_switch(monkeypatch):
    """The same launches and the same bits for an fp32 input, with the switch on or off."""
    hip = _hip()
    import conv_dgrad_cases as D
    d = D.inputs(PLUMB.id)
    out = []
    for half in (False, True):
        names = ('act_quant', 'xnor_conv2d', 'signw_conv2d', 'pack_weight', 'ste_backward', 'quant_values', 'act_quant_half',
                 'signw_conv2d_half', 'signw_conv2d_dgrad_half', 'signw_conv2d_dgrad')
        spy = {n: _Spy(getattr(hip, n)) for n in names}
        with monkeypatch.context() as m:
            for n, s in spy.items():
                m.setattr(hip, n, s)
            conv = _module(PLUMB, half=half)
            x, y = _step(conv, d['x'], d['gy'])
        assert type(y.grad_fn).__name__ == STEP and y.dtype == torch.float32
        out.append((_grads(conv, x, y), {n: s.calls for n, s in spy.items()}))
    for a, b in zip(out[0][0], out[1][0]):
        assert _same_bits(a, b)
    assert out[0][1] == out[1][1]
    assert out[1][1]['act_quant_half'] == out[1][1]['signw_conv2d_half'] == out[1][1]['signw_conv2d_dgrad_half'] == 0


def test_autocast_rule_of_supported():
    from quant.binary import hip_train
    d = H.inputs(PLUMB.id, BF)
    conv = _module(PLUMB)
    xb, xh = d['x'].to(DEV), d['x'].to(DEV).half()
    assert hip_train.supported(conv, xb) and hip_train.supported(conv, xh)
    with torch.autocast('cuda', BF):
        assert hip_train.supported(conv, xb) and not hip_train.supported(conv, xh)
    with torch.autocast('cuda', torch.float16):
        assert hip_train.supported(conv, xh) and not hip_train.supported(conv, xb)


def test_under_bf16_autocast_a_small_stack_takes_the_step(monkeypatch):
    """conv -> bn -> QuantConv2d under torch.autocast('cuda', torch.bfloat16): the quantized layer is handed bf16 and takes the
    16-bit step, forward and backward; with the switch off the same stack takes the torch formulation."""
    from quant.binary.binary_conv import QuantConv2d
    hip = _hip()
    dgrad, quant = _Spy(hip.signw_conv2d_dgrad_half), _Spy(hip.act_quant_half)
    monkeypatch.setattr(hip, 'signw_conv2d_dgrad_half', dgrad)
    monkeypatch.setattr(hip, 'act_quant_half', quant)
    seen = {}

    def build(half):
        torch.manual_seed(5)
        q = QuantConv2d('ls-2', 'ls-1', 8, 16, 3, {'kind': 'symmetric', 'alpha': 2}, padding=1, bias=True)
        q.hip_train_half = half
        q.register_forward_hook(lambda m, i, o: seen.update(x=i[0].dtype, y=o.dtype, fn=type(o.grad_fn).__name__))
        return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.BatchNorm2d(8), q).to(DEV).train()
    x = detgen.normal('cthalf.stack.x', (2, 3, 9, 8)).to(DEV)
    for half in (True, False):
        net = build(half)
        with torch.autocast('cuda', BF):
            y = net(x)
        assert seen['x'] == BF and y.dtype == BF
        assert (seen['fn'] == STEP_HALF) == half
        y.float().square().mean().backward()
        grads = [p.grad for p in net.parameters()]
        assert all(g is not None and g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in grads)
        assert float(net[0].weight.grad.abs().max()) > 0
    assert (dgrad.calls, quant.calls) == (1, 1)
