"""lsq_linear_signw_dgrad_half on the GPU (liblsq_hip_linear_train_half.so) and QuantLinear's 16-bit train step
(``hip_train_half``): (a) the kernel's three contracts bit for bit against the composition of the existing kernels on
``gy.float()`` / ``x.float()``, on every case of tests/golden/linear_train_half_cases.py in both types, from offset views too,
and against the fp64 reference; (b) the whole step against the same reference; (c) the plumbing.

Bounds.  The fp32 kernel is held to 1e-5 of max |gxq64| (tests/test_gpu_linear_train.py); the estimator multiplies that error
by |m_x|, and one rounding into the type adds u |result| (u = 2^-8 bf16, 2^-11 fp16; fp16 also half its smallest subnormal,
2^-25):  |gx - gx64| <= (1 + u) 1e-5 |m_x| max |gxq64| + u |gx64| + tiny per element."""

import ctypes

import pytest
import torch

import detgen
import linear_train_half_cases as L

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STEP, STEP_HALF = '_QuantLinearStepBackward', '_QuantLinearStepHalfBackward'
BOUND = 1e-5          # of max |.64|: the fp32 kernels' bound (tests/test_gpu_linear_train.py)
SENTINEL = -7.25      # (a value of both types)
PAD = 64
DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
BF = torch.bfloat16
WORST = {}            # (what, type) -> worst ratio seen so far, printed as it grows


def _hip():
    from quant import _hip
    return _hip


class _Spy:
    def __init__(self, fn):
        self.fn, self.calls, self.args = fn, 0, None

    def __call__(self, *a, **k):
        self.calls += 1
        self.args = a
        return self.fn(*a, **k)


def _bits(t):
    """The tensor's bit patterns (so that -0 and +0 differ)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _note(what, dtype, ratio):
    key = (what, L.DTYPE_NAMES[dtype])
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
        _REFS[key] = L.step64(case, dtype, None if xscales is None else list(xscales), list(wscales))
    return _REFS[key]


def _gx_bound(ref, dtype):
    """(bound, unit): unit = 1e-5 |m_x| max |gxq64|; bound = (1 + u) unit + u |gx64| (+ 2^-25 for fp16)."""
    u = L.UNIT[dtype]
    unit = BOUND * ref['m_x'].abs() * float(ref['gxq'].abs().max())
    return (1 + u) * unit + u * ref['gx'].abs() + L.TINY[dtype], unit


# ------------------------------------------------------------------------------------------------- (a) the kernel alone
def _operands(hip, case, dtype):
    d = L.inputs(case.id, dtype)
    m, f, o = case.N * case.T, case.F, case.O
    geom = hip.make_geom(1, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    wsc_cpu = L.weight_scales(case.id)
    wsc = wsc_cpu.to(DEV)
    wbits, _ = hip.pack_weight(d['w'].to(DEV).view(o, f, 1, 1), geom, wsc)
    xs_cpu = torch.stack(d['xscales']) if d['xscales'] else None
    xs = None if xs_cpu is None else xs_cpu.to(DEV)
    return d, (m, f, o), wsc_cpu, wsc, wbits, xs_cpu, xs


@pytest.mark.parametrize('pair', L.PAIRS, ids=L.pair_id)
def test_kernel_contracts_hold_bit_for_bit(pair):
    """(A) x = NULL, fp32 out = lsq_linear_signw_dgrad(gy.float()); (B) x = NULL, 16-bit out = (A).to(dtype); (C) x given =
    lsq_ste_backward(x.float() viewed [N, T F], (A)).to(dtype) (and unrounded with an fp32 out).  Then straight through the C
    ABI with gy, x and gx as views one element into their buffers and a workspace of exactly the stated size between
    sentinels: the same bits, twice, and every sentinel intact."""
    case, dtype = pair
    hip = _hip()
    d, (m, f, o), _, wsc, wbits, _, xs = _operands(hip, case, dtype)
    n, t = case.N, case.T
    gy, x, alpha = d['gy'].to(DEV).view(m, o), d['x'].to(DEV).view(m, f), d['alpha']
    a_ref = hip.linear_signw_dgrad(gy.float(), wbits, wsc, m, f, o)
    c_ref = hip.ste_backward(x.float().view(n, t * f), a_ref.view(n, t * f), xs, alpha).view(m, f)
    got_a = hip.linear_signw_dgrad_half(gy, wbits, wsc, m, f, o, out_dtype=torch.float32)
    got_b = hip.linear_signw_dgrad_half(gy, wbits, wsc, m, f, o)
    got_c = hip.linear_signw_dgrad_half(gy, wbits, wsc, m, f, o, x, xs, alpha, T=t)
    got_c32 = hip.linear_signw_dgrad_half(gy, wbits, wsc, m, f, o, x, xs, alpha, T=t, out_dtype=torch.float32)
    assert _same_bits(got_a, a_ref), 'A'
    assert _same_bits(got_b, a_ref.to(dtype)), 'B'
    assert _same_bits(got_c, c_ref.to(dtype)), 'C'
    assert _same_bits(got_c32, c_ref), 'C fp32'
    assert tuple(got_c.shape) == (m, f)

    lib = hip.linear_train_half_lib()
    kw, kx = wsc.shape[0], 0 if xs is None else xs.shape[0]
    need = int(lib.lsq_linear_signw_dgrad_half_workspace_bytes(kw, f, o))
    assert need > 0 and need % 8 == 0
    (gy_buf, gy_v), (x_buf, x_v) = L.shifted(gy), L.shifted(x)
    assert gy_v.data_ptr() % 4 == 2 and x_v.data_ptr() % 4 == 2
    cnt = m * f
    wsbuf = torch.full((need + 16 * PAD,), 0xA5, dtype=torch.uint8, device=DEV)
    ws_ptr = wsbuf.data_ptr() + 8 * PAD
    assert ws_ptr % 8 == 0
    for with_x, want in ((True, got_c), (False, got_b), (True, got_c)):
        out = torch.full((cnt + 1 + PAD,), SENTINEL, dtype=dtype, device=DEV)
        assert (out.data_ptr() + 2) % 4 == 2
        code = lib.lsq_linear_signw_dgrad_half(
            gy_v.data_ptr(), DT[dtype], wbits.data_ptr(), kw, wsc.data_ptr(), m, f, o, x_v.data_ptr() if with_x else None, t, kx,
            None if xs is None else xs.data_ptr(), alpha, out.data_ptr() + 2, DT[dtype], ws_ptr, need, hip.stream_ptr(DEV))
        assert code == 0
        torch.cuda.synchronize()
        assert _same_bits(out[1:1 + cnt].view_as(want), want), with_x
        assert float(out[0]) == SENTINEL and bool((out[1 + cnt:] == SENTINEL).all())
        assert bool((wsbuf[:8 * PAD] == 0xA5).all()) and bool((wsbuf[8 * PAD + need:] == 0xA5).all())
    assert torch.equal(gy_v, gy) and torch.equal(x_v, x) and float(gy_buf[0]) == SENTINEL and float(x_buf[0]) == SENTINEL
    assert bool((gy_buf[1 + gy.numel():] == SENTINEL).all()) and bool((x_buf[1 + x.numel():] == SENTINEL).all())


@pytest.mark.parametrize('pair', L.PAIRS, ids=L.pair_id)
def test_kernel_with_the_estimator_equals_the_fp64_input_gradient(pair):
    """(C) against step64: |gx - gx64| <= (1 + u) 1e-5 |m_x| max |gxq64| + u |gx64| + tiny per element, exactly +0 wherever
    m_x = 0 and gx64 = 0, no case and no element set aside."""
    case, dtype = pair
    hip = _hip()
    d, (m, f, o), wsc_cpu, wsc, wbits, xs_cpu, xs = _operands(hip, case, dtype)
    ref = _reference(case, dtype, xs_cpu, wsc_cpu)
    got = hip.linear_signw_dgrad_half(d['gy'].to(DEV).view(m, o), wbits, wsc, m, f, o, d['x'].to(DEV).view(m, f), xs, d['alpha'],
                                      T=case.T)
    assert got.dtype == dtype
    g = got.cpu().view(L.x_shape(case))
    err = (g.double() - ref['gx']).abs()
    bound, unit = _gx_bound(ref, dtype)
    ratio = _worst(err, bound)
    zero = (ref['m_x'] == 0) & (ref['gx'] == 0)
    print(f'\nlinear-train-half kernel ratio {L.pair_id(pair)} {ratio:.4f} zero_bound={int(zero.sum())}/{unit.numel()} '
          + _note('kernel gx', dtype, ratio))
    assert bool((err <= bound).all()), (L.pair_id(pair), ratio)
    assert bool((g[zero] == 0).all()) and not bool(torch.signbit(g[zero]).any()), L.pair_id(pair)


# ------------------------------------------------------------------------------------------ (b) the step, switch on
def _module(case, half=True, fp32=False):
    lin = L.make_module(case)
    lin.hip_train_half = half
    lin.hip_train = fp32
    return lin.to(DEV).train()


STEP_NAMES = ('linear_signw_dgrad_half', 'act_quant_half', 'linear_signw_half', 'act_quant', 'linear_signw', 'linear_signw_dgrad',
              'pack_weight', 'linear_xnor')


@pytest.mark.parametrize('pair', L.PAIRS, ids=L.pair_id)
def test_train_step_equals_the_fp64_step(monkeypatch, pair):
    case, dtype = pair
    from quant.binary import hip_train_linear
    hip = _hip()
    spy = {n: _Spy(getattr(hip, n)) for n in STEP_NAMES}
    for n, s in spy.items():
        monkeypatch.setattr(hip, n, s)
    d = L.inputs(case.id, dtype)
    lin = _module(case)
    x = d['x'].to(DEV).requires_grad_()
    assert hip_train_linear.supported(lin, x) and not lin.hip_train and not lin.act_half_solve
    y = lin(x)
    assert type(y.grad_fn).__name__ == STEP_HALF and y.dtype == dtype and tuple(y.shape) == L.gy_shape(case)
    fp = case.xs == 'fp'
    want = dict(linear_signw_dgrad_half=0, act_quant_half=0 if fp else 1, linear_signw_half=1 if fp else 0, act_quant=0,
                linear_signw=0, linear_signw_dgrad=0, pack_weight=1, linear_xnor=0 if fp else 1)
    assert {n: s.calls for n, s in spy.items()} == want
    y.backward(d['gy'].to(DEV))
    assert {n: s.calls for n, s in spy.items()} == dict(want, linear_signw_dgrad_half=1)
    assert x.grad.dtype == dtype and lin.weight.grad.dtype == torch.float32
    assert lin.bias is None or lin.bias.grad.dtype == torch.float32

    wscales = lin.w_approximate.plane_scales().detach().float().cpu()
    xscales = None
    if not fp:
        xscales = lin.last_act_scales.detach().cpu()
        assert tuple(xscales.shape) == (L.planes(case.xs), case.N)
    ref = _reference(case, dtype, xscales, wscales)
    u = L.UNIT[dtype]
    ratios = {}
    err_y = (y.detach().cpu().double() - ref['y']).abs()
    bound_y = (1 + u) * BOUND * float(ref['y'].abs().max()) + u * ref['y'].abs() + L.TINY[dtype]
    ratios['y'] = _worst(err_y, bound_y)
    err_x = (x.grad.cpu().double() - ref['gx']).abs()
    bound_x, _ = _gx_bound(ref, dtype)
    ratios['gx'] = _worst(err_x, bound_x)
    ratios['gw'] = _of_max((lin.weight.grad.cpu().double() - ref['gw']).abs(), ref['gw']) / BOUND
    if case.bias:
        ratios['gb'] = _of_max((lin.bias.grad.cpu().double() - ref['gb']).abs(), ref['gb']) / BOUND
    print(f'\nlinear-train-half step ratios {L.pair_id(pair)} ' + ' '.join(f'{k}={v:.4f}' for k, v in ratios.items()) + ' '
          + _note('step y', dtype, ratios['y']) + ' ' + _note('step gx', dtype, ratios['gx']))
    assert bool((err_y <= bound_y).all()), (L.pair_id(pair), 'y', ratios)
    assert bool((err_x <= bound_x).all()), (L.pair_id(pair), 'gx', ratios)
    zero = (ref['m_x'] == 0) & (ref['gx'] == 0)
    gx = x.grad.cpu()
    assert bool((gx[zero] == 0).all()) and not bool(torch.signbit(gx[zero]).any())
    assert ratios['gw'] <= 1.0, (L.pair_id(pair), 'gw', ratios)
    if case.bias:
        assert ratios['gb'] <= 1.0, (L.pair_id(pair), 'gb', ratios)


# ------------------------------------------------------------------------------------------------------ (c) plumbing
PLUMB = L.BY_ID['rows_per_sample']          # [3, 5, 64] -> 130, ls-1 activations, gf-8 weights
PLUMB2 = L.BY_ID['odd_rows']                # [3, 35] -> 63, ls-2 activations
WBITS = 4                                   # position of the step's weight planes among the saved tensors


def _step(lin, x, gy):
    x = x.to(DEV).requires_grad_()
    y = lin(x)
    y.backward(gy.to(DEV))
    return x, y


def _grads(lin, x, y):
    return (y.detach().clone(), None if x.grad is None else x.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone())


@pytest.mark.parametrize('case', [PLUMB, PLUMB2], ids=lambda c: c.id)
def test_two_forwards_of_one_module_before_both_backwards(case):
    """Each backward reads the weight planes, the input and the scales its own forward saved."""
    d = L.inputs(case.id, BF)
    x2_cpu = detgen.normal('lthalf.plumb.x2', d['x'].shape, scale=0.6).to(BF)
    g1, g2 = d['gy'].to(DEV), detgen.normal('lthalf.plumb.g2', d['gy'].shape).to(BF).to(DEV)
    singles = []
    for xc, g in ((d['x'], g1), (x2_cpu, g2)):
        lin = _module(case)
        x, y = _step(lin, xc, g)
        singles.append(_grads(lin, x, y))
    lin = _module(case)
    xa, xb = d['x'].to(DEV).requires_grad_(), x2_cpu.to(DEV).requires_grad_()
    ya, yb = lin(xa), lin(xb)
    assert type(ya.grad_fn).__name__ == STEP_HALF
    wa, wb = ya.grad_fn.saved_tensors[WBITS], yb.grad_fn.saved_tensors[WBITS]
    assert wa.dtype == torch.int64 and wa.numel() > 0 and wa.data_ptr() != wb.data_ptr() and torch.equal(wa, wb)
    torch.autograd.backward([ya, yb], [g1, g2])
    assert _same_bits(ya.detach(), singles[0][0]) and _same_bits(yb.detach(), singles[1][0])
    assert _same_bits(xa.grad, singles[0][1]) and _same_bits(xb.grad, singles[1][1])
    sums = (singles[0][2] + singles[1][2], singles[1][2] + singles[0][2])      # (whichever backward ran first)
    assert any(torch.equal(lin.weight.grad, s) for s in sums)
    assert torch.equal(lin.bias.grad, singles[0][3] + singles[1][3])


def test_input_without_a_gradient_saves_and_launches_nothing(monkeypatch):
    hip = _hip()
    d = L.inputs(PLUMB.id, BF)
    lin = _module(PLUMB)
    xg, yg = _step(lin, d['x'], d['gy'])
    base = _grads(lin, xg, yg)
    dgrad = _Spy(hip.linear_signw_dgrad_half)
    monkeypatch.setattr(hip, 'linear_signw_dgrad_half', dgrad)
    lin = _module(PLUMB)
    x = d['x'].to(DEV)
    y = lin(x)
    assert type(y.grad_fn).__name__ == STEP_HALF and y.grad_fn.saved_tensors[WBITS].numel() == 0
    y.backward(d['gy'].to(DEV))
    assert dgrad.calls == 0 and x.grad is None
    assert _same_bits(y.detach(), base[0]) and torch.equal(lin.weight.grad, base[2]) and torch.equal(lin.bias.grad, base[3])


def test_with_the_switch_off_a_16_bit_input_takes_the_torch_formulation(monkeypatch):
    from quant.binary import hip_train_linear
    from quant.binary.binary_linear import QuantLinear
    hip = _hip()
    assert QuantLinear.hip_train_half is False
    dgrad = _Spy(hip.linear_signw_dgrad_half)
    monkeypatch.setattr(hip, 'linear_signw_dgrad_half', dgrad)
    d = L.inputs(PLUMB.id, BF)
    for fp32_switch in (False, True):                 # hip_train is the fp32 inputs' switch: it does not bring the 16-bit step
        lin = _module(PLUMB, half=False, fp32=fp32_switch)
        x = d['x'].to(DEV).requires_grad_()
        assert not hip_train_linear.supported(lin, x)
        with torch.autocast('cuda', BF):              # (fp32 weights against a bf16 input: torch needs autocast to decide the types)
            y = lin(x)
        assert type(y.grad_fn).__name__ not in (STEP, STEP_HALF)
        y.backward(d['gy'].to(DEV).to(y.dtype))
        assert dgrad.calls == 0 and x.grad is not None


def test_the_fp32_step_is_unchanged_by_the_switch(monkeypatch):
    """The same launches and the same bits for an fp32 input, with the switch on or off; with the 16-bit switch alone an fp32
    input stays on the torch formulation."""
    hip = _hip()
    d = L.inputs(PLUMB.id, BF)
    xf, gf = d['x'].float(), d['gy'].float()
    out = []
    names = ('act_quant', 'linear_xnor', 'linear_signw', 'pack_weight', 'ste_backward', 'quant_values', 'act_quant_half',
             'linear_signw_half', 'linear_signw_dgrad_half', 'linear_signw_dgrad')
    for half in (False, True):
        spy = {n: _Spy(getattr(hip, n)) for n in names}
        with monkeypatch.context() as mp:
            for n, s in spy.items():
                mp.setattr(hip, n, s)
            lin = _module(PLUMB, half=half, fp32=True)
            x, y = _step(lin, xf, gf)
        assert type(y.grad_fn).__name__ == STEP and y.dtype == torch.float32
        out.append((_grads(lin, x, y), {n: s.calls for n, s in spy.items()}))
    for a, b in zip(out[0][0], out[1][0]):
        assert _same_bits(a, b)
    assert out[0][1] == out[1][1] and out[1][1]['linear_signw_dgrad'] == 1
    assert out[1][1]['act_quant_half'] == out[1][1]['linear_signw_half'] == out[1][1]['linear_signw_dgrad_half'] == 0
    lin = _module(PLUMB, half=True, fp32=False)
    x, y = _step(lin, xf, gf)
    assert type(y.grad_fn).__name__ not in (STEP, STEP_HALF)


def test_autocast_rule_of_supported():
    from quant.binary import hip_train_linear
    d = L.inputs(PLUMB.id, BF)
    lin = _module(PLUMB)
    xb, xh = d['x'].to(DEV), d['x'].to(DEV).half()
    assert hip_train_linear.supported(lin, xb) and hip_train_linear.supported(lin, xh)
    with torch.autocast('cuda', BF):
        assert hip_train_linear.supported(lin, xb) and not hip_train_linear.supported(lin, xh)
    with torch.autocast('cuda', torch.float16):
        assert hip_train_linear.supported(lin, xh) and not hip_train_linear.supported(lin, xb)


@pytest.mark.parametrize('mode', ['eval_only', 'train_and_eval'])
def test_moving_average_modes_track_the_scales_as_the_fp32_step_does(mode):
    """Three steps of the 16-bit step on bf16 inputs beside the fp32 step on the same values: the tracked scales agree (the
    quantizer's scales of a 16-bit row are those of the row as fp32), 'train_and_eval' quantizes with the tracked values."""
    from quant.binary import QuantLinear
    mods = []
    for half in (True, False):
        lin = QuantLinear('ls-2', 'ls-1', 128, 40, {'kind': 'symmetric', 'alpha': 3}, mode, 0.9)
        with torch.no_grad():
            lin.weight.copy_(detgen.normal('lthalf.ma.w', lin.weight.shape, scale=0.3))
            lin.bias.copy_(detgen.normal('lthalf.ma.b', lin.bias.shape, scale=0.1))
        lin.hip_train_half, lin.hip_train = half, not half
        mods.append(lin.to(DEV).train())
    for step in range(3):
        xb = detgen.normal(f'lthalf.ma.x{step}', (6, 3, 128), scale=1.1).to(BF).to(DEV)
        ys = []
        for lin, x in zip(mods, (xb, xb.float())):
            x = x.clone().requires_grad_()
            y = lin(x)
            y.float().sum().backward()
            ys.append((y.detach(), x.grad, type(y.grad_fn).__name__))
        assert ys[0][2] == STEP_HALF and ys[1][2] == STEP
        ma = [m.x_approximate.moving_avg_module.moving_average for m in mods]
        assert torch.allclose(ma[0], ma[1], rtol=2e-6), (step, ma)
        assert torch.allclose(mods[0].last_act_scales, mods[1].last_act_scales, rtol=2e-6)
        # one rounding of y into bf16 on top of the fp32 step's value
        assert float((ys[0][0].float() - ys[1][0]).abs().max()) <= 2.0 ** -8 * float(ys[1][0].abs().max()) * (1 + 1e-3)


def test_wgrad_kernel_routes_the_weight_gradient_to_the_float_copies(monkeypatch):
    from quant.binary import hip_train_linear
    hip = _hip()
    case = L.BY_ID['tiles64_t4']
    monkeypatch.setattr(hip_train_linear, 'WGRAD_KERNEL', True)
    wgrad, mm = _Spy(hip.linear_signx_wgrad), _Spy(hip.quant_values)
    monkeypatch.setattr(hip, 'linear_signx_wgrad', wgrad)
    monkeypatch.setattr(hip, 'quant_values', mm)
    d = L.inputs(case.id, BF)
    lin = _module(case)
    x, y = _step(lin, d['x'], d['gy'])
    assert type(y.grad_fn).__name__ == STEP_HALF and (wgrad.calls, mm.calls) == (1, 0)
    assert wgrad.args[0].dtype == torch.float32 and wgrad.args[1].dtype == torch.float32
    assert torch.equal(wgrad.args[0], d['gy'].to(DEV).float().view(-1, case.O))
    ref = _reference(case, BF, lin.last_act_scales.detach().cpu(), lin.w_approximate.plane_scales().detach().float().cpu())
    assert _of_max((lin.weight.grad.cpu().double() - ref['gw']).abs(), ref['gw']) <= BOUND


def test_more_than_65535_samples_are_refused_on_the_host(monkeypatch):
    from quant.binary import hip_train_linear
    from quant.binary.binary_linear import QuantLinear
    hip = _hip()
    names = ('act_quant_half', 'linear_signw_dgrad_half', 'pack_weight')
    spy = {n: _Spy(getattr(hip, n)) for n in names}
    for n, s in spy.items():
        monkeypatch.setattr(hip, n, s)
    lin = QuantLinear('ls-1', 'ls-1', 64, 16, dict(L.SYM2))
    lin.hip_train_half = True
    lin = lin.to(DEV).train()
    assert hip_train_linear.supported(lin, torch.empty((65535, 64), dtype=BF, device=DEV))
    assert not hip_train_linear.supported(lin, torch.empty((65536, 64), dtype=BF, device=DEV))
    assert all(s.calls == 0 for s in spy.values())


def test_under_bf16_autocast_a_small_stack_takes_the_step(monkeypatch):
    """LayerNorm -> Linear -> QuantLinear under torch.autocast('cuda', torch.bfloat16): the quantized layer is handed bf16 (the
    Linear's output) and takes the 16-bit step, forward and backward; every parameter gets a finite fp32 gradient; with the
    switch off the same stack takes the torch formulation.  (In the order Linear -> LayerNorm -> QuantLinear autocast hands the
    layer fp32 -- layer_norm is one of the ops it runs in fp32 --, which the 16-bit switch leaves to the torch formulation.)"""
    from quant.binary.binary_linear import QuantLinear
    hip = _hip()
    dgrad, quant = _Spy(hip.linear_signw_dgrad_half), _Spy(hip.act_quant_half)
    monkeypatch.setattr(hip, 'linear_signw_dgrad_half', dgrad)
    monkeypatch.setattr(hip, 'act_quant_half', quant)
    seen = {}

    def build(half, norm_first=True):
        torch.manual_seed(5)
        q = QuantLinear('ls-2', 'ls-1', 64, 24, {'kind': 'symmetric', 'alpha': 2})
        q.hip_train_half = half
        q.register_forward_hook(lambda m, i, o: seen.update(x=i[0].dtype, y=o.dtype, fn=type(o.grad_fn).__name__))
        front = [torch.nn.LayerNorm(32), torch.nn.Linear(32, 64)] if norm_first else [torch.nn.Linear(32, 64), torch.nn.LayerNorm(64)]
        return torch.nn.Sequential(*front, q).to(DEV).train()
    x = detgen.normal('lthalf.stack.x', (6, 5, 32)).to(DEV)
    for half in (True, False):
        net = build(half)
        with torch.autocast('cuda', BF):
            y = net(x)
        assert seen['x'] == BF and y.dtype == BF
        assert (seen['fn'] == STEP_HALF) == half
        y.float().square().mean().backward()
        grads = [p.grad for p in net.parameters()]
        assert all(g is not None and g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in grads)
        assert float(net[1].weight.grad.abs().max()) > 0
    assert (dgrad.calls, quant.calls) == (1, 1)
    net = build(True, norm_first=False)
    with torch.autocast('cuda', BF):
        y = net(x)
    assert seen['x'] == torch.float32 and seen['fn'] not in (STEP, STEP_HALF)
    y.float().square().mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert (dgrad.calls, quant.calls) == (1, 1)
