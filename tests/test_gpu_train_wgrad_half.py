"""lsq_train_wgrad_half on the GPU (liblsq_hip_train_half.so) and ``hip_train.WGRAD_HALF_KERNEL``: the 16-bit weight and bias
gradient against the fp64 closed form on every case of tests/golden/train_wgrad_half_cases.py in both types, exact anchors on
integer operands, the fold per sample, determinism, what a call may write, refusals, and QuantConv2d's 16-bit train step."""

import ctypes

import pytest
import torch

import conv_train_half_cases as H
import detgen
import train_wgrad_half_cases as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BOUND_GB = 1e-5       # the step's grad_b, of max |gb64| (tests/test_gpu_conv_train_half.py)
SENTINEL = -7.25
PAD = 64
STEP_HALF = '_QuantConv2dStepHalfBackward'


def _hip():
    from quant import _hip
    return _hip


def _geom(c):
    return _hip().make_geom(c.N, c.C, c.H, c.W, c.O, c.k[0], c.k[1], (c.stride, c.stride), c.pad, (1, 1), 1)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _common_gy(tag, shape, scale):
    """A gradient whose values are exact in bf16 AND fp16 (bf16 values, the few below 2^-10 set to 0), so that both types share
    one fp64 reference."""
    gy = (detgen.normal(tag, shape) * scale).to(torch.bfloat16).float()
    gy[gy.abs() < 2.0 ** -10] = 0.0
    assert torch.equal(gy.to(torch.float16).float(), gy) and torch.equal(gy.to(torch.bfloat16).float(), gy)
    return gy


_REFS = {}


def _reference(c):
    """Planes and scales from lsq_act_quant, the common gradient and the fp64 closed form of a case: computed once, left unchanged."""
    if c.id not in _REFS:
        hip = _hip()
        geom = _geom(c)
        code, k = T.SCHEMES[c.scheme]
        x = detgen.normal(f'twh.x.{c.id}', (c.N, c.C, c.H, c.W), scale=1.3)
        planes = torch.zeros((k * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
        scales = torch.empty((k, c.N), dtype=torch.float32, device=DEV)
        hip.act_quant(x.to(DEV), geom, code, k, 3, 2.0, planes, scales)
        torch.cuda.synchronize()
        gy = _common_gy(f'twh.gy.{c.id}', (c.N, c.O) + T.out_hw(c), 0.25)
        ref = T.closed_form(c, T.xq64(T.unpack_planes(planes, k, c), scales), gy)
        _REFS[c.id] = dict(geom=geom, k=k, planes=planes, scales=scales, gy=gy, **ref)
    return _REFS[c.id]


def _hold(g, gb, ref, what):
    """The bound of the fp32 kernel, per element, and an exact 0 wherever the bound is 0."""
    err = (g.cpu().double() - ref['g']).abs()
    errb = (gb.cpu().double() - ref['gb']).abs()
    ratio = float((err / (T.BOUND * ref['mag'] + 1e-30)).max())
    ratiob = float((errb / (T.BOUND * ref['magb'] + 1e-30)).max())
    print(f'\ntrain-wgrad-half {what}: grad_wq {ratio:.4f} grad_b {ratiob:.4f} of the bound')
    assert bool((err <= T.BOUND * ref['mag'] + 1e-30).all()), (what, 'grad_wq', ratio)
    assert bool((errb <= T.BOUND * ref['magb'] + 1e-30).all()), (what, 'grad_b', ratiob)
    zero = ref['mag'] == 0
    assert bool((g.cpu()[zero] == 0).all()), (what, 'exact zeros')
    return ratio, ratiob


# ------------------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize('pair', T.PAIRS, ids=T.pair_id)
def test_equals_the_fp64_closed_form(pair):
    c, dtype = pair
    hip = _hip()
    ref = _reference(c)
    g, gb = hip.wgrad_half(ref['planes'], ref['k'], ref['scales'], ref['gy'].to(dtype).to(DEV), ref['geom'], bias=True)
    torch.cuda.synchronize()
    assert g.dtype == gb.dtype == torch.float32 and tuple(g.shape) == (c.O, c.C) + c.k and tuple(gb.shape) == (c.O,)
    _hold(g, gb, ref, T.pair_id(pair))
    g2, none = hip.wgrad_half(ref['planes'], ref['k'], ref['scales'], ref['gy'].to(dtype).to(DEV), ref['geom'])
    assert none is None and _bits_equal(g2, g)


# ---------------------------------------------------------------------------------------------------- 2. exact anchors
def _anchor(c):
    """Integer operands: gy = m / 8 with m in [-8, 8], scales powers of two that differ per sample and plane, random bits."""
    k = T.kx_of(c)
    gen = torch.Generator().manual_seed(len(c.id) + 17 * c.C + c.O)
    bits = torch.randint(0, 2, (k, c.N, c.C, c.H, c.W), generator=gen)
    gy = torch.randint(-8, 9, (c.N, c.O) + T.out_hw(c), generator=gen).float() / 8
    scales = torch.tensor([[2.0 ** -((n + 2 * p) % 5) for n in range(c.N)] for p in range(k)])
    assert k <= 3 and all(len({float(scales[p, n]) for p in range(k)}) == k for n in range(c.N))
    return bits, gy, scales


@pytest.mark.parametrize('c', T.ANCHORS, ids=lambda c: c.id)
@pytest.mark.parametrize('dtype', T.DTYPES, ids=lambda t: T.DTYPE_NAMES[t])
def test_integer_operands_give_the_closed_form_exactly(c, dtype):
    hip = _hip()
    bits, gy, scales = _anchor(c)
    ref = T.closed_form(c, T.xq64(bits, scales), gy)
    # every partial sum is an integer of the unit 2^-3 2^-4 below 2^24: fp32 holds each of them exactly
    assert float(ref['mag'].max()) * 128 < 2 ** 24 and float(ref['magb'].max()) * 8 < 2 ** 24
    assert torch.equal(gy.to(dtype).float(), gy)
    g, gb = hip.wgrad_half(T.pack_planes(bits, c.pad).to(DEV), scales.shape[0], scales.to(DEV), gy.to(dtype).to(DEV), _geom(c),
                           bias=True)
    torch.cuda.synchronize()
    assert torch.equal(g.cpu().double(), ref['g']), int((g.cpu().double() != ref['g']).sum())
    assert torch.equal(gb.cpu().double(), ref['gb'])


# -------------------------------------------------------------------------------------------------- 3. the fold per sample
@pytest.mark.parametrize('dtype', T.DTYPES, ids=lambda t: T.DTYPE_NAMES[t])
def test_equal_scales_fold_for_that_sample_alone(dtype):
    """kx = 2; samples 0 and 2 have v_0 = v_1 (a folded pair: opposite bits are an exact 0), sample 1 has not.  Channels 0..7 carry
    opposite bits everywhere; out-channels 0..3 get no gradient from sample 1 -- there the closed form is 0 and so must the
    result be, while v t_0 - v t_1 summed plane by plane leaves the rounding of its first term."""
    hip = _hip()
    c = T.Case('fold', 70, 40, 3, 9, 9, (3, 3), 1, (1, 1), 'ls-T')
    gen = torch.Generator().manual_seed(11)
    bits = torch.randint(0, 2, (2, c.N, c.C, c.H, c.W), generator=gen)
    bits[1, :, :8] = 1 - bits[0, :, :8]
    gy = _common_gy('twh.fold.gy', (c.N, c.O) + T.out_hw(c), 0.7)
    gy[1, :4] = 0.0
    scales = torch.tensor([[0.8125, 0.59375, 1.21875], [0.8125, 0.3125, 1.21875]])
    ref = T.closed_form(c, T.xq64(bits, scales), gy)
    zero = ref['mag'] == 0
    assert bool(zero[:4, :8].all()) and int(zero.sum()) == 4 * 8 * 9 and float(ref['mag'][4:, :8].min()) > 0
    g, gb = hip.wgrad_half(T.pack_planes(bits, c.pad).to(DEV), 2, scales.to(DEV), gy.to(dtype).to(DEV), _geom(c), bias=True)
    torch.cuda.synchronize()
    _hold(g, gb, ref, f'fold-{T.DTYPE_NAMES[dtype]}')
    assert bool((g.cpu()[:4, :8] == 0).all())


# ----------------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize('dtype', T.DTYPES, ids=lambda t: T.DTYPE_NAMES[t])
@pytest.mark.parametrize('cid', ['padded_7x7', 'tail_9x9'])
def test_bitwise_the_same_across_calls_streams_and_addresses(cid, dtype):
    hip = _hip()
    c = T.BY_ID[cid]
    ref = _reference(c)
    assert T.plan(c).S > 1                                # the K split and its reduction are exercised
    gy = ref['gy'].to(dtype).to(DEV)
    args = (ref['planes'], ref['k'], ref['scales'])
    g1, b1 = hip.wgrad_half(*args, gy, ref['geom'], bias=True)
    g2, b2 = hip.wgrad_half(*args, gy, ref['geom'], bias=True)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        g3, b3 = hip.wgrad_half(*args, gy, ref['geom'], bias=True)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert _bits_equal(g1, g2) and _bits_equal(g1, g3) and _bits_equal(b1, b2) and _bits_equal(b1, b3)
    for offset in (0, 2, 6):                              # 16-byte loads at 0, element loads at 2 and 6: the same bits
        buf, view = T.at_byte_offset(gy, offset)
        assert view.data_ptr() % 16 == offset and view.is_contiguous()
        g4, b4 = hip.wgrad_half(*args, view, ref['geom'], bias=True)
        torch.cuda.synchronize()
        assert _bits_equal(g1, g4) and _bits_equal(b1, b4), offset
        assert torch.equal(view, gy)


# ---------------------------------------------------------------------------------------------- 5. nothing else written
def _raw(hip, c, ref, dtype, gy, gw_ptr, gb_ptr, ws_ptr, ws_bytes, kx=None, dt=None):
    return hip.train_half_lib().lsq_train_wgrad_half(
        ref['planes'].data_ptr(), ref['k'] if kx is None else kx, ref['scales'].data_ptr(), gy.data_ptr(),
        T.DTYPE_CODES[dtype] if dt is None else dt, ctypes.byref(ref['geom']), gw_ptr, gb_ptr, ws_ptr, ws_bytes, hip.stream_ptr(DEV))


@pytest.mark.parametrize('dtype', T.DTYPES, ids=lambda t: T.DTYPE_NAMES[t])
@pytest.mark.parametrize('cid', ['one_chunk', 'tail_9x9'])
def test_a_call_writes_its_outputs_and_nothing_else(cid, dtype):
    """Through the C ABI: grad_wq and grad_b between sentinels, a workspace of exactly the stated size between sentinels and
    poisoned with NaNs; without grad_b the smaller workspace, and no trace of a bias gradient anywhere."""
    hip = _hip()
    c = T.BY_ID[cid]
    ref = _reference(c)
    gy = ref['gy'].to(dtype).to(DEV)
    want_g, want_b = hip.wgrad_half(ref['planes'], ref['k'], ref['scales'], gy, ref['geom'], bias=True)
    n = want_g.numel()
    for with_bias in (True, False):
        need = T.workspace_bytes(c, with_bias)
        assert need == hip.train_half_lib().lsq_train_wgrad_half_workspace_bytes(ctypes.byref(ref['geom']), ref['k'], int(with_bias))
        for poison in (float('nan'), 3.0e38):
            gw = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
            gb = torch.full((c.O + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
            ws = torch.full((need // 4 + 2 * PAD,), poison, dtype=torch.float32, device=DEV)
            assert (ws.data_ptr() + 4 * PAD) % 16 == 0
            code = _raw(hip, c, ref, dtype, gy, gw.data_ptr() + 4 * PAD, gb.data_ptr() + 4 * PAD if with_bias else None,
                        ws.data_ptr() + 4 * PAD if need else None, need)
            assert code == 0
            torch.cuda.synchronize()
            assert _bits_equal(gw[PAD:PAD + n].view_as(want_g), want_g)
            assert bool((gw[:PAD] == SENTINEL).all()) and bool((gw[PAD + n:] == SENTINEL).all())
            if with_bias:
                assert _bits_equal(gb[PAD:PAD + c.O], want_b)
                assert bool((gb[:PAD] == SENTINEL).all()) and bool((gb[PAD + c.O:] == SENTINEL).all())
            else:
                assert bool((gb == SENTINEL).all())
            edge = torch.cat([ws[:PAD], ws[PAD + need // 4:]])
            assert bool(torch.isnan(edge).all()) if poison != poison else bool((edge == poison).all())


# ------------------------------------------------------------------------------------------------ 6. refusals on the device
def test_refused_calls_write_nothing_on_the_device():
    hip = _hip()
    c = T.BY_ID['tail_9x9']
    ref = _reference(c)
    need = T.workspace_bytes(c, True)
    gy = ref['gy'].to(torch.bfloat16).to(DEV)
    gw = torch.full((c.O * c.C * 9,), SENTINEL, dtype=torch.float32, device=DEV)
    gb = torch.full((c.O,), SENTINEL, dtype=torch.float32, device=DEV)
    ws = torch.full((need // 4 + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    call = lambda **kw: _raw(hip, c, ref, torch.bfloat16, kw.pop('gy', gy), kw.pop('gw', gw.data_ptr()), kw.pop('gb', gb.data_ptr()),
                             kw.pop('ws', ws.data_ptr()), kw.pop('bytes', need), **kw)
    assert call(dt=0) == -6 and call(dt=3) == -6                                  # LSQ_E_UNSUPPORTED: another dtype
    assert call(gw=gw.data_ptr() + 2) == -6 and call(gb=gb.data_ptr() + 2) == -6  # outputs not aligned to 4 bytes
    assert call(kx=0) == -3 and call(kx=9) == -3                                  # LSQ_E_SCHEME
    assert call(ws=None) == -1                                                    # LSQ_E_NULL: a workspace is needed
    assert call(bytes=need - 4) == -5 and call(ws=ws.data_ptr() + 4) == -5        # LSQ_E_WORKSPACE
    assert call(gw=None) == -1
    torch.cuda.synchronize()
    assert bool((gw == SENTINEL).all()) and bool((gb == SENTINEL).all()) and bool((ws == SENTINEL).all())
    with pytest.raises(hip.LsqHipError):
        bad = hip.make_geom(c.N, c.C, c.H, c.W, c.O, 3, 3, (1, 1), (1, 1), (2, 1), 1)      # dilation: LSQ_E_UNSUPPORTED
        gy_bad = torch.zeros((c.N, c.O, 7, 9), dtype=torch.bfloat16, device=DEV)
        hip.wgrad_half(ref['planes'], ref['k'], ref['scales'], gy_bad, bad)


# ------------------------------------------------------------------------------------------------------------ 7. the step
class _Spy:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self.fn(*a, **k)


def _wgrad_geometry(c):
    return (c.groups == 1 and (c.dil_h, c.dil_w) == (1, 1) and c.stride_h == c.stride_w and c.stride_h in (1, 2)
            and c.pad_h <= c.KH - 1 and c.pad_w <= c.KW - 1 and max(c.KH, c.KW) <= 8)


STEP_CASES = [c for c in H.CASES if c.xs != 'fp' and _wgrad_geometry(c)]
STEP_PAIRS = [(c, t) for c in STEP_CASES for t in H.DTYPES]
NAMES = ('wgrad_half', 'wgrad', 'quant_values', 'signw_conv2d_dgrad_half', 'act_quant_half', 'ste_backward')


def _module(case):
    conv = H.make_module(case)
    conv.hip_train_half = True
    return conv.to(DEV).train()


def _run_step(monkeypatch, case, dtype, switch):
    """One forward + backward of the case's module with ``WGRAD_HALF_KERNEL = switch``: the results and the calls."""
    from quant.binary import hip_train
    hip = _hip()
    d = H.inputs(case.id, dtype)
    with monkeypatch.context() as m:
        m.setattr(hip_train, 'WGRAD_HALF_KERNEL', switch)
        spy = {n: _Spy(getattr(hip, n)) for n in NAMES}
        for n, s in spy.items():
            m.setattr(hip, n, s)
        miopen = _Spy(torch.nn.grad.conv2d_weight)
        m.setattr(torch.nn.grad, 'conv2d_weight', miopen)
        conv = _module(case)
        x = d['x'].to(DEV).requires_grad_()
        y = conv(x)
        assert type(y.grad_fn).__name__ == STEP_HALF
        kept = y.grad_fn.saved_tensors[4].numel()
        y.backward(d['gy'].to(DEV))
        torch.cuda.synchronize()
    calls = {n: s.calls for n, s in spy.items()}
    calls['conv2d_weight'] = miopen.calls
    return conv, x, y.detach(), calls, kept


def test_the_step_cases_are_the_binary_ones_the_kernel_states():
    assert len(STEP_CASES) >= 8 and H.BY_ID['s2_3x5'] in STEP_CASES and H.BY_ID['odd_planes'] in STEP_CASES
    assert all(c.xs != 'fp' for c in STEP_CASES) and any(c.bias for c in STEP_CASES) and any(not c.bias for c in STEP_CASES)


@pytest.mark.parametrize('pair', STEP_PAIRS, ids=H.pair_id)
def test_train_step_with_the_16_bit_weight_gradient(monkeypatch, pair):
    case, dtype = pair
    conv, x, y, calls, kept = _run_step(monkeypatch, case, dtype, True)
    assert kept > 0
    assert calls == dict(wgrad_half=1, wgrad=0, quant_values=0, signw_conv2d_dgrad_half=1, act_quant_half=1, ste_backward=1,
                         conv2d_weight=0), calls
    assert conv.weight.grad.dtype == torch.float32 and (conv.bias is None or conv.bias.grad.dtype == torch.float32)
    ref = H.step64(case, dtype, list(conv.last_act_scales.detach().cpu()),
                   list(conv.w_approximate.plane_scales().detach().float().cpu()))
    err_w = (conv.weight.grad.cpu().double() - ref['gw']).abs()
    bound_w = 2e-6 * ref['m_w'].abs() * ref['mag_w'] + 1e-30
    print(f'\ntrain-wgrad-half step {H.pair_id(pair)}: grad_w {float((err_w / bound_w).max()):.4f} of the bound')
    assert bool((err_w <= bound_w).all()), float((err_w / bound_w).max())
    if case.bias:
        err_b = (conv.bias.grad.cpu().double() - ref['gb']).abs()
        assert float(err_b.max()) <= BOUND_GB * float(ref['gb'].abs().max())
    # the forward and the input gradient are those of the switch-off step, bit for bit
    conv0, x0, y0, calls0, kept0 = _run_step(monkeypatch, case, dtype, False)
    assert kept0 == 0 and calls0['wgrad_half'] == 0
    assert torch.equal(y.view(torch.int16), y0.view(torch.int16)) and torch.equal(x.grad.view(torch.int16), x0.grad.view(torch.int16))


def test_with_the_switch_off_the_calls_and_bits_are_todays(monkeypatch):
    """Off: gy.float(), lsq_quant_values and conv2d_weight as before, also under WGRAD_KERNEL (lsq_train_wgrad on gy.float())."""
    from quant.binary import hip_train
    case, dtype = H.BY_ID['s2_3x5'], torch.bfloat16
    conv, x, y, calls, kept = _run_step(monkeypatch, case, dtype, False)
    assert kept == 0 and calls == dict(wgrad_half=0, wgrad=0, quant_values=1, signw_conv2d_dgrad_half=1, act_quant_half=1,
                                       ste_backward=1, conv2d_weight=1), calls
    again = _run_step(monkeypatch, case, dtype, False)
    assert torch.equal(conv.weight.grad, again[0].weight.grad) and torch.equal(conv.bias.grad, again[0].bias.grad)
    monkeypatch.setattr(hip_train, 'WGRAD_KERNEL', True)
    conv1, x1, y1, calls1, kept1 = _run_step(monkeypatch, case, dtype, False)
    assert kept1 > 0 and calls1['wgrad'] == 1 and calls1['wgrad_half'] == 0 and calls1['conv2d_weight'] == 0
    both = _run_step(monkeypatch, case, dtype, True)             # both switches: the 16-bit kernel takes the step
    assert both[3]['wgrad_half'] == 1 and both[3]['wgrad'] == 0


def test_fp_activations_and_a_refused_geometry_take_todays_route(monkeypatch):
    fp = next(c for c in H.CASES if c.xs == 'fp' and c.groups == 1)
    refused = H.BY_ID['s3_3x3']                                   # stride 3: outside lsq_train_wgrad's geometry
    assert refused.xs != 'fp' and not _wgrad_geometry(refused)
    for case in (fp, refused):
        conv, x, y, calls, kept = _run_step(monkeypatch, case, torch.bfloat16, True)
        assert kept == 0 and calls['wgrad_half'] == 0 and calls['conv2d_weight'] == 1, (case.id, calls)
        off = _run_step(monkeypatch, case, torch.bfloat16, False)
        assert torch.equal(conv.weight.grad, off[0].weight.grad)


def test_a_frozen_weight_keeps_no_planes_and_the_bias_takes_todays_sum(monkeypatch):
    from quant.binary import hip_train
    hip = _hip()
    monkeypatch.setattr(hip_train, 'WGRAD_HALF_KERNEL', True)
    case = H.BY_ID['s2_3x5']
    d = H.inputs(case.id, torch.bfloat16)
    spy = _Spy(hip.wgrad_half)
    monkeypatch.setattr(hip, 'wgrad_half', spy)
    conv = _module(case)
    conv.weight.requires_grad_(False)
    y = conv(d['x'].to(DEV).requires_grad_())
    assert y.grad_fn.saved_tensors[4].numel() == 0
    y.backward(d['gy'].to(DEV))
    assert spy.calls == 0 and conv.weight.grad is None
    assert torch.equal(conv.bias.grad, d['gy'].to(DEV).float().sum(dim=(0, 2, 3)))


def test_two_forwards_before_one_backward_read_their_own_planes(monkeypatch):
    from quant.binary import hip_train
    monkeypatch.setattr(hip_train, 'WGRAD_HALF_KERNEL', True)
    case, dtype = H.BY_ID['s2_3x5'], torch.bfloat16
    d = H.inputs(case.id, dtype)
    x2_cpu = detgen.normal('twh.two.x2', d['x'].shape, scale=0.6).to(dtype)
    g1, g2 = d['gy'].to(DEV), detgen.normal('twh.two.g2', d['gy'].shape).to(dtype).to(DEV)
    singles = []
    for xc, g in ((d['x'], g1), (x2_cpu, g2)):
        conv = _module(case)
        conv(xc.to(DEV)).backward(g)
        singles.append((conv.weight.grad.clone(), conv.bias.grad.clone()))
    conv = _module(case)
    ya, yb = conv(d['x'].to(DEV)), conv(x2_cpu.to(DEV))
    pa, pb = ya.grad_fn.saved_tensors[4], yb.grad_fn.saved_tensors[4]
    assert pa.numel() > 0 and pa.data_ptr() != pb.data_ptr() and not torch.equal(pa, pb)
    torch.autograd.backward([ya, yb], [g1, g2])
    assert torch.equal(conv.weight.grad, singles[0][0] + singles[1][0])
    assert torch.equal(conv.bias.grad, singles[0][1] + singles[1][1])
