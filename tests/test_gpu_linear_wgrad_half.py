"""lsq_linear_signx_wgrad_half on the GPU (liblsq_hip_linear_wgrad_half.so) and QuantLinear's 16-bit train step with
``WGRAD_HALF_KERNEL``: (a) the kernel's two contracts bit for bit against the composition of the existing kernels on
``gy.float()`` / ``x.float()``, on every case of tests/golden/linear_wgrad_half_cases.py in both types, and independently against
the fp64 references; the output buffer, operands shifted by one element, determinism, refused calls that write nothing; (b) the
step against the fp64 step of tests/golden/linear_train_half_cases.py and against the same step with the switch off; (c) what is
launched and what is not; LeNet's fc1 under bf16 autocast in the training loop.

Bounds.  (A) and (B) are held to BOUND = 1e-5 of max |ref| (tests/test_linear_wgrad_half_host.py keeps the bf16 hi + lo split
alone within half of it at every case); the step's grad_w and grad_b to the 1e-5 of max |.64| tests/test_gpu_linear_train_half.py
holds them to on the fp32 routes."""

import pytest
import torch

import linear_train_half_cases as L
import linear_wgrad_cases as C
import linear_wgrad_half_cases as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BOUND = H.BOUND
STEP_BOUND = 1e-5     # of max |.64|: tests/test_gpu_linear_train_half.py's figure for grad_w and grad_b
STEP_HALF = '_QuantLinearStepHalfBackward'
E_UNSUPPORTED = -6
DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
BF = torch.bfloat16
PAD = 37              # floats of guard on each side of an output written through the C ABI
PER_CLASS = ('lenet_fc1', 'tiles64_vec', 'tiles128')          # one case of each kernel class with O % 4 == 0


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
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


_OPS, _REFS = {}, {}


def _ops(case, dtype):
    """The (case, type)'s operands on the device, made once and never written."""
    key = (case.id, dtype)
    if key not in _OPS:
        d = H.inputs(case.id, dtype)
        _OPS[key] = {k: d[k].to(DEV) for k in ('gy', 'x', 'xs', 'w', 'ws')}
    return _OPS[key]


def _refs(case, dtype):
    """(ref_a, ref_b) in fp64 on the CPU, computed once per (case, type) and left unchanged."""
    key = (case.id, dtype)
    if key not in _REFS:
        d = H.inputs(case.id, dtype)
        a = H.ref_a(case, d, DEV)
        _REFS[key] = (a, H.ref_b(d, a))
    return _REFS[key]


def _half(case, t, weight=True, gy=None, x=None):
    return _hip().linear_signx_wgrad_half(t['gy'] if gy is None else gy, t['x'] if x is None else x, t['xs'], H.ALPHA, case.N,
                                          case.T, case.F, case.O, *((t['w'], t['ws']) if weight else ()))


def _of_max(got, ref):
    return float((got.cpu().double() - ref).abs().max()) / float(ref.abs().max())


# ------------------------------------------------------------------------------------------------- (a) the kernel alone
@pytest.mark.parametrize('pair', H.PAIRS, ids=H.pair_id)
def test_contracts_hold_bit_for_bit_and_against_fp64(pair):
    """(A) w = NULL: lsq_linear_signx_wgrad(gy.float(), x.float()); (B) w given: lsq_ste_backward(w, (A), wscales, -1).  Then,
    independently of those kernels, both within BOUND of max |ref| of the fp64 references."""
    case, dtype = pair
    hip, t = _hip(), _ops(case, dtype)
    a_ref = hip.linear_signx_wgrad(t['gy'].float(), t['x'].float(), t['xs'], H.ALPHA, case.N, case.T, case.F, case.O)
    b_ref = hip.ste_backward(t['w'], a_ref, t['ws'], -1.0)
    got_a, got_b = _half(case, t, weight=False), _half(case, t)
    assert tuple(got_a.shape) == tuple(got_b.shape) == (case.O, case.F)
    assert _same_bits(got_a, a_ref), 'A'
    assert _same_bits(got_b, b_ref), 'B'
    ref_a, ref_b = _refs(case, dtype)
    ea, eb = _of_max(got_a, ref_a), _of_max(got_b, ref_b)
    print(f'\nlinear-wgrad-half {H.pair_id(pair)}: A err/max = {ea:.3e}  B err/max = {eb:.3e}')
    assert ea <= BOUND, (H.pair_id(pair), 'A', ea)
    assert eb <= BOUND, (H.pair_id(pair), 'B', eb)


@pytest.mark.parametrize('cid', ['ragged', 'rows_per_sample', 'eight_planes'])
def test_one_flipped_sign_is_far_outside_the_bound(cid):
    """What ONE wrong sign bit of the image would cost the reference: more than 100 bounds, so the check above can see it."""
    case = H.BY_ID[cid]
    d = H.inputs(cid, BF)
    c = H.as_fp32_case(case, d)
    ref, _ = _refs(case, BF)
    flipped = [b.clone() for b in c['signs']]
    flipped[-1][0, 0] = -flipped[-1][0, 0]
    wrong = C.reference64(dict(c, signs=flipped))
    assert float((wrong - ref).abs().max()) > 100 * BOUND * float(ref.abs().max())


def _raw(case, t, dtype, out_ptr, gy_ptr=None, x_ptr=None, weight=True, dtype_code=None, kx=None, kw=None):
    hip = _hip()
    lib = hip.linear_wgrad_half_lib()
    k = t['xs'].shape[0]
    need = int(lib.lsq_linear_signx_wgrad_half_workspace_bytes(k, case.N, case.T, case.F, case.O))
    assert need > 0
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    code = lib.lsq_linear_signx_wgrad_half(
        t['gy'].data_ptr() if gy_ptr is None else gy_ptr, t['x'].data_ptr() if x_ptr is None else x_ptr,
        DT[dtype] if dtype_code is None else dtype_code, k if kx is None else kx, t['xs'].data_ptr(), H.ALPHA, case.N, case.T,
        case.F, case.O, t['w'].data_ptr() if weight else None, (t['ws'].shape[0] if kw is None else kw) if weight else 0,
        t['ws'].data_ptr() if weight else None, out_ptr, ws.data_ptr(), need, hip.stream_ptr(DEV))
    torch.cuda.synchronize()
    return code


@pytest.mark.parametrize('dtype', L.DTYPES, ids=lambda d: L.DTYPE_NAMES[d])
@pytest.mark.parametrize('cid', PER_CLASS + ('odd_rows', 'tiles64_ragged'))
def test_output_buffer_and_operands_shifted_by_one_element(cid, dtype):
    """out written exactly into its place inside a NaN-filled buffer, 37 floats of guard on each side left NaN; gy, and x, at
    an address 2 bytes past a 16-byte boundary give the same bits as the aligned call.  With O % 4 == 0 that compares the
    8-byte and the 2-byte gradient loads of the tiled kernels."""
    case = H.BY_ID[cid]
    t = _ops(case, dtype)
    cnt = case.O * case.F
    for weight in (False, True):
        want = _half(case, t, weight)
        buf = torch.full((PAD + cnt + PAD,), float('nan'), device=DEV)
        assert _raw(case, t, dtype, buf.data_ptr() + 4 * PAD, weight=weight) == 0
        assert bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + cnt:]).all())
        out = buf[PAD:PAD + cnt].view(case.O, case.F)
        assert not bool(torch.isnan(out).any())
        assert _same_bits(out, want), weight
        (gy_buf, gy_v), (x_buf, x_v) = L.shifted(t['gy']), L.shifted(t['x'])
        assert gy_v.data_ptr() % 16 == 2 and x_v.data_ptr() % 16 == 2
        assert _same_bits(_half(case, t, weight, gy=gy_v), want), ('gy', weight)
        assert _same_bits(_half(case, t, weight, x=x_v), want), ('x', weight)
        assert _same_bits(_half(case, t, weight, gy=gy_v, x=x_v), want), ('gy, x', weight)


@pytest.mark.parametrize('cid', PER_CLASS)
def test_two_calls_and_a_side_stream_give_the_same_bits(cid):
    case = H.BY_ID[cid]
    t = _ops(case, BF)
    g1, g2 = _half(case, t), _half(case, t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g3 = _half(case, t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _same_bits(g1, g2) and _same_bits(g1, g3)


def test_refused_calls_return_the_code_and_write_nothing():
    case = H.BY_ID['eight_planes']
    t = _ops(case, BF)
    out = torch.full((case.O * case.F + 1,), 12345.0, device=DEV)
    gy_buf, gy_v = L.shifted(t['gy'])
    refusals = [dict(dtype_code=0), dict(kx=0), dict(kx=9), dict(kw=0), dict(kw=9),
                dict(gy_ptr=gy_v.data_ptr() + 1), dict(out_ptr=out.data_ptr() + 2)]
    for kw in refusals:
        ptr = kw.pop('out_ptr', out.data_ptr())
        assert _raw(case, t, BF, ptr, **kw) == E_UNSUPPORTED, kw
        assert bool((out == 12345.0).all()), kw
    assert _raw(case, t, BF, out.data_ptr()) == 0 and not bool((out[:-1] == 12345.0).any()) and float(out[-1]) == 12345.0


# ------------------------------------------------------------------------------------------ (b) the step, switch on
BINARY = [p for p in L.PAIRS if p[0].xs != 'fp']


def _module(case, half=True):
    lin = L.make_module(case)
    lin.hip_train_half = half
    return lin.to(DEV).train()


def _step(lin, x, gy):
    x = x.to(DEV).requires_grad_()
    y = lin(x)
    y.backward(gy.to(DEV))
    return x, y


@pytest.fixture
def HTL():
    from quant.binary import hip_train_linear
    return hip_train_linear


@pytest.mark.parametrize('pair', BINARY, ids=L.pair_id)
def test_train_step_with_the_kernel(pair, monkeypatch, HTL):
    """grad_w and grad_b within 1e-5 of max |.64| of step64; y and grad_x bit-equal to the same step with the switch off; the
    cached weight-scale buffers equal."""
    case, dtype = pair
    d = L.inputs(case.id, dtype)
    out = {}
    for on in (True, False):
        monkeypatch.setattr(HTL, 'WGRAD_HALF_KERNEL', on)
        lin = _module(case)
        x, y = _step(lin, d['x'], d['gy'])
        assert type(y.grad_fn).__name__ == STEP_HALF
        out[on] = (lin, x, y)
    lin, x, y = out[True]
    off, x0, y0 = out[False]
    assert y.dtype == dtype and torch.equal(y.view(torch.int16), y0.view(torch.int16))
    assert x.grad.dtype == dtype and torch.equal(x.grad.view(torch.int16), x0.grad.view(torch.int16))
    for (n1, b1), (n2, b2) in zip(lin.w_approximate.named_buffers(), off.w_approximate.named_buffers()):
        assert n1 == n2 and torch.equal(b1, b2), n1
    assert lin.weight.grad.dtype == torch.float32 and tuple(lin.weight.grad.shape) == (case.O, case.F)
    ref = L.step64(case, dtype, list(lin.last_act_scales.detach().cpu()),
                   list(lin.w_approximate.plane_scales().detach().float().cpu()))
    ew = _of_max(lin.weight.grad, ref['gw'])
    e0 = _of_max(off.weight.grad, ref['gw'])
    print(f'\nlinear-wgrad-half step {L.pair_id(pair)}: gw err/max = {ew:.3e} (switch off {e0:.3e})', end='')
    if case.bias:
        assert lin.bias.grad.dtype == torch.float32
        eb = _of_max(lin.bias.grad, ref['gb'])
        print(f'  gb err/max = {eb:.3e}', end='')
        assert eb <= STEP_BOUND, (L.pair_id(pair), 'gb', eb)
    else:
        assert lin.bias is None
    assert ew <= STEP_BOUND, (L.pair_id(pair), 'gw', ew)


# ------------------------------------------------------------------------------------------------------ (c) plumbing
PLUMB = L.BY_ID['rows_per_sample']          # [3, 5, 64] -> 130, ls-1 activations, gf-8 weights
NAMES = ('linear_signx_wgrad_half', 'linear_signx_wgrad', 'quant_values', 'ste_backward', 'linear_signw_dgrad_half')


@pytest.fixture
def spies(monkeypatch):
    hip = _hip()
    spy = {n: _Spy(getattr(hip, n)) for n in NAMES}
    for n, s in spy.items():
        monkeypatch.setattr(hip, n, s)
    return spy


def _calls(spy):
    return {n: s.calls for n, s in spy.items()}


@pytest.mark.parametrize('dtype', L.DTYPES, ids=lambda d: L.DTYPE_NAMES[d])
def test_what_the_step_launches(dtype, monkeypatch, HTL, spies):
    monkeypatch.setattr(HTL, 'WGRAD_HALF_KERNEL', True)
    d = L.inputs(PLUMB.id, dtype)
    lin = _module(PLUMB)
    _step(lin, d['x'], d['gy'])
    assert _calls(spies) == dict(linear_signx_wgrad_half=1, linear_signx_wgrad=0, quant_values=0, ste_backward=0,
                                 linear_signw_dgrad_half=1)
    gy, x = spies['linear_signx_wgrad_half'].args[:2]
    assert gy.dtype == dtype and x.dtype == dtype
    assert torch.equal(gy, d['gy'].to(DEV).view(-1, PLUMB.O)) and torch.equal(x, d['x'].to(DEV).view(-1, PLUMB.F))
    assert lin.weight.grad is not None and lin.bias.grad is not None
    for s in spies.values():
        s.calls = 0
    lin.weight.requires_grad_(False)                                  # a frozen weight: no call
    lin.bias.grad = None
    xg, _ = _step(lin, d['x'], d['gy'])
    assert _calls(spies) == dict(linear_signx_wgrad_half=0, linear_signx_wgrad=0, quant_values=0, ste_backward=0,
                                 linear_signw_dgrad_half=1)
    assert xg.grad is not None and lin.bias.grad is not None


def test_a_layer_without_bias(monkeypatch, HTL, spies):
    from quant.binary.binary_linear import QuantLinear
    monkeypatch.setattr(HTL, 'WGRAD_HALF_KERNEL', True)
    d = L.inputs(PLUMB.id, BF)
    res = []
    for bias in (True, False):
        lin = QuantLinear(PLUMB.xs, PLUMB.ws, PLUMB.F, PLUMB.O, dict(PLUMB.clamp), bias=bias)
        with torch.no_grad():
            lin.weight.copy_(d['w'])
        lin.hip_train_half = True
        lin = lin.to(DEV).train()
        x, y = _step(lin, d['x'], d['gy'])
        assert type(y.grad_fn).__name__ == STEP_HALF and (lin.bias is None) == (not bias)
        res.append((x.grad, lin.weight.grad))
    assert spies['linear_signx_wgrad_half'].calls == 2
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][0].view(torch.int16), res[1][0].view(torch.int16))


@pytest.mark.parametrize('flag', [True, False])
def test_fp_activations_keep_torch_mm(flag, monkeypatch, HTL, spies):
    monkeypatch.setattr(HTL, 'WGRAD_HALF_KERNEL', flag)
    case = L.BY_ID['one_product']
    assert case.xs == 'fp'
    d = L.inputs(case.id, BF)
    lin = _module(case)
    x, y = _step(lin, d['x'], d['gy'])
    assert type(y.grad_fn).__name__ == STEP_HALF
    assert spies['linear_signx_wgrad_half'].calls == 0 and spies['quant_values'].calls == 1 and spies['ste_backward'].calls == 1
    assert lin.weight.grad is not None


def test_with_the_switch_off_the_wrapper_is_never_called(HTL, spies):
    assert HTL.WGRAD_HALF_KERNEL is False
    d = L.inputs(PLUMB.id, BF)
    lin = _module(PLUMB)
    _step(lin, d['x'], d['gy'])
    assert spies['linear_signx_wgrad_half'].calls == 0 and spies['quant_values'].calls == 1 and spies['ste_backward'].calls == 1


def test_both_switches_on_the_half_kernel_runs(monkeypatch, HTL, spies):
    monkeypatch.setattr(HTL, 'WGRAD_KERNEL', True)
    monkeypatch.setattr(HTL, 'WGRAD_HALF_KERNEL', True)
    d = L.inputs(PLUMB.id, BF)
    lin = _module(PLUMB)
    _step(lin, d['x'], d['gy'])
    assert spies['linear_signx_wgrad_half'].calls == 1 and spies['linear_signx_wgrad'].calls == 0
    assert spies['quant_values'].calls == 0 and spies['ste_backward'].calls == 0


# ------------------------------------------------------------------------------------------------ the training loop
def test_lenet_fc1_trains_under_bf16_autocast_with_the_kernel(monkeypatch, HTL, spies):
    """quant.common.training.train on cuda:0 under torch.autocast('cuda', torch.bfloat16) with QLeNet5's fc1 a QuantLinear
    (ls-2 activations) on hip_train_half: with WGRAD_HALF_KERNEL every step's weight gradient comes from the new call (12 = 3
    epochs x 4 batches), the loss falls, and the first epoch agrees with the switch-off run from the same seed (rel 2e-2, as
    test_lenet_fc1_trains_with_the_kernel of tests/test_gpu_linear_wgrad.py)."""
    from quant.common.initialization import get_lr_scheduler, get_optimizer
    from quant.common.metrics import LossMetric
    from quant.common.training import train
    from quant.models.lenet import QLeNet5
    clamp = {'kind': 'symmetric', 'alpha': 3}
    fc1q = {'x_quant': 'ls-2', 'w_quant': 'ls-1', 'clamp': clamp}
    g = torch.Generator().manual_seed(5)
    data = torch.randn(64, 1, 28, 28, generator=g)
    target = torch.randint(0, 10, (64,), generator=g)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, target), batch_size=16)
    losses, calls = {}, {}
    for on in (True, False):
        monkeypatch.setattr(HTL, 'WGRAD_HALF_KERNEL', on)
        before = spies['linear_signx_wgrad_half'].calls
        torch.manual_seed(11)
        model = QLeNet5(loss_fn=torch.nn.functional.nll_loss, fc1_quant=fc1q).to(DEV)
        model.fc1.hip_train_half = True
        seen = {}
        model.fc1.register_forward_hook(lambda m, i, o: seen.update(x=i[0].dtype, fn=type(o.grad_fn).__name__))
        opt = get_optimizer(model.parameters(), {'algorithm': 'sgd', 'lr': 0.02, 'momentum': 0.9})
        sched = get_lr_scheduler(opt, {'scheduler': 'step_lr', 'step_size': 10, 'gamma': 0.5}, 3, len(loader))
        metrics = {'Loss': LossMetric(model.loss_fn, accumulate=True)}
        with torch.autocast('cuda', torch.bfloat16):
            losses[on] = [train(model, loader, metrics, opt, sched, torch.device(DEV), e, 100)['Loss'] for e in (1, 2, 3)]
        assert seen == dict(x=torch.bfloat16, fn=STEP_HALF), seen
        calls[on] = spies['linear_signx_wgrad_half'].calls - before
    print('losses', losses)
    assert calls == {True: 4 * 3, False: 0}                          # 4 batches x 3 epochs
    assert spies['linear_signx_wgrad'].calls == 0
    assert losses[True][2] < losses[True][0]
    assert losses[True][0] == pytest.approx(losses[False][0], rel=2e-2)
