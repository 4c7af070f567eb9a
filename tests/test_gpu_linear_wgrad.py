"""lsq_linear_signx_wgrad (liblsq_hip_linear_wgrad.so) and QuantLinear's train step with WGRAD_KERNEL on the GPU: the kernel
against fp64 for every activation depth and every kernel variant, rows per sample, the signs at the chain's edge values,
the output buffer and unaligned operands, determinism, refused calls that write nothing; the autograd step
(quant.binary.hip_train_linear) against the torch formulation on the device, what is launched and what is not, LeNet's fc1
in the training loop."""

import pytest
import torch

import detgen
import linear_wgrad_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BOUND = C.BOUND   # |gwq - gwq64| <= BOUND * max |gwq64|; tests/test_linear_wgrad_host.py keeps the split alone within half of it
SYM = {'kind': 'symmetric', 'alpha': 2}
E_UNSUPPORTED = -6


def _hip():
    from quant import _hip
    return _hip


def _dev(c):
    for k in ('gy', 'x', 'xs'):
        c[k + '_d'] = c[k].to(DEV)
    return c


def _run(c, gy=None, x=None, alpha=C.ALPHA):
    return _hip().linear_signx_wgrad(c['gy_d'] if gy is None else gy, c['x_d'] if x is None else x, c['xs_d'], alpha,
                                     c['n'], c['t'], c['f'], c['o'])


def _check(c, gwq, ref=None):
    ref = C.reference64(c, DEV) if ref is None else ref
    err = (gwq.cpu().double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"wgrad N={c['n']} T={c['t']} F={c['f']} O={c['o']} kx={c['xs'].shape[0]}: err/max = {err / scale:.3e}")
    assert tuple(gwq.shape) == (c['o'], c['f'])
    assert err <= BOUND * scale, (c['m'], c['f'], c['o'], err / scale)
    return ref, scale


ACCURACY = C.accuracy_cases()


@pytest.mark.parametrize('i', range(len(ACCURACY)), ids=[f'{s}-M{m}-O{o}-F{f}' for s, m, o, f, _ in ACCURACY])
def test_kernel_against_fp64(i):
    """Every scheme x every summed length M (one row per sample); output and input features rotate.  Where M >= 1000 a
    single bf16 operand misses the bound by at least 10x, so the lo pass is needed and present.  The seeds are those at
    which the prescribed arithmetic alone stays within half the bound (test_linear_wgrad_host.py, on the CPU)."""
    scheme, m, o, f, seed = ACCURACY[i]
    c = _dev(C.make(m, 1, f, o, scheme, seed))
    ref, scale = _check(c, _run(c))
    if m >= 1000:
        e1 = (C.emulated64(c, lo_pass=False, device=DEV) - ref).abs().max().item()
        print(f'  one bf16 operand: err/max = {e1 / scale:.3e}')
        assert e1 >= 10 * BOUND * scale


@pytest.mark.parametrize('n,t', [(6, 3), (5, 7)])
@pytest.mark.parametrize('f', [128, 96])
@pytest.mark.parametrize('scheme', ['ls-2', 'gf-3'])
def test_rows_per_sample(n, t, f, scheme):
    """Input [N, T, F] with per-SAMPLE scales: row m takes the scales of sample m // T (another sample's scale moves the
    signs and the operand far outside the bound)."""
    c = _dev(C.make(n, t, f, 50, scheme, seed=200 + 10 * n + t))
    assert c['xs'].shape == (C.planes(scheme), n) and float(c['xs'][0].std()) > 0
    _check(c, _run(c))


EDGES = [(300, 1033, 1000, 'gf-3'),      # 64 x 64 tiles (17 x 16 of them), 4-byte gradient loads, ragged M, O and F
         (65, 1032, 1000, 'gf-2'),       # 64 x 64 tiles, 16-byte gradient loads, one row past a word
         (2048, 2048, 2048, 'ls-2'),     # 128 x 128 tiles (16 x 16), 16-byte loads: the MLP geometry
         (130, 2047, 2041, 'ls-T'),      # 128 x 128 tiles, 4-byte loads, ragged M, O and F
         (1024, 800, 1000, 'ls-2'),      # 208 tiles of 64 x 64: 32 x 32 tiles, the units split over 8 waves
         (8192, 130, 65, 'ls-1'),        # long K, few tiles: 15 workgroups, 512 units in 8 ranges
         (64, 500, 800, 'ls-2')]         # LeNet fc1: one word, 8 units, one per wave


@pytest.mark.parametrize('i', range(len(EDGES)), ids=[f'M{m}-O{o}-F{f}' for m, o, f, _ in EDGES])
def test_kernel_variants_and_edge_tiles(i):
    m, o, f, scheme = EDGES[i]
    c = _dev(C.make(m, 1, f, o, scheme, seed=300 + i))
    _check(c, _run(c))


@pytest.mark.parametrize('kx', [1, 2, 3])
@pytest.mark.parametrize('m,o', [(70, 40), (9, 7)])
def test_signs_at_the_edge_values_of_the_chain(kx, m, o):
    """Explicit scales (exact in fp32, another set per row) and rows that hold +0.0 and -0.0, +-alpha, values beyond alpha,
    +-v1 (the second residual is exactly 0), +-v1 +- v2 and +-v1 +- v2 +- v3: sign(+-0) = +1 at every step of the chain.  A
    wrong sign moves an output by 2 v gy."""
    f = 48
    rows = torch.arange(m, dtype=torch.float32)
    v = torch.stack([0.5 + rows / 128, 0.25 + rows / 512, 0.0625 + rows / 1024])[:kx].contiguous()
    x = detgen.normal('linwgrad.edge.x', (m, f), seed=kx, scale=1.2)
    v1, v2, v3 = v[0], v[1 % kx], v[2 % kx]
    special = [torch.zeros(m), -torch.zeros(m), torch.full((m,), C.ALPHA), torch.full((m,), -C.ALPHA), torch.full((m,), 3.0),
               torch.full((m,), -2.5), v1, -v1, v1 + v2, v1 - v2, -v1 + v2, -v1 - v2, (v1 + v2) + v3, (v1 + v2) - v3,
               (v1 - v2) + v3, (v1 - v2) - v3, (-v1 + v2) + v3, (-v1 + v2) - v3, (-v1 - v2) + v3, (-v1 - v2) - v3]
    for j, col in enumerate(special):
        x[:, 2 * j] = col                               # (the odd columns keep random values)
    assert torch.signbit(x[:, 2]).all() and (x[:, 2] == 0).all()
    c = _dev(C.make(m, 1, f, o, None, seed=400 + kx, xs=v, x=x))
    if kx >= 2:                                         # the chain does meet exact zeros: x = v1 gives d_2 = +0
        assert ((x.clamp(-C.ALPHA, C.ALPHA) - v1.view(-1, 1) * c['signs'][0]) == 0).any()
    gwq = _run(c)
    ref, scale = _check(c, gwq)
    flipped = [b.clone() for b in c['signs']]
    flipped[-1][0, 0] = -flipped[-1][0, 0]              # what ONE wrong sign would cost: far outside the bound
    wrong = C.reference64(dict(c, signs=flipped), DEV)
    assert (wrong - ref).abs().max().item() > 100 * BOUND * scale


# ------------------------------------------------------------------------------------------------ output buffer, alignment
def _raw_call(c, gy_ptr, x_ptr, gwq_ptr, kx=None):
    wl = _hip().linear_wgrad_lib()
    k = c['xs'].shape[0]
    need = int(wl.lsq_linear_signx_wgrad_workspace_bytes(k, c['n'], c['t'], c['f'], c['o']))
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    code = wl.lsq_linear_signx_wgrad(gy_ptr, x_ptr, k if kx is None else kx, c['xs_d'].data_ptr(), C.ALPHA, c['n'], c['t'],
                                     c['f'], c['o'], gwq_ptr, ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    return code


def _shifted(t):
    """A copy of ``t`` whose data pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty((t.numel() + 1,), device=DEV)
    buf[1:] = t.reshape(-1)
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize('shape', [(64, 500, 800, 'ls-2'), (65, 1032, 1000, 'gf-3'), (130, 2048, 2048, 'ls-1'),
                                   (300, 1033, 1000, 'ls-T'), (7, 33, 65, 'gf-2')])
def test_output_buffer_and_unaligned_operands(shape):
    """gwq written exactly into its place inside a NaN-filled buffer; gy, and x, at an address 4 bytes past 16 give the same
    bits as the aligned call.  With O % 4 == 0 that compares the 16-byte and the 4-byte gradient loads: (500, 800) on the
    split kernel, (1032, 1000) on 64 x 64 and (2048, 2048) on 128 x 128 tiles."""
    m, o, f, scheme = shape
    c = _dev(C.make(m, 1, f, o, scheme, seed=500 + m))
    pad = 37
    buf = torch.full((pad + o * f + pad,), float('nan'), device=DEV)
    assert _raw_call(c, c['gy_d'].data_ptr(), c['x_d'].data_ptr(), buf.data_ptr() + 4 * pad) == 0
    gwq = buf[pad:pad + o * f].view(o, f)
    assert not torch.isnan(gwq).any()
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + o * f:]).all()
    _check(c, gwq)
    bits = gwq.contiguous().view(torch.int32)
    assert torch.equal(_run(c).view(torch.int32), bits)
    assert torch.equal(_run(c, gy=_shifted(c['gy_d'])).view(torch.int32), bits)
    assert torch.equal(_run(c, x=_shifted(c['x_d'])).view(torch.int32), bits)


@pytest.mark.parametrize('shape', [(64, 500, 800, 'ls-2'), (1024, 1032, 1000, 'gf-3'), (512, 2048, 2048, 'ls-1')])
def test_two_calls_give_the_same_bits(shape):
    m, o, f, scheme = shape
    c = _dev(C.make(m, 1, f, o, scheme, seed=600 + m))
    g1, g2 = _run(c), _run(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g3 = _run(c)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for g in (g2, g3):
        assert torch.equal(g1.view(torch.int32), g.view(torch.int32))


@pytest.mark.parametrize('kx', [9, 0])
def test_unsupported_plane_counts_are_refused_and_write_nothing(kx):
    c = _dev(C.make(16, 1, 128, 40, 'gf-8', seed=700))
    gwq = torch.full((40, 128), 12345.0, device=DEV)
    assert _raw_call(c, c['gy_d'].data_ptr(), c['x_d'].data_ptr(), gwq.data_ptr(), kx=kx) == E_UNSUPPORTED
    assert (gwq == 12345.0).all()


# ------------------------------------------------------------------------------------------------ the train step
@pytest.fixture
def kernel_on(monkeypatch):
    import quant.binary.hip_train_linear as HTL
    monkeypatch.setattr(HTL, 'WGRAD_KERNEL', True)
    return HTL


def _twins(xs, ws, f, o, bias, clamp=SYM, tag='step'):
    from quant.binary import QuantLinear
    mods = []
    for hip_path in (True, False):
        lin = QuantLinear(xs, ws, f, o, clamp, bias=bias)
        with torch.no_grad():
            lin.weight.copy_(detgen.normal(f'linwgrad.{tag}.w', lin.weight.shape, scale=0.3))
            if bias:
                lin.bias.copy_(detgen.normal(f'linwgrad.{tag}.b', lin.bias.shape, scale=0.1))
        lin.hip_train = hip_path
        mods.append(lin.to(DEV).train())
    return mods


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


PAIRS = [('ls-2', 'ls-1'), ('ls-1', 'ls-1'), ('gf-2', 'ls-1'), ('ls-T', 'ls-1'), ('ls-1', 'gf-2'), ('ls-1', 'ls-2'),
         ('ls-2', 'ls-T'), ('gf-4', 'gf-3')]
STEP_CASES = [(xs, ws, shape, bias) for xs, ws in PAIRS for bias in (True, False) for shape in [(64, 800), (6, 3, 128)]]


@pytest.mark.parametrize('xs,ws,shape,bias', STEP_CASES)
def test_train_step_with_the_kernel_equals_the_torch_formulation(xs, ws, shape, bias, kernel_on):
    """One train-mode step of QuantLinear with hip_train and WGRAD_KERNEL (the weight gradient on lsq_linear_signx_wgrad)
    against the SAME module on the torch formulation on the device: output, the three gradients, the cached weight scales.
    gw: 2e-5, the figure test_gpu_linear_train.py grants a bf16 hi + lo GEMM against fp32 torch (its gx)."""
    o = 50
    l1, l2 = _twins(xs, ws, shape[-1], o, bias)
    out = []
    for lin in (l1, l2):
        x = detgen.normal(f'linwgrad.step.x.{shape}', shape, scale=1.2).to(DEV).requires_grad_()
        y = lin(x)
        y.backward(detgen.normal(f'linwgrad.step.gy.{shape}', (*shape[:-1], o)).to(DEV))
        out.append((x, y))
    (x1, y1), (x2, y2) = out
    assert type(y1.grad_fn).__name__ == '_QuantLinearStepBackward' and type(y2.grad_fn).__name__ != '_QuantLinearStepBackward'
    r = dict(y=_rel(y1, y2), gx=_rel(x1.grad, x2.grad), gw=_rel(l1.weight.grad, l2.weight.grad),
             gb=_rel(l1.bias.grad, l2.bias.grad) if bias else 0.0)
    print('train step rel. errors:', {k: f'{v:.2e}' for k, v in r.items()})
    assert r['y'] <= 1e-5, r
    assert r['gx'] <= 2e-5, r
    assert r['gw'] <= 2e-5, r
    assert r['gb'] <= 1e-5, r
    for (n1, b1), (n2, b2) in zip(l1.w_approximate.named_buffers(), l2.w_approximate.named_buffers()):
        assert n1 == n2 and torch.equal(b1, b2) and float(b1.abs().sum()) > 0, n1


def test_two_forwards_then_both_backwards(kernel_on):
    l1, l2 = _twins('ls-2', 'ls-2', 128, 50, True, tag='two')
    res = []
    for lin in (l1, l2):
        xa = detgen.normal('linwgrad.two.xa', (6, 3, 128), scale=1.2).to(DEV).requires_grad_()
        xb = detgen.normal('linwgrad.two.xb', (5, 128), scale=0.7).to(DEV).requires_grad_()
        ya, yb = lin(xa), lin(xb)
        ya.backward(detgen.normal('linwgrad.two.ga', (6, 3, 50)).to(DEV))
        ga_w, ga_b = lin.weight.grad.clone(), lin.bias.grad.clone()
        lin.weight.grad = None
        lin.bias.grad = None
        yb.backward(detgen.normal('linwgrad.two.gb', (5, 50)).to(DEV))
        res.append((ya, yb, xa.grad, xb.grad, ga_w, ga_b, lin.weight.grad, lin.bias.grad))
    bounds = (1e-5, 1e-5, 2e-5, 2e-5, 2e-5, 1e-5, 2e-5, 1e-5)
    for a, b, bound in zip(res[0], res[1], bounds):
        assert _rel(a, b) <= bound, (_rel(a, b), bound)


STEP_FUNCTIONS = ('linear_signw_dgrad', 'linear_signx_wgrad', 'quant_values', 'ste_backward')


@pytest.fixture
def counters(monkeypatch):
    hip = _hip()
    calls = {name: 0 for name in STEP_FUNCTIONS}

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper

    for name in STEP_FUNCTIONS:
        monkeypatch.setattr(hip, name, counted(name, getattr(hip, name)))
    return calls


def test_what_the_step_launches(kernel_on, counters):
    l1, _ = _twins('ls-2', 'ls-1', 128, 50, True, tag='need')
    x = detgen.normal('linwgrad.need.x', (6, 3, 128), scale=1.2).to(DEV)
    gy = detgen.normal('linwgrad.need.gy', (6, 3, 50)).to(DEV)
    l1(x.clone().requires_grad_()).backward(gy)
    assert counters == dict(linear_signw_dgrad=1, linear_signx_wgrad=1, quant_values=0, ste_backward=2)
    for k in counters:
        counters[k] = 0
    l1.weight.requires_grad_(False)                                   # a frozen weight: neither route
    xg = x.clone().requires_grad_()
    l1(xg).backward(gy)
    assert counters == dict(linear_signw_dgrad=1, linear_signx_wgrad=0, quant_values=0, ste_backward=1)
    assert xg.grad is not None


@pytest.mark.parametrize('flag', [True, False])
def test_fp_activations_keep_torch_mm(flag, monkeypatch, counters):
    import quant.binary.hip_train_linear as HTL
    monkeypatch.setattr(HTL, 'WGRAD_KERNEL', flag)
    l1, l2 = _twins('fp', 'ls-1', 128, 50, True, tag='fp')
    x = detgen.normal('linwgrad.fp.x', (6, 3, 128), scale=1.2).to(DEV)
    gy = detgen.normal('linwgrad.fp.gy', (6, 3, 50)).to(DEV)
    y = l1(x)
    assert type(y.grad_fn).__name__ == '_QuantLinearStepBackward'
    y.backward(gy)
    l2(x).backward(gy)
    assert counters['linear_signx_wgrad'] == 0 and counters['quant_values'] == 1
    assert _rel(l1.weight.grad, l2.weight.grad) <= 1e-5


def test_the_default_step_does_not_call_the_kernel(counters):
    import quant.binary.hip_train_linear as HTL
    assert HTL.WGRAD_KERNEL is False
    l1, _ = _twins('ls-2', 'ls-1', 128, 50, True, tag='off')
    x = detgen.normal('linwgrad.off.x', (6, 3, 128), scale=1.2).to(DEV)
    l1(x).backward(detgen.normal('linwgrad.off.gy', (6, 3, 50)).to(DEV))
    assert counters['linear_signx_wgrad'] == 0 and counters['quant_values'] == 1


# ------------------------------------------------------------------------------------------------ the training loop
def test_lenet_fc1_trains_with_the_kernel(kernel_on, counters):
    """quant.common.training.train on cuda:0 with QLeNet5's fc1 a QuantLinear (ls-2 activations) on hip_train with
    WGRAD_KERNEL: every step's weight gradient comes from the kernel (12 = 3 epochs x 4 batches), the loss falls, and the
    first epoch agrees with the torch formulation's from the same seed (rel 2e-2, as test_gpu_linear_train.py)."""
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
    losses = {}
    for hip_path in (True, False):
        torch.manual_seed(11)
        model = QLeNet5(loss_fn=torch.nn.functional.nll_loss, x_quant='ls-2', w_quant='ls-1', clamp=clamp, fc1_quant=fc1q).to(DEV)
        model.fc1.hip_train = hip_path
        opt = get_optimizer(model.parameters(), {'algorithm': 'sgd', 'lr': 0.02, 'momentum': 0.9})
        sched = get_lr_scheduler(opt, {'scheduler': 'step_lr', 'step_size': 10, 'gamma': 0.5}, 3, len(loader))
        metrics = {'Loss': LossMetric(model.loss_fn, accumulate=True)}
        losses[hip_path] = [train(model, loader, metrics, opt, sched, torch.device(DEV), e, 100)['Loss'] for e in (1, 2, 3)]
    print('losses', losses)
    assert counters['linear_signx_wgrad'] == 4 * 3                  # 4 batches x 3 epochs, the hip_train model only
    assert losses[True][2] < losses[True][0]
    assert losses[True][0] == pytest.approx(losses[False][0], rel=2e-2)
