"""lsq_linear_signw_dgrad (liblsq_hip_linear_train.so) and the train step of QuantLinear on the GPU: the kernel against fp64
for every weight depth and both kernels, the output buffer and unaligned gradients, determinism, a refused call that writes
nothing; the autograd step (quant.binary.hip_train_linear) against the torch formulation on the device -- schemes, shapes,
moving-average modes, two forwards before backward, what is launched and what is not, LeNet's fc1 in the training loop."""

import pytest
import torch

import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BOUND = 1e-5      # |gx - gx64| <= BOUND * max |gx64|: the bound test_gpu_linear_fp.py holds the forward to
SYM = {'kind': 'symmetric', 'alpha': 2}
E_UNSUPPORTED = -6


def _hip():
    from quant import _hip
    return _hip


def _wscales(w, ws):
    """Scales [kw, O] of the sign planes lsq_pack_weight writes (ls-T: two planes of one scale) and the oracle's list.
    Rows too short for the scale solve (ls-2 at F = 1) get 0.25 * 2^-q, the scales the greedy quantizer tends to for
    uniform(-0.5, 0.5) weights (mean |w| = 0.25, every plane halves the residual's range).  Unlike the forward, this
    kernel multiplies the scale into the operand BEFORE the bf16 split, so scales that are no quantization of w (1, 0.6 for
    |w| < 0.5 makes every w_q = +-(1 - 0.6): the planes cancel 4-fold) would test cancellation the quantizers never produce."""
    o, f = w.shape
    try:
        sc = P.weight_scales(w.view(o, f, 1, 1), ws)
    except RuntimeError:
        k = {'ls-1': 1, 'ls-2': 2, 'ls-T': 1}.get(ws) or int(ws[3:])
        sc = [torch.full((o,), 0.25 * 0.5 ** q) for q in range(k)]
    planes = [sc[0], sc[0]] if ws == 'ls-T' else list(sc)
    return torch.stack(planes).contiguous(), sc


def _signs(w, wsc):
    """The +-1 planes as the oracle forms them: s_q = sign(w - sum_(p<q) ws_p s_p) in fp32, sign(0) = +1."""
    out, acc = [], torch.zeros_like(w)
    for q in range(wsc.shape[0]):
        r = w - acc
        s = torch.where(r < 0, -torch.ones_like(r), torch.ones_like(r))
        out.append(s.double())
        acc = acc + wsc[q].view(-1, 1) * s
    return out


def _case(m, f, o, ws, seed):
    hip = _hip()
    gy = detgen.normal(f'lintrain.gy.{seed}', (m, o), seed=seed)
    w = detgen.uniform(f'lintrain.w.{seed}', (o, f), -0.5, 0.5, seed=seed)
    wsc, sc = _wscales(w, ws)
    g = hip.make_geom(1, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    wbits, _ = hip.pack_weight(w.to(DEV).view(o, f, 1, 1), g, wsc.to(DEV))
    wq = P.quantize_weight(w.view(o, f, 1, 1), ws, sc).view(o, f)
    gx64 = (gy.double().to(DEV) @ wq.double().to(DEV)).cpu()
    return dict(gy=gy.to(DEV), gy_cpu=gy, w=w, wbits=wbits, wsc=wsc.to(DEV), wsc_cpu=wsc, m=m, f=f, o=o, wq=wq, gx64=gx64)


def _run(c, gy=None):
    return _hip().linear_signw_dgrad(c['gy'] if gy is None else gy, c['wbits'], c['wsc'], c['m'], c['f'], c['o'])


def _check(c, gx):
    ref = c['gx64']
    err = (gx.cpu().double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"dgrad M={c['m']} F={c['f']} O={c['o']} kw={c['wsc'].shape[0]}: err/max = {err / scale:.3e}")
    assert err <= BOUND * scale, (c['m'], c['f'], c['o'], err / scale)
    return err, scale


def _one_bf16_operand(c):
    """gx with ONE bf16 operand per product, (gy ws).bfloat16(), everything else in fp64."""
    signs = _signs(c['w'], c['wsc_cpu'])
    wq = sum(c['wsc_cpu'][q].double().view(-1, 1) * s for q, s in enumerate(signs))
    assert torch.allclose(wq, c['wq'].double(), rtol=0, atol=1e-6)                 # the planes are the oracle's w_q
    dev = DEV if c['m'] * c['f'] * c['o'] > 1 << 28 else 'cpu'
    out = 0
    for q, s in enumerate(signs):
        a = (c['gy_cpu'] * c['wsc_cpu'][q].view(1, -1)).bfloat16().double()
        out = out + (a.to(dev) @ s.to(dev)).cpu()
    return out


WS = ('ls-1', 'ls-2', 'ls-T', 'gf-2', 'gf-3', 'gf-8')
OS = (1, 63, 64, 65, 800, 4096)       # the summed dimension
FS = (1, 10, 33, 1000)
MS = (1, 7, 16, 256)


@pytest.mark.parametrize('ws', WS)
@pytest.mark.parametrize('oi', range(len(OS)))
def test_kernel_against_fp64(ws, oi):
    """Every weight depth x every count of output features (the summed dimension); input features and rows rotate so that
    every value of each meets several depths.  Where O >= 800, a single bf16 operand misses the bound by at least 10x (so
    the lo term is needed and present).
    Seeds: with ONE output (M = F = 1) max |ref| is a single random sum of O terms, and a draw in which it cancels puts the
    prescribed arithmetic itself outside the bound -- hi + lo summed EXACTLY (fp64, on the CPU) is 1.12e-5 of |ref| at
    (1, 1, 800) ls-1 with seed 4.  The seed base below is the first of 0, 1000, 2000, ... at which that exact hi + lo sum is
    within half the bound at all 36 cases (worst 3.8e-6); the choice was made on the CPU and never looked at the kernel."""
    wi = WS.index(ws)
    o, f, m = OS[oi], FS[(oi + wi) % 4], MS[(oi + 2 * wi) % 4]
    c = _case(m, f, o, ws, seed=1000 + 100 * wi + oi)
    err, scale = _check(c, _run(c))
    if o >= 800:
        e1 = (_one_bf16_operand(c) - c['gx64']).abs().max().item()
        print(f'  one bf16 operand: err/max = {e1 / scale:.3e}')
        assert e1 >= 10 * BOUND * scale


# the ragged tiled shapes of test_gpu_linear_fp.py (M, F, O, scheme) with F and O exchanged
TILED = [(1000, 1033, 65, 'gf-3'), (1024, 1000, 800, 'ls-2'), (4100, 2000, 130, 'ls-1'), (300, 4100, 1, 'ls-T')]


@pytest.mark.parametrize('i', range(len(TILED)))
def test_tiled_kernel_edges(i):
    """Shapes with at least 256 tiles of 64 x 64 in M x F (the tiled kernel, 64 x 64 and 128 x 128 tiles), ragged rows,
    columns and summed dimension."""
    m, f, o, ws = TILED[i]
    c = _case(m, f, o, ws, seed=300 + i)
    _check(c, _run(c))


def test_kernel_at_the_mlp_shape():
    c = _case(8192, 4096, 4096, 'ls-2', seed=400)
    err, scale = _check(c, _run(c))
    e1 = (_one_bf16_operand(c) - c['gx64']).abs().max().item()
    assert e1 >= 10 * BOUND * scale


# ------------------------------------------------------------------------------------------------ output buffer, alignment
def _raw_call(c, gy_ptr, gx_ptr, kw=None):
    hip = _hip()
    tl = hip.linear_train_lib()
    kw = c['wsc'].shape[0] if kw is None else kw
    need = int(tl.lsq_linear_signw_dgrad_workspace_bytes(c['wsc'].shape[0], c['f'], c['o']))
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    code = tl.lsq_linear_signw_dgrad(gy_ptr, c['wbits'].data_ptr(), kw, c['wsc'].data_ptr(), c['m'], c['f'], c['o'], gx_ptr,
                                     ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    return code


@pytest.mark.parametrize('shape', [(7, 33, 65, 'ls-2'), (16, 1000, 800, 'gf-3'), (1000, 1033, 65, 'ls-1'),
                                   (4100, 2000, 130, 'gf-2'), (1024, 1000, 800, 'ls-T'), (2048, 2048, 800, 'gf-3')])
def test_output_buffer_and_unaligned_gradient(shape):
    """gx written exactly into its place inside a NaN-filled buffer; gy at an address 4 bytes past 16 gives the same bits
    as the aligned gy.  With O % 4 == 0 that compares the 16-byte and the 4-byte load paths: (16, 800) on the split kernel,
    (1024, 800) on 64 x 64 and (2048, 800) on 128 x 128 tiles."""
    m, f, o, ws = shape
    c = _case(m, f, o, ws, seed=500 + m)
    pad = 37
    buf = torch.full((pad + m * f + pad,), float('nan'), device=DEV)
    assert _raw_call(c, c['gy'].data_ptr(), buf.data_ptr() + 4 * pad) == 0
    gx = buf[pad:pad + m * f].view(m, f)
    assert not torch.isnan(gx).any()
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + m * f:]).all()
    _check(c, gx)
    gbuf = torch.empty((m * o + 1,), device=DEV)
    gbuf[1:] = c['gy'].view(-1)
    gu = gbuf[1:].view(m, o)                      # data pointer 4 bytes past a 16-byte boundary
    assert gu.data_ptr() % 16 == 4
    gxu = _run(c, gu)
    assert torch.equal(gxu.view(torch.int32), gx.contiguous().view(torch.int32))


@pytest.mark.parametrize('shape', [(16, 4096, 4096, 'ls-2'), (1024, 1000, 800, 'gf-3'), (64, 800, 500, 'ls-1')])
def test_two_calls_give_the_same_bits(shape):
    m, f, o, ws = shape
    c = _case(m, f, o, ws, seed=600 + m)
    g1, g2 = _run(c), _run(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g3 = _run(c)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for g in (g2, g3):
        assert torch.equal(g1.view(torch.int32), g.view(torch.int32))


def test_nine_planes_are_refused_and_write_nothing():
    c = _case(16, 128, 40, 'gf-8', seed=700)
    gx = torch.full((16, 128), 12345.0, device=DEV)
    assert _raw_call(c, c['gy'].data_ptr(), gx.data_ptr(), kw=9) == E_UNSUPPORTED
    assert (gx == 12345.0).all()


# ------------------------------------------------------------------------------------------------ the train step
def _twins(xs, ws, f, o, bias, clamp=SYM, mode='off', momentum=0.99, tag='step'):
    from quant.binary import QuantLinear
    mods = []
    for hip_path in (True, False):
        lin = QuantLinear(xs, ws, f, o, clamp, mode, momentum, bias=bias)
        with torch.no_grad():
            lin.weight.copy_(detgen.normal(f'lintrain.{tag}.w', lin.weight.shape, scale=0.3))
            if bias:
                lin.bias.copy_(detgen.normal(f'lintrain.{tag}.b', lin.bias.shape, scale=0.1))
        lin.hip_train = hip_path
        mods.append(lin.to(DEV).train())
    return mods


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _assert_step_close(x1, y1, l1, x2, y2, l2, bias):
    r = dict(y=_rel(y1, y2), gx=_rel(x1.grad, x2.grad), gw=_rel(l1.weight.grad, l2.weight.grad),
             gb=_rel(l1.bias.grad, l2.bias.grad) if bias else 0.0)
    print('train step rel. errors:', {k: f'{v:.2e}' for k, v in r.items()})
    assert r['y'] <= 1e-5, r
    assert r['gx'] <= 2e-5, r                     # (bf16 hi + lo terms of the transposed GEMM)
    assert r['gw'] <= 1e-5, r
    assert r['gb'] <= 1e-5, r


PAIRS = [('ls-2', 'ls-1'), ('ls-1', 'ls-1'), ('gf-2', 'ls-1'), ('ls-T', 'ls-1'), ('fp', 'ls-1'), ('fp', 'ls-2'), ('fp', 'ls-T'),
         ('ls-1', 'gf-2'), ('ls-1', 'ls-2'), ('ls-2', 'ls-T'), ('gf-4', 'gf-3')]
STEP_CASES = [(xs, ws, shape, bias) for xs, ws in PAIRS for bias in (True, False)
              for shape in [(64, 800), (6, 3, 128)] + ([(4, 3, 96)] if xs == 'fp' else [])]


@pytest.mark.parametrize('xs,ws,shape,bias', STEP_CASES)
def test_train_step_on_the_kernels_equals_the_torch_formulation(xs, ws, shape, bias):
    """One train-mode step of QuantLinear through quant.binary.hip_train_linear (forward on lsq_act_quant + lsq_linear_xnor /
    lsq_linear_signw, backward on lsq_linear_signw_dgrad + lsq_ste_backward + lsq_quant_values) against the SAME module on
    the torch formulation on the device (autograd through STESign): output, the three gradients, the cached weight scales."""
    o = 50
    l1, l2 = _twins(xs, ws, shape[-1], o, bias)
    out = []
    for lin in (l1, l2):
        x = detgen.normal(f'lintrain.step.x.{shape}', shape, scale=1.2).to(DEV).requires_grad_()
        y = lin(x)
        assert tuple(y.shape) == (*shape[:-1], o)
        y.backward(detgen.normal(f'lintrain.step.gy.{shape}', (*shape[:-1], o)).to(DEV))
        out.append((x, y))
    (x1, y1), (x2, y2) = out
    assert type(y1.grad_fn).__name__ == '_QuantLinearStepBackward' and type(y2.grad_fn).__name__ != '_QuantLinearStepBackward'
    _assert_step_close(x1, y1, l1, x2, y2, l2, bias)
    for (n1, b1), (n2, b2) in zip(l1.w_approximate.named_buffers(), l2.w_approximate.named_buffers()):
        assert n1 == n2 and torch.equal(b1, b2) and float(b1.abs().sum()) > 0, n1
    if xs != 'fp':
        assert l1.last_act_scales.shape == (l1.x_approximate.n_planes, shape[0])


@pytest.mark.parametrize('mode', ['eval_only', 'train_and_eval'])
def test_train_step_moving_average_modes_on_the_kernels(mode):
    """The activation quantizer's moving average in training: it tracks the batch's mean scales; 'train_and_eval' quantizes
    with the tracked values.  Kernels against the torch formulation over three steps, tracked buffers included."""
    l1, l2 = _twins('ls-2', 'ls-1', 128, 40, True, {'kind': 'symmetric', 'alpha': 3}, mode, 0.9, tag='ma')
    for step in range(3):
        ys = []
        for lin in (l1, l2):
            x = detgen.normal(f'lintrain.ma.x{step}', (6, 3, 128), scale=1.1).to(DEV).requires_grad_()
            y = lin(x)
            y.sum().backward()
            ys.append((y, x.grad))
        assert type(ys[0][0].grad_fn).__name__ == '_QuantLinearStepBackward'
        assert float((ys[0][0] - ys[1][0]).abs().max()) <= 1e-5 * float(ys[1][0].abs().max())
        assert float((ys[0][1] - ys[1][1]).abs().max()) <= 2e-5 * float(ys[1][1].abs().max())
        ma = [m.x_approximate.moving_avg_module.moving_average for m in (l1, l2)]
        assert torch.allclose(ma[0], ma[1], rtol=2e-6), (step, ma)


@pytest.mark.parametrize('xs', ['ls-2', 'fp'])
def test_two_forwards_then_both_backwards(xs):
    """What backward reads belongs to the step: a second forward of the same module (another input, other activation
    scales) before the first backward changes nothing."""
    l1, l2 = _twins(xs, 'ls-2', 128, 50, True, tag='two')
    res = []
    for lin in (l1, l2):
        xa = detgen.normal('lintrain.two.xa', (6, 3, 128), scale=1.2).to(DEV).requires_grad_()
        xb = detgen.normal('lintrain.two.xb', (5, 128), scale=0.7).to(DEV).requires_grad_()
        ya, yb = lin(xa), lin(xb)
        ya.backward(detgen.normal('lintrain.two.ga', (6, 3, 50)).to(DEV))
        ga_w, ga_b = lin.weight.grad.clone(), lin.bias.grad.clone()
        lin.weight.grad = None
        lin.bias.grad = None
        yb.backward(detgen.normal('lintrain.two.gb', (5, 50)).to(DEV))
        res.append((ya, yb, xa.grad, xb.grad, ga_w, ga_b, lin.weight.grad, lin.bias.grad))
    bounds = (1e-5, 1e-5, 2e-5, 2e-5, 1e-5, 1e-5, 1e-5, 1e-5)
    for a, b, bound in zip(res[0], res[1], bounds):
        assert _rel(a, b) <= bound, (_rel(a, b), bound)


def test_second_derivative_raises():
    l1, _ = _twins('ls-2', 'ls-1', 128, 50, True, tag='dd')
    x = detgen.normal('lintrain.dd.x', (6, 128), scale=1.2).to(DEV).requires_grad_()
    y = l1(x)
    (g,) = torch.autograd.grad(y.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ------------------------------------------------------------------------------------------------ what is launched
STEP_FUNCTIONS = ('act_quant', 'pack_weight', 'linear_xnor', 'linear_signw', 'linear_signw_dgrad', 'quant_values', 'ste_backward')


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


@pytest.mark.parametrize('xs', ['ls-2', 'fp'])
def test_nothing_is_computed_for_an_input_that_needs_no_gradient(xs, counters):
    l1, _ = _twins(xs, 'ls-1', 128, 50, True, tag='need')
    x = detgen.normal('lintrain.need.x', (6, 3, 128), scale=1.2).to(DEV)
    gy = detgen.normal('lintrain.need.gy', (6, 3, 50)).to(DEV)
    l1(x).backward(gy)                                                # the input wants no gradient
    assert counters['linear_signw_dgrad'] == 0
    assert counters['quant_values'] == 1 and counters['ste_backward'] == 1        # the weight's
    assert l1.weight.grad is not None and l1.bias.grad is not None
    for k in counters:
        counters[k] = 0
    l1.weight.requires_grad_(False)                                   # a frozen weight
    xg = x.clone().requires_grad_()
    l1(xg).backward(gy)
    assert counters['linear_signw_dgrad'] == 1 and counters['ste_backward'] == 1  # the input's
    assert counters['quant_values'] == 0
    assert xg.grad is not None


def test_paths_that_stay_on_torch(counters):
    from quant.binary import QuantLinear
    x = detgen.normal('lintrain.torch.x', (5, 3, 128), scale=1.2).to(DEV)

    def module(xs, ws, f, flag):
        m = QuantLinear(xs, ws, f, 20, SYM)
        with torch.no_grad():
            m.weight.copy_(detgen.normal('lintrain.torch.w', m.weight.shape, scale=0.3))
        m.hip_train = flag
        return m.to(DEV).train()

    cases = [(module('ls-2', 'ls-1', 128, False), x),                 # hip_train = False (the default)
             (module('ls-2', 'fp', 128, True), x),                    # fp weights
             (module('fp', 'gf-9', 128, True), x),                    # nine weight planes
             (module('ls-1', 'ls-1', 128, True).double(), x.double()),            # fp64 module and input
             (module('ls-2', 'ls-1', 96, True), x[..., :96].contiguous())]        # binary activations, T > 1, F % 64 != 0
    for mod, xin in cases:
        xin = xin.clone().requires_grad_()
        y = mod(xin)
        ref = mod._forward_torch(xin)
        assert torch.equal(y, ref)
        assert type(y.grad_fn).__name__ != '_QuantLinearStepBackward'
        y.sum().backward()
    assert all(v == 0 for v in counters.values()), counters
    assert QuantLinear.hip_train is False


# ------------------------------------------------------------------------------------------------ the training loop
@pytest.mark.parametrize('xs', ['ls-2', 'fp'])
def test_lenet_fc1_trains_on_the_kernels(xs):
    """quant.common.training.train on cuda:0 with QLeNet5's fc1 a QuantLinear: with hip_train its step runs on the kernels
    (12 = 3 epochs x 4 batches), the loss falls, and the first epoch agrees with the torch formulation's from the same seed
    (rel 2e-2: a binarized net amplifies fp32 reassociation, as in the convolution's training-loop test)."""
    import quant.binary.hip_train_linear as HTL
    from quant.common.initialization import get_lr_scheduler, get_optimizer
    from quant.common.metrics import LossMetric
    from quant.common.training import train
    from quant.models.lenet import QLeNet5
    clamp = {'kind': 'symmetric', 'alpha': 3}
    fc1q = {'x_quant': xs, 'w_quant': 'ls-1', 'clamp': clamp}
    g = torch.Generator().manual_seed(5)
    data = torch.randn(64, 1, 28, 28, generator=g)
    target = torch.randint(0, 10, (64,), generator=g)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, target), batch_size=16)
    calls = []
    orig = HTL.train_step_forward
    losses = {}
    try:
        HTL.train_step_forward = lambda lin, x: (calls.append(lin), orig(lin, x))[1]
        for hip_path in (True, False):
            torch.manual_seed(11)
            model = QLeNet5(loss_fn=torch.nn.functional.nll_loss, x_quant='ls-2', w_quant='ls-1', clamp=clamp, fc1_quant=fc1q).to(DEV)
            model.fc1.hip_train = hip_path
            opt = get_optimizer(model.parameters(), {'algorithm': 'sgd', 'lr': 0.02, 'momentum': 0.9})
            sched = get_lr_scheduler(opt, {'scheduler': 'step_lr', 'step_size': 10, 'gamma': 0.5}, 3, len(loader))
            metrics = {'Loss': LossMetric(model.loss_fn, accumulate=True)}
            losses[hip_path] = [train(model, loader, metrics, opt, sched, torch.device(DEV), e, 100)['Loss'] for e in (1, 2, 3)]
    finally:
        HTL.train_step_forward = orig
    print('losses', losses)
    assert len(calls) == 4 * 3                                  # 4 batches x 3 epochs, the hip_train model only
    assert losses[True][2] < losses[True][0]
    assert losses[True][0] == pytest.approx(losses[False][0], rel=2e-2)
