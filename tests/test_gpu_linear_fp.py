"""lsq_linear_signw (liblsq_hip_linear_fp.so) and QuantLinear('fp', w) on the GPU: the kernel against fp64 for every weight
depth, both clamps and both kernels, the output buffer and unaligned inputs, determinism, the module's dispatch and weight
cache, the paths that must stay on torch, LeNet's fc1, and a refused call that writes nothing."""

import pytest
import torch
import torch.nn.functional as F

import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BOUND = 1e-5      # |y - y64| <= BOUND * max |y64|
SYM = {'kind': 'symmetric', 'alpha': 2}
IDENT = {'kind': 'identity'}
E_UNSUPPORTED = -6


def _hip():
    from quant import _hip
    return _hip


def _wscales(w, ws):
    """Scales [kw, O] of the sign planes lsq_pack_weight writes (ls-T: two planes of one scale) and the oracle's list."""
    o, f = w.shape
    try:
        sc = P.weight_scales(w.view(o, f, 1, 1), ws)
    except RuntimeError:              # rows too short for the scale solve (F = 1): any positive scales serve the kernel test
        k = {'ls-1': 1, 'ls-2': 2, 'ls-T': 1}.get(ws) or int(ws[3:])
        sc = [torch.full((o,), 0.6 ** q) for q in range(k)]
    planes =[sc[0], sc[0]] if ws == 'ls-T' else list(sc)
    return torch.stack(planes).contiguous(), sc


def _case(m, f, o, ws, clamp, bias, seed):
    hip = _hip()
    x = detgen.normal(f'linfp.x.{seed}', (m, f), seed=seed, scale=1.2)
    w = detgen.uniform(f'linfp.w.{seed}', (o, f), -0.5, 0.5, seed=seed)
    wsc, sc = _wscales(w, ws)
    g = hip.make_geom(1, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    wbits, _ = hip.pack_weight(w.to(DEV).view(o, f, 1, 1), g, wsc.to(DEV))
    b = detgen.normal(f'linfp.b.{seed}', (o,), seed=seed, scale=0.5) if bias else None
    xc = P.clamp_act(x, clamp)
    wq = P.quantize_weight(w.view(o, f, 1, 1), ws, sc).view(o, f)
    y64 = F.linear(xc.double().to(DEV), wq.double().to(DEV), None if b is None else b.double().to(DEV)).cpu()
    return dict(x=x.to(DEV), wbits=wbits, wsc=wsc.to(DEV), b=None if b is None else b.to(DEV), alpha=2.0 if clamp is SYM else -1.0,
                m=m, f=f, o=o, xc=xc, wq=wq, bias_cpu=b, y64=y64)


def _run(c, x=None):
    return _hip().linear_signw(c['x'] if x is None else x, c['alpha'], c['wbits'], c['wsc'], c['b'], c['m'], c['f'], c['o'])


def _check(c, y):
    y64 = c['y64']
    err = (y.cpu().double() - y64).abs().max().item()
    scale = y64.abs().max().item()
    assert err <= BOUND * scale, (c['m'], c['f'], c['o'], err / scale)
    return err, scale


WS = ('ls-1', 'ls-2', 'ls-T', 'gf-2', 'gf-3', 'gf-8')
FS = (1, 63, 64, 65, 800, 4096)
OS = (1, 10, 33, 1000)
MS = (1, 7, 16, 256)


@pytest.mark.parametrize('ws', WS)
@pytest.mark.parametrize('fi', range(len(FS)))
def test_kernel_against_fp64(ws, fi):
    """Every weight depth x every feature count; out-features, rows, clamp and bias rotate so that every value of each meets
    several depths.  Where F >= 800, a single bf16 activation operand misses the bound by at least 10x (so the lo term is
    needed and present)."""
    wi = WS.index(ws)
    f, o, m = FS[fi], OS[(fi + wi) % 4], MS[(fi + 2 * wi) % 4]
    clamp = SYM if (fi + wi) % 2 else IDENT
    c = _case(m, f, o, ws, clamp, bias=(fi // 2 + wi) % 2 == 0, seed=100 * wi + fi)
    err, scale = _check(c, _run(c))
    if f >= 800:
        b = None if c['bias_cpu'] is None else c['bias_cpu'].double()
        y1 = F.linear(c['xc'].bfloat16().double(), c['wq'].double(), b)
        assert (y1 - c['y64']).abs().max().item() >= 10 * BOUND * scale


@pytest.mark.parametrize('o', OS)
@pytest.mark.parametrize('m', MS)
def test_kernel_every_width_and_batch(o, m):
    for f, ws, clamp in ((65, 'ls-2', SYM), (800, 'gf-3', IDENT)):
        c = _case(m, f, o, ws, clamp, bias=m % 2 == 1, seed=7 * m + o)
        _check(c, _run(c))


TILED = [(1000, 65, 1033, 'gf-3'), (1024, 800, 1000, 'ls-2'), (4100, 130, 2000, 'ls-1'), (300, 1, 4100, 'ls-T')]


@pytest.mark.parametrize('i', range(len(TILED)))
def test_tiled_kernel_edges(i):
    """Shapes with at least 256 tiles of 64 x 64 (the tiled kernel, 64 x 64 and 128 x 128 tiles), ragged rows and columns."""
    m, f, o, ws = TILED[i]
    c = _case(m, f, o, ws, SYM if i % 2 else IDENT, bias=i % 2 == 0, seed=300 + i)
    _check(c, _run(c))


def test_kernel_at_the_mlp_shape():
    c = _case(8192, 4096, 4096, 'ls-2', SYM, bias=True, seed=400)
    err, scale = _check(c, _run(c))
    y1 = F.linear(c['xc'].bfloat16().double().to(DEV), c['wq'].double().to(DEV), c['bias_cpu'].double().to(DEV)).cpu()
    assert (y1 - c['y64']).abs().max().item() >= 10 * BOUND * scale


# ------------------------------------------------------------------------------------------------ output buffer, alignment
def _raw_call(c, x_ptr, y_ptr, kw=None, stream=None):
    hip = _hip()
    return hip.linear_fp_lib().lsq_linear_signw(x_ptr, c['alpha'], c['wbits'].data_ptr(), c['wsc'].shape[0] if kw is None else kw,
                                                c['wsc'].data_ptr(), None if c['b'] is None else c['b'].data_ptr(),
                                                c['m'], c['f'], c['o'], y_ptr, stream)


@pytest.mark.parametrize('shape', [(7, 65, 33, 'ls-2'), (16, 800, 1000, 'gf-3'), (1000, 65, 1033, 'ls-1'),
                                   (4100, 130, 2000, 'gf-2'), (1024, 800, 1000, 'ls-T'), (2048, 800, 2048, 'gf-3')])
def test_output_buffer_and_unaligned_input(shape):
    """y written exactly into its place inside a NaN-filled buffer; x at an address 4 bytes past 16 gives the same bits as
    the aligned x.  With F % 4 == 0 that compares the 16-byte and the 4-byte load paths: (16, 800) on the split kernel,
    (1024, 800) on 64 x 64 and (2048, 800) on 128 x 128 tiles."""
    m, f, o, ws = shape
    c = _case(m, f, o, ws, SYM, bias=True, seed=500 + m)
    pad = 37
    buf = torch.full((pad + m * o + pad,), float('nan'), device=DEV)
    assert _raw_call(c, c['x'].data_ptr(), buf.data_ptr() + 4 * pad) == 0
    torch.cuda.synchronize()
    y = buf[pad:pad + m * o].view(m, o)
    assert not torch.isnan(y).any()
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + m * o:]).all()
    _check(c, y)
    xbuf = torch.empty((m * f + 1,), device=DEV)
    xbuf[1:] = c['x'].view(-1)
    xu = xbuf[1:].view(m, f)                      # data pointer 4 bytes past a 16-byte boundary
    assert xu.data_ptr() % 16 == 4
    yu = _run(c, xu)
    assert torch.equal(yu.view(torch.int32), y.contiguous().view(torch.int32))


@pytest.mark.parametrize('shape', [(16, 4096, 4096, 'ls-2'), (1024, 800, 1000, 'gf-3')])
def test_two_calls_give_the_same_bits(shape):
    m, f, o, ws = shape
    c = _case(m, f, o, ws, IDENT, bias=True, seed=600 + m)
    y1, y2 = _run(c), _run(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y3 = _run(c)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for y in (y2, y3):
        assert torch.equal(y1.view(torch.int32), y.view(torch.int32))


def test_nine_planes_are_refused_and_write_nothing():
    c = _case(16, 128, 40, 'gf-8', SYM, bias=True, seed=700)
    y = torch.full((16, 40), 12345.0, device=DEV)
    assert _raw_call(c, c['x'].data_ptr(), y.data_ptr(), kw=9) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (y == 12345.0).all()


# ------------------------------------------------------------------------------------------------ QuantLinear('fp', w)
def _module(ws, f, o, clamp, seed, bias=True):
    from quant.binary import QuantLinear
    m = QuantLinear('fp', ws, f, o, clamp, bias=bias)
    detgen.fill_module(m, seed=seed)
    with torch.no_grad():
        for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight.view(o, f, 1, 1), ws)):
            buf.copy_(v)
    return m


def _module_oracle(m, x, clamp):
    o, f = m.out_features, m.in_features
    wq = P.quantize_weight(m.weight.detach().cpu().view(o, f, 1, 1), m.w_quant,
                           [b.cpu() for b in m.w_approximate.cached_scales()]).view(o, f)
    b = None if m.bias is None else m.bias.detach().cpu().double()
    return F.linear(P.clamp_act(x.cpu(), clamp).double(), wq.double(), b)


@pytest.fixture
def counters(monkeypatch):
    hip = _hip()
    calls = {'signw': 0, 'pack': 0}
    signw, pack = hip.linear_signw, hip.pack_weight

    def counted_signw(*a, **k):
        calls['signw'] += 1
        return signw(*a, **k)

    def counted_pack(*a, **k):
        calls['pack'] += 1
        return pack(*a, **k)

    monkeypatch.setattr(hip, 'linear_signw', counted_signw)
    monkeypatch.setattr(hip, 'pack_weight', counted_pack)
    return calls


def _close(y, ref):
    err = (y.cpu().double() - ref).abs().max().item()
    assert err <= BOUND * ref.abs().max().item(), err / ref.abs().max().item()


@pytest.mark.parametrize('ws', ('ls-1', 'ls-2', 'ls-T', 'gf-3'))
@pytest.mark.parametrize('shape', [(9, 100), (4, 3, 100), (2, 5, 7, 65)])
def test_quant_linear_eval_takes_the_kernel(ws, shape, counters):
    i = ('ls-1', 'ls-2', 'ls-T', 'gf-3').index(ws)
    clamp = SYM if i % 2 else IDENT
    f, o = shape[-1], 70
    m = _module(ws, f, o, clamp, seed=31 + i, bias=len(shape) != 3).eval().to(DEV)
    x = detgen.normal(f'qlinfp.x.{i}', shape, scale=1.3).to(DEV)
    with torch.no_grad():
        y = m(x)
    assert counters['signw'] == 1
    assert y.shape == (*shape[:-1], o)
    _close(y, _module_oracle(m, x, clamp).view(*shape[:-1], o))
    assert not hasattr(m, 'last_act_scales')


def test_quant_linear_eval_takes_strided_inputs(counters):
    """Inputs that are views with strides of their own (a CLS-token head h[:, 0], a slice of a wider tensor, a transpose)
    run the kernel and match the oracle, as the torch formulation accepted them before."""
    f, o = 100, 40
    m = _module('ls-2', f, o, SYM, seed=45).eval().to(DEV)
    h = detgen.normal('qlinfp.stride.h', (6, 5, f), scale=1.3).to(DEV)
    wide = detgen.normal('qlinfp.stride.w', (4, 3, f + 7), scale=1.3).to(DEV)
    z = detgen.normal('qlinfp.stride.z', (f, 9), scale=1.3).to(DEV)
    inputs = [h[:, 0], wide[..., :f], wide[..., 7:], z.t(), h.transpose(0, 1)]
    for i, x in enumerate(inputs):
        assert not x.is_contiguous()
        with torch.no_grad():
            y = m(x)
        assert counters['signw'] == i + 1
        assert y.shape == (*x.shape[:-1], o)
        _close(y, _module_oracle(m, x.contiguous(), SYM).view(*x.shape[:-1], o))


def test_weights_are_packed_once_per_eval_session(counters):
    m = _module('ls-2', 200, 50, SYM, seed=41).eval().to(DEV)
    x = detgen.normal('qlinfp.cache.x', (6, 200)).to(DEV)
    with torch.no_grad():
        y1, y2 = m(x), m(x)
        assert counters['pack'] == 1 and counters['signw'] == 2
        assert torch.equal(y1, y2)
        m.weight.mul_(-1.0)                       # in-place change: repacked, the output follows
        y3 = m(x)
        assert counters['pack'] == 2
        _close(y3, _module_oracle(m, x, SYM))
        assert (y3 - y1).abs().max().item() > 1e-2
        m.train()
        m.eval()
        y4 = m(x)
        assert counters['pack'] == 3
        assert torch.equal(y3, y4)


def test_paths_that_stay_on_torch(counters):
    x = detgen.normal('qlinfp.torch.x', (5, 3, 96), scale=1.2)
    cases = []
    m = _module('ls-1', 96, 20, SYM, seed=51).to(DEV)                 # train mode
    cases.append((m.train(), x.to(DEV), False))
    m = _module('ls-2', 96, 20, SYM, seed=52).eval().to(DEV)          # an input that wants a gradient
    cases.append((m, x.to(DEV).requires_grad_(True), True))
    m = _module('ls-1', 96, 20, SYM, seed=53).eval()                  # CPU
    cases.append((m, x, False))
    from quant.binary import QuantLinear
    m = QuantLinear('fp', 'fp', 96, 20, SYM)                          # fp / fp
    detgen.fill_module(m, seed=54)
    cases.append((m.eval().to(DEV), x.to(DEV), False))
    m = _module('gf-9', 96, 20, SYM, seed=55).eval().to(DEV)          # nine weight planes
    cases.append((m, x.to(DEV), False))
    for mod, xin, grad in cases:
        with torch.set_grad_enabled(grad):
            y = mod(xin)
            ref = mod._forward_torch(xin)
        assert torch.equal(y, ref)
    assert counters['signw'] == 0


def test_lenet_with_an_fp_activation_fc1_end_to_end(counters):
    """QLeNet5(fc1_quant={'x_quant': 'fp', ...}) on the GPU: fc1 runs lsq_linear_signw; fc1's output against fp64 and the
    network's output against the CPU formulation applied to the same fc1 input."""
    from quant.binary import QuantLinear
    from quant.models.lenet import QLeNet5
    fc1q = {'x_quant': 'fp', 'w_quant': 'ls-1', 'clamp': SYM}
    model = QLeNet5(loss_fn=None, x_quant='ls-2', w_quant='ls-1', clamp=SYM, fc1_quant=fc1q)
    assert isinstance(model.fc1, QuantLinear)
    detgen.fill_module(model, seed=5)
    with torch.no_grad():
        model.conv2.w_approximate.v1.copy_(P.weight_scales(model.conv2.weight, 'ls-1')[0])
        model.fc1.w_approximate.v1.copy_(P.weight_scales(model.fc1.weight.view(500, 800, 1, 1), 'ls-1')[0])
    model.eval().to(DEV)
    seen = {}
    model.fc1.register_forward_hook(lambda mod, inp, out: seen.update(x=inp[0].detach().cpu(), y=out.detach().cpu()))
    with torch.no_grad():
        logp = model(detgen.normal('qlenetfp.x', (64, 1, 28, 28)).to(DEV)).cpu()
    assert counters['signw'] == 1
    fc1 = model.fc1
    model.cpu()
    y_ref = _module_oracle(fc1, seen['x'], SYM)
    _close(seen['y'], y_ref)
    with torch.no_grad():
        ref = F.log_softmax(model.fc2(F.relu(y_ref.float())), dim=1)
    assert ((logp - ref).abs().max() / ref.abs().max()).item() <= 1e-4
