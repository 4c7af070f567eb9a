"""lsq_linear_xnor (liblsq_hip_linear.so) and QuantLinear on the GPU: bit for bit the 1x1 popcount convolution over the same
planes, exact integers at the ends of their range, QuantLinear's eval forward against the oracle, and LeNet's fc1."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detgen
from oracle import lsq_exact
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4        # |y - y_ref| <= TOL * max |y_ref| with the oracle's scales injected (bit planes exact)

# activation schemes: (LSQ_SCHEME_* code, planes)
ACT = {'ls-1': (1, 1), 'ls-2': (2, 2), 'ls-T': (3, 2), 'gf-3': (4, 3)}
WGT = ('ls-1', 'ls-2', 'ls-T', 'gf-2')
CLAMP = {'kind': 'symmetric', 'alpha': 2}


def _hip():
    from quant import _hip
    return _hip


def _operands(n, t, f, o, xs, ws, seed, bias=True):
    """Activation planes / scales of x [n, t * f] (lsq_act_quant) and weight planes of w [o, f] (lsq_pack_weight)."""
    hip = _hip()
    code, k = ACT[xs]
    x = detgen.normal(f'lin.x.{seed}', (n, t * f), scale=1.1, seed=seed).to(DEV)
    w = detgen.normal(f'lin.w.{seed}', (o, f), seed=seed)
    gx = hip.make_geom(n, t * f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    planes = torch.zeros((k * hip.act_plane_words(gx),), dtype=torch.int64, device=DEV)
    scales = torch.empty((k, n), dtype=torch.float32, device=DEV)
    hip.act_quant(x, gx, code, k, 3, 2.0, planes, scales)
    # weight plane scales [kw, O] of the scheme's shape (ls-T: two planes of one scale); their values do not matter here
    kw = 1 if ws == 'ls-1' else 2
    wsc = detgen.uniform(f'lin.ws.{seed}', (kw, o), 0.1, 1.0, seed=seed)
    if ws == 'ls-T':
        wsc[1] = wsc[0]
    wsc = wsc.to(DEV).contiguous()
    gw = hip.make_geom(n * t, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    wbits, wsum = hip.pack_weight(w.to(DEV).view(o, f, 1, 1), gw, wsc)
    b = detgen.normal(f'lin.b.{seed}', (o,), seed=seed).to(DEV) if bias else None
    return planes, scales, k, wbits, wsum.view(-1, o), wsc, b, gw


def _popcount_route(planes, scales, k, t, wbits, wsum, wsc, b, gw):
    """lsq_xnor_conv2d on the 1x1 view (M, F, 1, 1), the scales of sample m // t at row m."""
    hip = _hip()
    m, o = gw.N, gw.O
    y = torch.empty((m, o, 1, 1), dtype=torch.float32, device=DEV)
    xs = scales.repeat_interleave(t, dim=1).contiguous()
    hip.xnor_conv2d(planes, k, xs, wbits, wsum.view(-1, o, 1), wsc, b, gw, y)
    return y.view(m, o)


def _same_bits(n, t, f, o, xs, ws, seed, bias):
    hip = _hip()
    planes, scales, k, wbits, wsum, wsc, b, gw = _operands(n, t, f, o, xs, ws, seed, bias)
    y = hip.linear_xnor(planes, k, scales, t, wbits, wsum, wsc, b, n * t, f, o)
    ref = _popcount_route(planes, scales, k, t, wbits, wsum, wsc, b, gw)
    torch.cuda.synchronize()
    assert y.shape == (n * t, o)
    bad = (y.view(torch.int32) != ref.view(torch.int32)).sum().item()
    assert bad == 0, (xs, ws, n, t, f, o, bias, bad, (y - ref).abs().max().item())
    return y


FS = (1, 63, 64, 65, 800, 4096)
OS = (1, 10, 33, 1000)
NS = (1, 7, 256)


@pytest.mark.parametrize('xs', list(ACT))
@pytest.mark.parametrize('ws', WGT)
@pytest.mark.parametrize('fi', range(len(FS)))
def test_bit_identical_to_the_1x1_popcount_route(xs, ws, fi):
    f = FS[fi]
    # out-features, batch and bias rotate with the feature count: every value of each meets every scheme pair
    o, n, bias = OS[fi % len(OS)], NS[fi % len(NS)], fi % 2 == 0
    _same_bits(n, 1, f, o, xs, ws, seed=fi, bias=bias)


@pytest.mark.parametrize('o', OS)
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('bias', (True, False))
def test_bit_identical_every_width_and_batch(o, n, bias):
    _same_bits(n, 1, 800, o, 'ls-2', 'ls-1', seed=7, bias=bias)
    _same_bits(n, 1, 65, o, 'gf-3', 'gf-2', seed=8, bias=bias)


@pytest.mark.parametrize('xs,ws', [('ls-1', 'ls-1'), ('ls-2', 'ls-T'), ('gf-3', 'ls-2')])
def test_bit_identical_with_rows_per_sample(xs, ws):
    """T = 3 rows per sample ([N, 3, F] inputs): the scales of sample m // 3 at row m."""
    _same_bits(7, 3, 128, 33, xs, ws, seed=11, bias=True)
    _same_bits(5, 3, 4096, 100, xs, ws, seed=12, bias=False)


def test_bit_identical_at_the_large_shape():
    """M = 8192, F = 4096, O = 4096: the 128 x 128 tiles."""
    _same_bits(8192, 1, 4096, 4096, 'ls-2', 'ls-1', seed=13, bias=True)


def test_exact_integers_at_the_extremes():
    """F = 2^16, all activation signs +1; weight rows all +1 / all -1 -> I = +F / -F.  y is the epilogue's fp32 expression on
    +-F, bit for bit: with unit scales exactly +-F, with random scales fp32(fp32(xs * I) * ws) (no bias: the fp64 product
    of two floats is exact, so one rounding to fp32 is the fma's)."""
    hip = _hip()
    n, f, o = 7, 1 << 16, 40
    x = torch.rand((n, f), device=DEV) + 0.5
    sign = torch.where(torch.arange(o) % 2 == 0, 1.0, -1.0)
    w = (sign.view(o, 1) * (torch.rand((o, f)) + 0.5)).to(DEV)
    gx = hip.make_geom(n, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    planes = torch.zeros((hip.act_plane_words(gx),), dtype=torch.int64, device=DEV)
    scales = torch.empty((1, n), dtype=torch.float32, device=DEV)
    hip.act_quant(x, gx, 1, 1, 3, -1.0, planes, scales)
    for unit in (True, False):
        wsc = torch.ones((1, o), device=DEV) if unit else (torch.rand((1, o)) + 0.25).to(DEV)
        xs = torch.ones((1, n), device=DEV) if unit else scales
        wbits, wsum = hip.pack_weight(w.view(o, f, 1, 1), gx, wsc)
        y = hip.linear_xnor(planes, 1, xs, 1, wbits, wsum.view(1, o), wsc, None, n, f, o).cpu()
        i_exact = (sign * f).view(1, o).to(torch.float64)
        v = (xs.cpu().to(torch.float64).view(n, 1) * i_exact).to(torch.float32)            # exact product, one rounding
        want = (v.to(torch.float64) * wsc.cpu().to(torch.float64)).to(torch.float32)
        assert torch.equal(y.view(torch.int32), want.view(torch.int32)), (unit, (y - want).abs().max().item())
        if unit:
            assert torch.equal(y, (sign * f).view(1, o).expand(n, o))


def test_two_calls_give_the_same_bits():
    hip = _hip()
    planes, scales, k, wbits, wsum, wsc, b, gw = _operands(256, 1, 800, 500, 'ls-2', 'ls-2', seed=21)
    y1 = hip.linear_xnor(planes, k, scales, 1, wbits, wsum, wsc, b, 256, 800, 500)
    y2 = hip.linear_xnor(planes, k, scales, 1, wbits, wsum, wsc, b, 256, 800, 500)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))


# ------------------------------------------------------------------------------------------------ QuantLinear
def _module(xs, ws, f, o, seed, mode='off'):
    from quant.binary import QuantLinear
    m = QuantLinear(xs, ws, f, o, CLAMP, moving_average_mode=mode)
    detgen.fill_module(m, seed=seed)
    with torch.no_grad():
        for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight.view(o, f, 1, 1), ws)):
            buf.copy_(v)
    return m


def _oracle(x, m, scales):
    n, f, o = x.shape[0], m.in_features, m.out_features
    x4 = P.clamp_act(x.reshape(n, -1, 1, 1), CLAMP)
    _, xq = P.quantize_activation(x4, m.x_quant, scales=scales)
    wq = P.quantize_weight(m.weight.detach().view(o, f, 1, 1), m.w_quant, m.w_approximate.cached_scales()).view(o, f)
    return F.linear(xq.reshape(x.shape), wq, m.bias.detach())


def _nscales(xs):
    return {'ls-1': 1, 'ls-2': 2, 'ls-T': 1, 'gf-3': 3}[xs]


@pytest.mark.parametrize('xs', list(ACT))
@pytest.mark.parametrize('ws', WGT)
@pytest.mark.parametrize('shape', [(64, 800), (6, 3, 128)])
def test_quant_linear_eval_against_the_oracle(xs, ws, shape):
    f, o = shape[-1], 70
    m = _module(xs, ws, f, o, seed=31)
    x = detgen.normal('qlin.x', shape, scale=1.2)
    m.eval().to(DEV)
    with torch.no_grad():
        y = m(x.to(DEV)).cpu()
    v = m.last_act_scales.cpu()
    ref = _oracle(x, m.cpu(), [v[i] for i in range(_nscales(xs))])
    assert y.shape == ref.shape == (*shape[:-1], o)
    err = ((y - ref).abs().max() / ref.abs().max()).item()
    assert err <= TOL, err
    if xs in ('ls-2', 'ls-T'):          # free-running v1: the exact oracle's, bit for bit
        rows = P.clamp_act(x.reshape(shape[0], -1), CLAMP).numpy()
        assert np.array_equal(v[0].numpy(), lsq_exact.solve_rows(rows, xs == 'ls-T', 3)), xs


def test_quant_linear_moving_average_eval():
    m = _module('ls-2', 'ls-1', 256, 30, seed=33, mode='eval_only')
    with torch.no_grad():
        m.x_approximate.moving_avg_module.moving_average.copy_(torch.tensor([0.9, 0.35]))
    x = detgen.normal('qlin.ma.x', (9, 256))
    m.eval().to(DEV)
    with torch.no_grad():
        y = m(x.to(DEV)).cpu()
    ref = _oracle(x, m.cpu(), [torch.full((9,), 0.9), torch.full((9,), 0.35)])
    assert ((y - ref).abs().max() / ref.abs().max()).item() <= TOL


def test_quant_linear_eval_is_deterministic():
    m = _module('ls-T', 'gf-2', 800, 500, seed=35).eval().to(DEV)
    x = detgen.normal('qlin.det.x', (64, 800)).to(DEV)
    with torch.no_grad():
        y1, y2 = m(x), m(x)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))


def test_lenet_with_a_binary_fc1_end_to_end():
    """QLeNet5(fc1_quant=...) on the GPU: fc1 runs lsq_linear_xnor; the network's output equals the CPU formulation applied
    to the same fc1 input with fc1's GPU scales (the layers in front of it are checked by the existing suite)."""
    from quant.binary import QuantLinear
    from quant.models.lenet import QLeNet5
    fc1q = {'x_quant': 'ls-2', 'w_quant': 'ls-1', 'clamp': CLAMP}
    model = QLeNet5(loss_fn=None, x_quant='ls-2', w_quant='ls-1', clamp=CLAMP, fc1_quant=fc1q)
    assert isinstance(model.fc1, QuantLinear)
    detgen.fill_module(model, seed=5)
    with torch.no_grad():
        model.conv2.w_approximate.v1.copy_(P.weight_scales(model.conv2.weight, 'ls-1')[0])
        model.fc1.w_approximate.v1.copy_(P.weight_scales(model.fc1.weight.view(500, 800, 1, 1), 'ls-1')[0])
    model.eval().to(DEV)
    seen = {}
    model.fc1.register_forward_hook(lambda mod, inp, out: seen.update(x=inp[0].detach().cpu(), y=out.detach().cpu()))
    with torch.no_grad():
        logp = model(detgen.normal('qlenet.x', (64, 1, 28, 28)).to(DEV)).cpu()
    fc1 = model.fc1
    v = fc1.last_act_scales.cpu()
    model.cpu()
    y_ref = _oracle(seen['x'], fc1, [v[0], v[1]])
    assert ((seen['y'] - y_ref).abs().max() / y_ref.abs().max()).item() <= TOL
    with torch.no_grad():
        ref = F.log_softmax(model.fc2(F.relu(y_ref)), dim=1)
    assert ((logp - ref).abs().max() / ref.abs().max()).item() <= TOL


# ------------------------------------------------------------------------------------------------ shared workspaces
def _act_entries(m):
    return [kk for kk in m._hip_cache if isinstance(kk, tuple) and kk[0] == 'act']


@pytest.mark.parametrize('kind', ('conv', 'linear'))
def test_workspace_eviction_keeps_every_batch_size_right(kind):
    """Batch sizes 1..6 and 1 again through one eval-mode module: at most four plane workspaces are kept, and every output
    has the bits of a fresh copy of the module (a workspace of another shape handed back, or an evicted one still in use,
    would change them)."""
    from quant.binary import QuantLinear
    from quant.binary.binary_conv import QuantConv2d

    def make():
        if kind == 'conv':
            return QuantConv2d('ls-2', 'ls-1', 64, 64, 3, CLAMP, padding=1), (64, 8, 8)
        return QuantLinear('ls-2', 'ls-1', 128, 32, CLAMP), (128,)

    m, row = make()
    detgen.fill_module(m, seed=41)
    with torch.no_grad():
        m.w_approximate.v1.copy_(m.weight.abs().flatten(1).mean(1))       # (any positive scales do: the copies load the same state)
    state = m.state_dict()
    m.eval().to(DEV)
    for step, n in enumerate((1, 2, 3, 4, 5, 6, 1)):
        x = detgen.normal(f'evict.{kind}.{step}', (n, *row), scale=1.2).to(DEV)
        fresh = make()[0]
        fresh.load_state_dict(state)
        fresh.eval().to(DEV)
        with torch.no_grad():
            y, ref = m(x), fresh(x)
        assert 'w' in m._hip_cache and len(_act_entries(fresh)) == 1                 # both ran on the kernels
        assert torch.equal(y.view(torch.int32), ref.view(torch.int32)), (kind, step, n)
        assert len(_act_entries(m)) == min(step + 1, 4), (kind, step)


def test_two_streams_through_one_quant_linear():
    """One QuantLinear on two streams with different inputs, nothing between the launches: each stream has its own plane
    workspace, and the results have the bits of the same calls on one stream."""
    m = _module('ls-2', 'ls-1', 128, 32, seed=43).eval().to(DEV)
    xa = detgen.normal('qlin.streams.a', (5, 128), scale=1.2).to(DEV)
    xb = detgen.normal('qlin.streams.b', (5, 128), scale=0.7).to(DEV)
    with torch.no_grad():
        ya, yb = m(xa), m(xb)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for kk in _act_entries(m):                 # (the packed weights stay: they were written on the stream that has just been waited for)
        del m._hip_cache[kk]
    with torch.no_grad():
        with torch.cuda.stream(s1):
            y1 = m(xa)
        with torch.cuda.stream(s2):
            y2 = m(xb)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int32), ya.view(torch.int32)) and torch.equal(y2.view(torch.int32), yb.view(torch.int32))
    keys = _act_entries(m)
    assert len(keys) == 2 and {kk[-1] for kk in keys} == {s1.cuda_stream, s2.cuda_stream}
    (p1, v1), (p2, v2) = (m._hip_cache[kk] for kk in keys)
    assert p1.data_ptr() != p2.data_ptr() and v1.data_ptr() != v2.data_ptr()
