"""lsq_weight_quant_pack (include/lsq_hip_weight_train.h): the scales against the solver, the exact oracle and fp64 closed forms,
the planes and tap sums against lsq_pack_weight, the refusals, and the train steps of the modules with
``hip_train_common.WEIGHT_KERNEL`` on.

Bound of the mean-type scales (derived, not measured): the terms |r_q| are fp32 values the test recomputes bit for bit (the
fp32 recurrence of the header); an fp64 sum of at most 16384 of them is within 16384 * 2^-53 < 2e-12 relative of exact
whatever its order, so rounding it once to fp32 gives the correctly rounded mean or its neighbour: 1 ulp."""

import copy
import ctypes

import numpy as np
import pytest
import torch

import train_step_cases as T
from oracle import lsq_exact as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MAX_ROW = 16384
# (O, C, KH, KW, groups)
GEOMS = [(20, 70, 3, 3, 1), (32, 32, 3, 3, 2), (24, 200, 1, 1, 1), (16, 64, 4, 4, 1), (16, 2, 1, 1, 1),
         (16, MAX_ROW, 1, 1, 1), (8, 512, 3, 3, 1)]
# (scheme, LSQ_SCHEME_*, k, skips)
SCHEMES = [('ls-1', 1, 1, (3,)), ('ls-2', 2, 2, (1, 3)), ('ls-T', 3, 2, (1, 3)), ('gf-2', 4, 2, (3,)), ('gf-8', 4, 8, (3,))]
HARD_ROWS = 5
BOUND_GX, BOUND_GW, BOUND_Y = 1e-5, 1e-5, 1e-5      # BOUND_GX / BOUND_GW_MIOPEN / BOUND_Y of tests/test_gpu_train_geometries.py


def _hip():
    from quant import _hip
    return _hip


def _geom(o, c, kh, kw, groups):
    return _hip().make_geom(1, c, kh, kw, o, kh, kw, (1, 1), (0, 0), (1, 1), groups)


def _weight(o, c, kh, kw, groups):
    """Gaussian rows (seed fixed); the first five are the hard rows: zeros with a -0.0, all equal, small integers (costs
    that tie exactly), one outlier of 1e4, and a ternary row whose minimum exceeds half its mean."""
    gen = torch.Generator().manual_seed(1234)
    m = (c // groups) * kh * kw
    w = torch.randn((o, m), generator=gen) * 0.05
    sign = torch.where(torch.arange(m) % 3 == 0, -1.0, 1.0)
    w[0] = 0.0
    w[0, 1] = -0.0
    w[1] = 0.37 * sign
    w[2] = (torch.arange(m) % 5 - 2).float()
    w[3, m // 2] = 1e4
    w[4] = (1.0 + 0.5 * torch.rand(m, generator=gen)) * sign
    return w.view(o, c // groups, kh, kw)


@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('scheme,sid,k,skip', [(s, i, k, sk) for s, i, k, sks in SCHEMES for sk in sks],
                         ids=lambda v: str(v))
def test_kernel_against_the_references(geom, scheme, sid, k, skip):
    hip = _hip()
    g = _geom(*geom)
    o = geom[0]
    w_cpu = _weight(*geom)
    rows = w_cpu.view(o, -1)
    m = rows.shape[1]
    w = w_cpu.to(DEV)
    assert hip.weight_quant_pack_supported(g, sid, k, skip)
    scales, wbits, wsum = hip.weight_quant_pack(w, g, sid, k, skip)
    again = hip.weight_quant_pack(w, g, sid, k, skip)
    assert all(torch.equal(a, b) for a, b in zip((scales, wbits, wsum), again))               # repeatable
    got = scales.cpu()
    assert tuple(got.shape) == (k, o)

    first_mean = 0
    if scheme in ('ls-2', 'ls-T'):
        ternary = scheme == 'ls-T'
        v12, _ = hip.solve_rows(w.view(o, m), skip, ternary)
        assert torch.equal(got[0], v12[0].cpu()), (got[0], v12[0])
        for r in range(HARD_ROWS, o):                      # input condition: the oracle's two best costs are apart
            d = {}
            want = E.solve_row(rows[r].numpy(), ternary, skip, d)
            cost = sorted(d['cost_sq'])
            assert len(cost) < 2 or cost[1] - cost[0] > 1e-9 * abs(cost[0]), (r, cost[:2])
            assert got[0, r].numpy() == want, (r, got[0, r], want)
        if m == 2 and not ternary:
            assert not bool(got[0].any())                   # fewer than three keys, no extra candidate: v1 = 0
        first_mean = 1
        if ternary:
            assert torch.equal(got[1], got[0])
            first_mean = 2
    resid = rows.clone()
    for q in range(k):
        if q >= first_mean:
            want = (resid.abs().double().sum(1) / m).float()
            ulp = torch.from_numpy(np.spacing(want.numpy()))
            assert bool(((got[q] - want).abs() <= ulp).all()), (q, got[q], want)
        resid = resid - got[q].view(-1, 1) * torch.where(resid >= 0, 1.0, -1.0)               # fp32, sign(+-0) = +1

    pbits, psum = hip.pack_weight(w, g, scales)
    assert torch.equal(wbits, pbits) and torch.equal(wsum, psum)


def test_graph_replays_equal_the_eager_call():
    hip = _hip()
    geom = GEOMS[0]
    g, w = _geom(*geom), _weight(*geom).to(DEV)
    eager = hip.weight_quant_pack(w, g, 2, 2, 3)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = hip.weight_quant_pack(w, g, 2, 2, 3)
    for _ in range(3):
        for t in captured:
            t.fill_(-1)
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(captured, eager))


def test_refusals_through_the_c_abi():
    hip = _hip()
    lib = hip.weight_train_lib()
    buf = torch.zeros(64, dtype=torch.int64, device=DEV)
    p, small, long_row = buf.data_ptr(), _geom(16, 2, 1, 1, 1), _geom(16, MAX_ROW + 1, 1, 1, 1)

    def call(g, sid, k, out=p):
        return lib.lsq_weight_quant_pack(p, ctypes.byref(g), sid, k, 3, out, p, p, None)

    assert hip.WEIGHT_TRAIN_MAX_ROW == MAX_ROW
    assert lib.lsq_weight_quant_pack_supported(ctypes.byref(long_row), 1, 1, 3) == 0
    assert call(long_row, 1, 1) == hip.E_UNSUPPORTED
    assert call(small, 4, 0) == call(small, 4, 9) == call(small, 7, 1) == -3      # LSQ_E_SCHEME
    assert call(small, 1, 1, None) == -1                                           # LSQ_E_NULL
    torch.cuda.synchronize()
    assert not bool(buf.any())                                                     # a refused call writes nothing


@pytest.mark.parametrize('kind', ['conv', 'linear'])
@pytest.mark.parametrize('ws', ['ls-1', 'ls-2', 'ls-T', 'gf-2'])
def test_train_step_with_the_weight_kernel(monkeypatch, kind, ws):
    from quant.binary import hip_train_common
    from quant.binary.binary_conv import QuantConv2d
    from quant.binary.binary_linear import QuantLinear
    hip = _hip()
    torch.manual_seed(7)
    if kind == 'conv':
        mod, x, g = QuantConv2d('ls-2', ws, 64, 64, 3, padding=1), torch.randn(4, 64, 8, 8), _geom(64, 64, 3, 3, 1)
    else:
        mod, x, g = QuantLinear('ls-2', ws, 128, 64), torch.randn(8, 128), _geom(64, 128, 1, 1, 1)
    mod.hip_train = True
    off, on = mod.to(DEV).train(), copy.deepcopy(mod).to(DEV).train()
    orig, calls = hip.weight_quant_pack, []

    def spy(*args):
        calls.append(args)
        return orig(*args)

    monkeypatch.setattr(hip, 'weight_quant_pack', spy)
    out = {}
    for name, m_, flag in (('off', off, False), ('on', on, True)):
        monkeypatch.setattr(hip_train_common, 'WEIGHT_KERNEL', flag)
        xd = x.to(DEV).requires_grad_()
        y = m_(xd)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
        y.backward(gy)
        out[name] = (y.detach(), xd.grad, m_.weight.grad, m_.w_approximate.plane_scales().detach().clone(),
                     m_.last_act_scales.detach().clone())
    assert len(calls) == 1

    wq = on.w_approximate
    scales, _, _ = orig(on.weight.detach().view(g.O, -1, g.KH, g.KW).contiguous(), g, wq.hip_scheme, wq.n_planes, 3)
    for i, buf in enumerate(wq.cached_scales()):
        assert torch.equal(buf, scales[i])
    assert torch.equal(out['on'][3], scales)
    with torch.no_grad():
        assert torch.equal(on.eval()(x.to(DEV)), out['on'][0])             # eval packs the stored buffers the old way
    if ws in ('ls-2', 'ls-T'):
        assert torch.equal(out['on'][3][0], out['off'][3][0])

    if torch.equal(out['on'][3], out['off'][3]):
        print(f'\n{kind} {ws}: weight scales bit-equal to the torch route')
        assert torch.equal(out['on'][1], out['off'][1]) and torch.equal(out['on'][2], out['off'][2])
        return
    x4, w4 = x.view(x.shape[0], -1, *x.shape[2:], *(1,) * (4 - x.dim())), mod.weight.detach().cpu().view(g.O, -1, g.KH, g.KW)
    for name in ('off', 'on'):                                             # each route against fp64 with its own scales
        y, gx, gw, wsc, xsc = (t.cpu() for t in out[name])
        ref = T.step64(x4, w4, mod.bias, gy.view(y.shape[0], g.O, *y.shape[2:], *(1,) * (4 - y.dim())).cpu(), list(xsc),
                       list(wsc), mod._alpha(), 1, (g.KH // 2, g.KW // 2))
        assert float((y.double().view_as(ref['y']) - ref['y']).abs().max()) <= BOUND_Y * float(ref['y'].abs().max())
        err_x = (gx.double().view_as(ref['gx']) - ref['gx']).abs()
        assert bool((err_x <= BOUND_GX * ref['m_x'].abs() * ref['mag_x'] + 1e-30).all()), name
        err_w = (gw.double().view_as(ref['gw']) - ref['gw']).abs()
        assert float(err_w.max()) <= BOUND_GW * float(ref['gw'].abs().max()), name

