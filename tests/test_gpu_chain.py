"""lsq_xnor_conv2d_chain tested directly (include/lsq_hip.h; csrc/lsq_xnor_mfma.hip, the CHAIN instantiations): the plane the
epilogue writes for the next layer, its exact row sums and the consumer's scale rebuilt from them, against the CPU model of
tests/golden/chain_cases.py and against lsq_act_quant / lsq_xnor_conv2d, at clamps whose unit exponents differ (every other
convolution test clamps at 2 or 3: one unit), on tiles that span up to eight samples, with 1-3 weight planes, every fused
epilogue, with and without a folded batch norm, sentinel-filled halos and preseeded sums; the 2^22 row limit; every refusal
of the entry point on real, sentinel-filled buffers; and the module's fall-backs on a two-layer harness.

Bars: bits, plane words, integer row sums and scales rebuilt from them are EQUAL; y against the fp64 convolution of the sign
tensors within TOL = 1e-4 of max |y| and a scale against the fp64 mean within 1e-6 relative (tests/test_gpu_parity.py).
Non-finite activations are out of scope: the clamp maps a NaN differently in the two kernels and no caller produces one.
Every call goes through quant._hip."""

import functools
import types

import numpy as np
import pytest
import torch

import chain_cases as CC
import detgen

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOL = 1e-4
SENT_WORD = 0x5A5AA5A55A5AA5A5           # what plane buffers are prefilled with: the halo must still hold it
SENT_Y = 12345.0
CASE_IDS = [c.id for c in CC.CASES]


def _hip():
    from quant import _hip
    return _hip


def _seeds(n):
    """What sum_units holds on entry: the sums are ADDED."""
    return torch.arange(1, n + 1, dtype=torch.int64, device=DEV) * 1000003


def _quantize(x, geom, alpha, pre=None):
    """lsq_act_quant(LS1) -> (plane words, zero halo; scales [1, N])."""
    hip = _hip()
    planes = torch.zeros((hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    scales = torch.empty((1, geom.N), dtype=torch.float32, device=DEV)
    hip.act_quant(x, geom, hip.SCHEME_LS1, 1, 3, alpha, planes, scales, None, pre)
    return planes, scales


def _consumer_geom(n, c, h, w, pad, o=64, stride=(1, 1), dil=(1, 1)):
    return _hip().make_geom(n, c, h, w, o, 3, 3, stride, pad, dil, 1)


@functools.lru_cache(maxsize=None)
def _prepared(cid):
    """Device inputs of a case: the producer's own input planes and scales (lsq_act_quant) and packed weights."""
    hip = _hip()
    c = CC.BY_ID[cid]
    d = {k: (None if v is None else v.to(DEV)) for k, v in CC.inputs(cid).items()}
    geom = hip.make_geom(c.N, c.C, c.H, c.W, c.O, 3, 3, c.stride, c.pad, c.dil, 1)
    assert hip.out_hw(geom) == (c.Ho, c.Wo)
    planes, xscales = _quantize(d['x'], geom, CC.ALPHA_IN)
    wbits, wsum = hip.pack_weight(d['w'], geom, d['wscales'])
    return geom, d, planes, xscales, wbits, wsum


def _epi(c, d):
    return dict(relu=c.act == 'relu', res_pre=d['res_pre'], res_post=d['res_post'], prelu=d['slope'])


def _plain(cid, popcount):
    hip = _hip()
    c = CC.BY_ID[cid]
    geom, d, planes, xscales, wbits, wsum = _prepared(cid)
    y = torch.full((c.N, c.O, c.Ho, c.Wo), SENT_Y, dtype=torch.float32, device=DEV)
    with hip.debug_switches(xnor_popcount=popcount):
        hip.xnor_conv2d(planes, 1, xscales, wbits, wsum, d['wscales'], d['bias'], geom, y, **_epi(c, d))
    return y


def _next_buffers(n, o, ho, wo, pad, fill=SENT_WORD):
    words = n * ((o + 63) // 64) * (ho + 2 * pad[0]) * (wo + 2 * pad[1])
    return torch.full((words,), fill, dtype=torch.int64, device=DEV)


def _chained(cid):
    """The producer launch into sentinel-filled plane words and preseeded sums -> (y, plane words, sums)."""
    hip = _hip()
    c = CC.BY_ID[cid]
    geom, d, planes, xscales, wbits, wsum = _prepared(cid)
    y = torch.full((c.N, c.O, c.Ho, c.Wo), SENT_Y, dtype=torch.float32, device=DEV)
    nplanes = _next_buffers(c.N, c.O, c.Ho, c.Wo, c.next_pad)
    units = _seeds(c.N)
    nxt = hip.NextLs1(nplanes.data_ptr(), units.data_ptr(), hip.ptr(d['s']), hip.ptr(d['t']), c.alpha, *c.next_pad)
    assert hip.xnor_conv2d_chain(planes, xscales, None, 0.0, wbits, wsum, d['wscales'], d['bias'], geom, y, nxt=nxt, **_epi(c, d))
    return y, nplanes, units


def _words(t, n, o, ho, wo, pad):
    return t.cpu().numpy().view(np.uint64).reshape(n, (o + 63) // 64, ho + 2 * pad[0], wo + 2 * pad[1])


def _split(words, ho, wo, pad):
    """(interior, halo words as a flat array)."""
    mask = np.zeros(words.shape, dtype=bool)
    mask[:, :, pad[0]:pad[0] + ho, pad[1]:pad[1] + wo] = True
    return words[:, :, pad[0]:pad[0] + ho, pad[1]:pad[1] + wo], words[~mask]


def _check_producer(c, d, y, nplanes, units, tag):
    """(ii)-(iv) of one producer launch: the plane against the CPU model of the GPU's own y and against lsq_act_quant's, the
    halo, the sums.  Prints its tallies before it asserts."""
    hip = _hip()
    torch.cuda.synchronize()
    s, t = (None, None) if d['s'] is None else (d['s'].cpu().numpy(), d['t'].cpu().numpy())
    y_np = y.cpu().numpy()
    words = _words(nplanes, c.N, c.O, c.Ho, c.Wo, c.next_pad)
    interior, halo = _split(words, c.Ho, c.Wo, c.next_pad)
    model = CC.model_words(CC.model_bits(y_np, s, t, c.alpha), c.next_pad)
    model_interior, _ = _split(model, c.Ho, c.Wo, c.next_pad)
    g2 = hip.make_geom(c.N, c.O, c.Ho, c.Wo, 64, 1, 1, (1, 1), c.next_pad, (1, 1), 1)     # (the layout needs no kernel size)
    qplanes, qscales = _quantize(y, g2, c.alpha, None if d['s'] is None else (d['s'], d['t']))
    torch.cuda.synchronize()
    qwords = _words(qplanes, c.N, c.O, c.Ho, c.Wo, c.next_pad)
    got = (units - _seeds(c.N)).cpu().numpy()
    scale = CC.model_scale(got, c.alpha, c.M)
    mean = CC.mean64(y_np, s, t, c.alpha)
    rel = float(np.max(np.abs(scale.astype(np.float64) - mean) / mean))
    want = CC.model_units(y_np, c.alpha) if s is None else None
    print(f'CHAIN-TALLY {tag} alpha={c.alpha} words={interior.size} words_differ_model={int((interior != model_interior).sum())} '
          f'words_differ_act_quant={int((interior != _split(qwords, c.Ho, c.Wo, c.next_pad)[0]).sum())} totals={c.N} '
          f'totals_differ={"n/a" if want is None else int((got != want).sum())} '
          f'scales_differ_act_quant={int((scale != qscales[0].cpu().numpy()).sum())} scale_rel_to_mean={rel:.3e}')
    assert np.array_equal(interior, model_interior), tag                       # (ii)
    assert halo.size == words.size - interior.size and np.all(halo == np.uint64(SENT_WORD)), tag
    assert np.array_equal(qwords, model), tag                                   # (iii): word for word, and its halo is zero
    if want is not None:
        assert np.array_equal(got, want), (tag, got, want)                      # (iv) exact integers
    assert np.array_equal(scale, qscales[0].cpu().numpy()), (tag, scale, qscales)
    assert rel <= 1e-6, (tag, rel)


@pytest.mark.parametrize('cid', CASE_IDS)
def test_producer(cid):
    c = CC.BY_ID[cid]
    geom, d, planes, xscales, wbits, wsum = _prepared(cid)
    y, nplanes, units = _chained(cid)
    # (i) the CHAIN instantiation's y: the plain kernel's, the popcount kernel's, and the fp64 convolution of the sign tensors
    assert torch.equal(y, _plain(cid, False)) and torch.equal(y, _plain(cid, True)), cid
    ref = CC.reference(cid)
    err = float((y.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f'CHAIN-Y {cid} rel_err={err:.3e}')
    assert err <= TOL, (cid, err)
    _check_producer(c, d, y, nplanes, units, cid)
    # (v) again on a side stream into fresh buffers: the atomics arrive in another order, the totals are the same
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y2, nplanes2, units2 = _chained(cid)
    side.synchronize()
    assert torch.equal(y2, y) and torch.equal(nplanes2, nplanes) and torch.equal(units2, units), cid


@pytest.mark.parametrize('cid', [c.id for c in CC.CASES if c.wplanes > 1])
def test_units_are_added_on_the_final_weight_plane_pass_only(cid):
    """2 and 3 weight planes: the launch makes one pass per plane and accumulates y; the epilogue's quantizer must see the
    accumulated y and run once.  One pass less gives another y, so the plane and sums belong to the last pass."""
    hip = _hip()
    c = CC.BY_ID[cid]
    geom, d, planes, xscales, wbits, wsum = _prepared(cid)
    y, nplanes, units = _chained(cid)
    torch.cuda.synchronize()
    got = (units - _seeds(c.N)).cpu().numpy()
    if d['s'] is None:
        assert np.array_equal(got, CC.model_units(y.cpu().numpy(), c.alpha))   # once: twice would be about double
    # the same launch with the first plane only: different y, different sums -- the sums follow the accumulated y
    y1 = torch.full_like(y, SENT_Y)
    nplanes1 = _next_buffers(c.N, c.O, c.Ho, c.Wo, c.next_pad)
    units1 = _seeds(c.N)
    nxt = hip.NextLs1(nplanes1.data_ptr(), units1.data_ptr(), hip.ptr(d['s']), hip.ptr(d['t']), c.alpha, *c.next_pad)
    assert hip.xnor_conv2d_chain(planes, xscales, None, 0.0, wbits, wsum, d['wscales'][:1].contiguous(), d['bias'], geom, y1, nxt=nxt,
                                 **_epi(c, d))
    torch.cuda.synchronize()
    assert not torch.equal(y1, y)
    s, t = (None, None) if d['s'] is None else (d['s'].cpu().numpy(), d['t'].cpu().numpy())
    scale = CC.model_scale(got, c.alpha, c.M)
    mean = CC.mean64(y.cpu().numpy(), s, t, c.alpha)
    assert np.all(np.abs(scale.astype(np.float64) - mean) <= 1e-6 * mean), (cid, scale, mean)
    words = _split(_words(nplanes, c.N, c.O, c.Ho, c.Wo, c.next_pad), c.Ho, c.Wo, c.next_pad)[0]
    model = CC.model_words(CC.model_bits(y.cpu().numpy(), s, t, c.alpha), (0, 0))
    assert np.array_equal(words, model), cid


# --------------------------------------------------------------------------------------------------------- the consumer
def _layer(tag, n, cin, cout, h, w, std):
    """A 3 x 3, stride 1, pad 1 layer from cin to cout channels whose output has a standard deviation of about ``std``:
    (geom, weights packed, wscales)."""
    hip = _hip()
    geom = hip.make_geom(n, cin, h, w, cout, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    ws = (detgen.uniform(tag + '.ws', (cout,), 0.8, 1.2) * (std / (CC.XS_NOMINAL * (cin * 6.0) ** 0.5))).view(1, -1).contiguous().to(DEV)
    w = detgen.normal(tag + '.w', (cout, cin, 3, 3)).to(DEV)
    wbits, wsum = hip.pack_weight(w, geom, ws)
    return geom, wbits, wsum, ws


def _affine(tag, ch, alpha):
    s = detgen.uniform(tag + '.s', (ch,), 0.8, 1.2) * (0.8 * alpha)
    s[::2] *= -1.0
    return s.to(DEV), detgen.normal(tag + '.t', (ch,), scale=0.1 * alpha).to(DEV)


@pytest.mark.parametrize('alpha', CC.ALPHAS)
@pytest.mark.parametrize('gid,ch', [('a', 64), ('c', 128), ('d', 256), ('f', 512)])
def test_consumer_scale_from_the_row_sums(gid, ch, alpha):
    """Two chained launches against the three unchained ones: the consumer (geometry of case a / c / d / f, 64-512 channels)
    takes its scale from the integers a producer left, and gives the y of the plain call on lsq_act_quant's scale."""
    hip = _hip()
    n, h, w, stride, pad, dil = CC.GEOMS[gid]
    affine = ch in (128, 512)
    tag = f'chain.cons.{gid}.{alpha}'
    x = detgen.normal(tag + '.x', (n, 64, h, w)).to(DEV)
    g1, wbits1, wsum1, ws1 = _layer(tag + '.l1', n, 64, ch, h, w, 1.0 if affine else 0.8 * alpha)
    planes0, scales0 = _quantize(x, g1, CC.ALPHA_IN)
    pre = _affine(tag, ch, alpha) if affine else None
    g2 = _consumer_geom(n, ch, h, w, pad, 64, stride, dil)
    w2 = detgen.normal(tag + '.w2', (64, ch, 3, 3)).to(DEV)
    ws2 = detgen.uniform(tag + '.ws2', (1, 64), 0.01, 0.02).to(DEV)
    wbits2, wsum2 = hip.pack_weight(w2, g2, ws2)
    ho, wo = hip.out_hw(g2)
    # chained: two launches (zero halo and zeroed sums, as the module provides them)
    nplanes = _next_buffers(n, ch, h, w, pad, fill=0)
    units = torch.zeros((n,), dtype=torch.int64, device=DEV)
    nxt = hip.NextLs1(nplanes.data_ptr(), units.data_ptr(), None if pre is None else pre[0].data_ptr(),
                      None if pre is None else pre[1].data_ptr(), alpha, *pad)
    y1 = torch.full((n, ch, h, w), SENT_Y, dtype=torch.float32, device=DEV)
    assert hip.xnor_conv2d_chain(planes0, scales0, None, 0.0, wbits1, wsum1, ws1, None, g1, y1, relu=not affine, nxt=nxt)
    y2 = torch.full((n, 64, ho, wo), SENT_Y, dtype=torch.float32, device=DEV)
    assert hip.xnor_conv2d_chain(nplanes, None, units, alpha, wbits2, wsum2, ws2, None, g2, y2)
    # unchained: three launches
    y1p = torch.full_like(y1, SENT_Y)
    hip.xnor_conv2d(planes0, 1, scales0, wbits1, wsum1, ws1, None, g1, y1p, relu=not affine)
    planes1, scales1 = _quantize(y1p, g2, alpha, pre)
    y2p = torch.full_like(y2, SENT_Y)
    hip.xnor_conv2d(planes1, 1, scales1, wbits2, wsum2, ws2, None, g2, y2p)
    torch.cuda.synchronize()
    rebuilt = CC.model_scale(units.cpu().numpy(), alpha, ch * h * w)
    print(f'CHAIN-CONSUMER {gid}{ch} alpha={alpha} words={nplanes.numel()} words_differ={int((nplanes != planes1).sum())} totals={n} '
          f'scales_differ={int((rebuilt != scales1[0].cpu().numpy()).sum())} y_differ={int((y2 != y2p).sum())}')
    assert torch.equal(y1, y1p)
    assert torch.equal(nplanes, planes1)                                        # halo included: zero on both sides
    assert np.array_equal(rebuilt, scales1[0].cpu().numpy()), (rebuilt, scales1)
    assert torch.equal(y2, y2p), float((y2 - y2p).abs().max())
    assert float(y2.abs().max()) > 0 and not bool((y2 == SENT_Y).any())


@pytest.mark.parametrize('alpha', (0.37, 1.0, 300.0))
def test_a_middle_layer_takes_its_scale_and_leaves_the_next_one(alpha):
    """Three layers in three launches (the middle one with x_units AND next) against the five unchained launches."""
    hip = _hip()
    n, h, w = 5, 6, 5                                     # 30 px per sample: every tile holds parts of two samples
    tag = f'chain.mid.{alpha}'
    x = detgen.normal(tag + '.x', (n, 128, h, w)).to(DEV)
    layers = [_layer(f'{tag}.l{i}', n, cin, cout, h, w, 0.8 * alpha) for i, (cin, cout) in enumerate(((128, 64), (64, 256), (256, 64)))]
    planes0, scales0 = _quantize(x, layers[0][0], CC.ALPHA_IN)
    ys, buffers = [], []
    planes_in, scales_in, units_in = planes0, scales0, None
    for i, (geom, wbits, wsum, ws) in enumerate(layers):
        y = torch.full((n, geom.O, h, w), SENT_Y, dtype=torch.float32, device=DEV)
        nxt = None
        if i < 2:
            nplanes, units = _next_buffers(n, geom.O, h, w, (1, 1), fill=0), torch.zeros((n,), dtype=torch.int64, device=DEV)
            nxt = hip.NextLs1(nplanes.data_ptr(), units.data_ptr(), None, None, alpha, 1, 1)
            buffers.append((nplanes, units))
        assert hip.xnor_conv2d_chain(planes_in, scales_in, units_in, alpha, wbits, wsum, ws, None, geom, y, relu=i == 0, nxt=nxt)
        ys.append(y)
        if i < 2:
            planes_in, scales_in, units_in = nplanes, None, units
    planes_in, scales_in = planes0, scales0
    for i, (geom, wbits, wsum, ws) in enumerate(layers):
        y = torch.full_like(ys[i], SENT_Y)
        hip.xnor_conv2d(planes_in, 1, scales_in, wbits, wsum, ws, None, geom, y, relu=i == 0)
        torch.cuda.synchronize()
        assert torch.equal(y, ys[i]), (i, float((y - ys[i]).abs().max()))
        if i < 2:
            planes_in, scales_in = _quantize(y, layers[i + 1][0], alpha)
            torch.cuda.synchronize()
            assert torch.equal(planes_in, buffers[i][0]), i
            assert np.array_equal(CC.model_scale(buffers[i][1].cpu().numpy(), alpha, geom.O * h * w), scales_in[0].cpu().numpy()), i
            assert np.array_equal(buffers[i][1].cpu().numpy(), CC.model_units(y.cpu().numpy(), alpha)), i


# --------------------------------------------------------------------------------------------------------- the row limit
def _big(hw, alpha=1.3):
    hip = _hip()
    tag = f'chain.big.{hw}'
    x = detgen.normal(tag + '.x', (1, 64, hw, hw)).to(DEV)
    geom, wbits, wsum, ws = _layer(tag, 1, 64, 64, hw, hw, 0.8 * alpha)
    planes, scales = _quantize(x, geom, CC.ALPHA_IN)
    return geom, wbits, wsum, ws, planes, scales


def test_a_consumer_row_of_exactly_2_22_elements_is_chained():
    hip = _hip()
    alpha, hw = 1.3, 256
    geom, wbits, wsum, ws, planes, scales = _big(hw)
    assert geom.O * hw * hw == 1 << 22
    y = torch.full((1, 64, hw, hw), SENT_Y, dtype=torch.float32, device=DEV)
    nplanes, units = _next_buffers(1, 64, hw, hw, (1, 1)), _seeds(1)
    nxt = hip.NextLs1(nplanes.data_ptr(), units.data_ptr(), None, None, alpha, 1, 1)
    assert hip.xnor_conv2d_chain(planes, scales, None, 0.0, wbits, wsum, ws, None, geom, y, relu=True, nxt=nxt)
    c = CC.Case('big256', 'f', 64, 64, (1, 1), 1, 'relu', alpha, False, False)
    c.N, c.Ho, c.Wo, c.M = 1, hw, hw, 1 << 22
    _check_producer(c, {'s': None, 't': None}, y, nplanes, units, 'row=2^22')
    # and the consumer side accepts a row of exactly 2^22
    y2 = torch.full((1, 64, hw, hw), SENT_Y, dtype=torch.float32, device=DEV)
    zeroed = _next_buffers(1, 64, hw, hw, (1, 1), fill=0)
    zeroed.view(1, 1, hw + 2, hw + 2)[:, :, 1:-1, 1:-1] = nplanes.view(1, 1, hw + 2, hw + 2)[:, :, 1:-1, 1:-1]
    seedless = units - _seeds(1)
    assert hip.xnor_conv2d_chain(zeroed, None, seedless, alpha, wbits, wsum, ws, None, geom, y2)
    planes1, scales1 = _quantize(y, geom, alpha)
    y2p = torch.full_like(y2, SENT_Y)
    hip.xnor_conv2d(planes1, 1, scales1, wbits, wsum, ws, None, geom, y2p)
    torch.cuda.synchronize()
    assert torch.equal(y2, y2p)


def test_a_consumer_row_above_2_22_elements_is_refused_and_nothing_is_written():
    hip = _hip()
    alpha, hw = 1.3, 260
    geom, wbits, wsum, ws, planes, scales = _big(hw)
    y = torch.full((1, 64, hw, hw), SENT_Y, dtype=torch.float32, device=DEV)
    nplanes, units = _next_buffers(1, 64, hw, hw, (1, 1)), _seeds(1)
    nxt = hip.NextLs1(nplanes.data_ptr(), units.data_ptr(), None, None, alpha, 1, 1)
    assert hip.xnor_conv2d_chain(planes, scales, None, 0.0, wbits, wsum, ws, None, geom, y, relu=True, nxt=nxt) is False
    assert hip.xnor_conv2d_chain(planes, None, units, alpha, wbits, wsum, ws, None, geom, y) is False      # x_units: C H W > 2^22
    torch.cuda.synchronize()
    assert bool((y == SENT_Y).all()) and bool((nplanes == SENT_WORD).all()) and torch.equal(units, _seeds(1))
    hip.xnor_conv2d(planes, 1, scales, wbits, wsum, ws, None, geom, y, relu=True)                          # the plain call serves it
    torch.cuda.synchronize()
    assert not bool((y == SENT_Y).any())


def _module(tag, cin, cout, alpha=1.3, **kw):
    from oracle import ref_port
    from quant.binary.binary_conv import QuantConv2d
    m = QuantConv2d('ls-1', 'ls-1', cin, cout, kw.pop('kernel_size', 3), {'kind': 'symmetric', 'alpha': alpha}, **kw)
    with torch.no_grad():
        m.weight.copy_(detgen.normal(f'chain.mod.{tag}.w', m.weight.shape, scale=float(m.weight[0].numel()) ** -0.5))
        m.bias.copy_(detgen.normal(f'chain.mod.{tag}.b', m.bias.shape, scale=0.1))
        m.w_approximate.v1.copy_(ref_port.weight_scales(m.weight, 'ls-1')[0])
    return m.eval().to(DEV)


def _batch_norm(ch):
    bn = torch.nn.BatchNorm2d(ch)
    with torch.no_grad():
        bn.weight.copy_(detgen.uniform('chain.bn.g', (ch,), 0.5, 1.5))
        bn.weight[::3] *= -1.0                           # (folded scales of both signs)
        bn.bias.copy_(detgen.normal('chain.bn.b', (ch,), scale=0.2))
        bn.running_mean.copy_(detgen.normal('chain.bn.m', (ch,), scale=0.3))
        bn.running_var.copy_(detgen.uniform('chain.bn.v', (ch,), 0.5, 1.5))
    return bn.eval().to(DEV)


def _run_pair(producer, bn2, consumer, x, on, clone=False):
    """producer -> (bn2) -> consumer through fused_forward, chained or not: (y2, launches per entry point)."""
    from quant.binary import chain
    hip = _hip()
    chain.ENABLED = on
    try:
        with torch.no_grad():
            for timed in (False, True):                   # (the first run allocates the workspaces)
                hip.enable_timing(timed)
                y1 = producer.fused_forward(x, None, relu=True, next_q=(bn2, consumer))
                y2 = consumer.fused_forward(y1.clone() if clone else y1, bn2)
            torch.cuda.synchronize()
            calls = {k: v[0] for k, v in hip.drain_timing().items()}
    finally:
        chain.ENABLED = True
        hip.enable_timing(False)
    return y2.clone(), calls


@pytest.mark.parametrize('hw,chained', [(256, True), (260, False)])
def test_module_pair_at_the_row_limit(hw, chained):
    """Two QuantConv2d at batch 1: a consumer row of 2^22 elements is chained, one of 64 x 260 x 260 keeps its quantizer launch
    (chain.MAX_ELEMENTS alone would have chained it); chain.ENABLED on and off give the same output bit for bit."""
    x = detgen.normal(f'chain.modbig.{hw}', (1, 64, hw, hw)).to(DEV)
    producer, consumer = _module('p', 64, 64, padding=1), _module('cc', 64, 64, padding=1)
    y_on, calls_on = _run_pair(producer, None, consumer, x, True)
    y_off, calls_off = _run_pair(producer, None, consumer, x, False)
    assert torch.equal(y_on, y_off)
    assert calls_off['lsq_act_quant'] == 2 and calls_on['lsq_act_quant'] == (1 if chained else 2), (calls_on, calls_off)


# ------------------------------------------------------------------------------------------------------------- refusals
def _refusal_setup(C=64, O=64, k=3, groups=1, dil=(1, 1), n=2, hw=6):
    hip = _hip()
    geom = hip.make_geom(n, C, hw, hw, O, k, k, (1, 1), (1, 1), dil, groups)
    ho, wo = hip.out_hw(geom)
    tag = f'chain.ref.{C}.{O}.{k}.{groups}.{dil}'
    planes, scales = _quantize(detgen.normal(tag + '.x', (n, C, hw, hw)).to(DEV), geom, CC.ALPHA_IN)
    ws = detgen.uniform(tag + '.ws', (1, O), 0.01, 0.02).to(DEV)
    wbits, wsum = hip.pack_weight(detgen.normal(tag + '.w', (O, C // groups, k, k)).to(DEV), geom, ws)
    y = torch.full((n, O, ho, wo), SENT_Y, dtype=torch.float32, device=DEV)
    nplanes, units = _next_buffers(n, O, ho, wo, (1, 1)), _seeds(n)
    pre = (torch.ones((O,), device=DEV), torch.zeros((O,), device=DEV))
    return types.SimpleNamespace(geom=geom, planes=planes, scales=scales, ws=ws, wbits=wbits, wsum=wsum, y=y, nplanes=nplanes, units=units,
                                 pre=pre, n=n)


def _untouched(b):
    torch.cuda.synchronize()
    return bool((b.y == SENT_Y).all()) and bool((b.nplanes == SENT_WORD).all()) and torch.equal(b.units, _seeds(b.n))


def _call(b, xscales='own', x_units=None, x_alpha=1.3, planes='own', units='own', scale=None, shift=None, alpha=1.3, pad=(1, 1),
          with_next=True):
    hip = _hip()
    nxt = None
    if with_next:
        nxt = hip.NextLs1(b.nplanes.data_ptr() if planes == 'own' else planes, b.units.data_ptr() if units == 'own' else units,
                          scale, shift, alpha, *pad)
    return hip.xnor_conv2d_chain(b.planes, b.scales if xscales == 'own' else xscales, x_units, x_alpha, b.wbits, b.wsum, b.ws, None,
                                 b.geom, b.y, nxt=nxt)


def test_refusals_leave_every_buffer_untouched():
    """Every argument combination the entry point refuses, on real, correctly sized, sentinel-filled buffers (a wrongly
    accepted call would still write in bounds): the code, and nothing written."""
    hip = _hip()
    b = _refusal_setup()
    with pytest.raises(hip.LsqHipError, match='code -3'):                      # LSQ_E_SCHEME: two sources for the scale
        _call(b, x_units=b.units)
    assert _untouched(b)
    for kw in (dict(planes=None), dict(units=None), dict(scale=b.pre[0].data_ptr()), dict(shift=b.pre[1].data_ptr())):
        with pytest.raises(hip.LsqHipError, match='code -1'):                  # LSQ_E_NULL
            _call(b, **kw)
        assert _untouched(b), kw
    for kw in (dict(alpha=0.0), dict(alpha=-1.3), dict(alpha=float('nan')), dict(pad=(-1, 1)), dict(pad=(1, -1)),
               dict(xscales=None, x_units=b.units, x_alpha=0.0, with_next=False),
               dict(xscales=None, x_units=b.units, x_alpha=-2.0, with_next=False)):
        assert _call(b, **kw) is False, kw                                      # LSQ_E_UNSUPPORTED
        assert _untouched(b), kw
    assert _call(b, scale=b.pre[0].data_ptr(), shift=b.pre[1].data_ptr()) is True      # (the buffers are what an accepted call needs)
    torch.cuda.synchronize()
    assert not bool((b.y == SENT_Y).any()) and not torch.equal(b.units, _seeds(b.n))
    for setup in (dict(O=32), dict(O=96), dict(k=5), dict(C=192), dict(C=128, groups=2), dict(dil=(1, 2))):
        b = _refusal_setup(**setup)
        assert _call(b) is False, setup
        assert _untouched(b), setup
        if setup not in (dict(O=32), dict(O=96)):                               # (outside the matrix-core kernel: x_units too)
            assert _call(b, xscales=None, x_units=b.units, with_next=False) is False, setup
            assert _untouched(b), setup
    b = _refusal_setup(dil=(2, 1))                                              # dil_h = 2 is inside the kernel
    assert _call(b) is True


# ---------------------------------------------------------------------------------------------------- module fall-backs
@pytest.mark.parametrize('which', ['chainable', '1x1', 'dilation_1_2', '192_channels', 'clone'])
def test_module_falls_back_to_its_own_quantizer_launch(which):
    """A producer that is told its consumer leaves plane and sums; a consumer outside the chained kernel (1 x 1, dil_w = 2, 192
    channels) or one that is fed another tensor object quantizes for itself: one more lsq_act_quant launch, and the output of
    the unchained pair bit for bit."""
    ch = 192 if which == '192_channels' else 128
    x = detgen.normal(f'chain.fb.{which}', (3, 64, 9, 7)).to(DEV)
    producer = _module('prod', 64, ch, padding=1)
    kw = {'1x1': dict(kernel_size=1), 'dilation_1_2': dict(padding=(1, 2), dilation=(1, 2))}.get(which, dict(padding=1))
    consumer = _module('cons' + which, ch, 64, **kw)
    bn2 = _batch_norm(ch)
    y_on, calls_on = _run_pair(producer, bn2, consumer, x, True, clone=which == 'clone')
    y_off, calls_off = _run_pair(producer, bn2, consumer, x, False, clone=which == 'clone')
    assert torch.equal(y_on, y_off), which
    assert calls_off['lsq_act_quant'] == 2
    assert calls_on['lsq_act_quant'] == (1 if which == 'chainable' else 2), (which, calls_on)
