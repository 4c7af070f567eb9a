"""lsq_xnor_conv2d_chain_fixed through its C entry point (include/lsq_hip_conv_chain.h; csrc/lsq_xnor_mfma.hip, the NQF
instantiations): y against the unchained lsq_xnor_conv2d (equal) and the fp64 convolution (1e-4 of max |y|, the bound of this
kernel's other tests), the consumer's planes against the CPU model of tests/golden/chain_fixed_cases.py on the y the call wrote
and against lsq_act_quant with the same given scales -- every word, halo included, equal --, and every refusal."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import chain_fixed_cases as FC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOL = 1e-4
SENT_WORD = 0x5A5AA5A55A5AA5A5
SENT_Y = 12345.0


def _hip():
    from quant import _hip
    return _hip


@functools.lru_cache(maxsize=None)
def _prepared(cid):
    """Device inputs of a case: the producer's own planes (lsq_act_quant with its given scales) and packed weights."""
    hip = _hip()
    c = FC.BY_ID[cid]
    d = {k: (None if v is None else v.to(DEV)) for k, v in FC.inputs(cid).items()}
    geom = hip.make_geom(c.N, c.C, c.H, c.W, c.O, 3, 3, (c.stride,) * 2, (c.pad,) * 2, (1, 1), 1)
    planes = torch.zeros((c.kx * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xscales = torch.empty((c.kx, c.N), dtype=torch.float32, device=DEV)
    hip.act_quant(d['x'], geom, hip.SCHEME_LS1 if c.kx == 1 else hip.SCHEME_LS2, c.kx, 3, FC.CC.ALPHA_IN, planes, xscales, d['xs'])
    wbits, wsum = hip.pack_weight(d['w'], geom, d['wscales'])
    return geom, d, planes, xscales, wbits, wsum


def _operands(cid):
    c = FC.BY_ID[cid]
    geom, d, planes, xscales, wbits, wsum = _prepared(cid)
    return (planes, c.kx, xscales, wbits, wsum, d['wscales'], d['bias'], geom), dict(res_post=d['res_post'], prelu=d['slope'])


def _words(t, c):
    ho, wo = FC.out_hw(c)
    return t.cpu().numpy().view(np.uint64).reshape(c.k, c.N, c.O // 64, ho + 2 * c.next_pad[0], wo + 2 * c.next_pad[1])


def _check(cid, scales=None):
    """(a), (b), (c) of one chained call with the case's scales (or ``scales``); returns (c of the CPU model, plane words)."""
    hip = _hip()
    c = FC.BY_ID[cid]
    args, epi = _operands(cid)
    d = _prepared(cid)[1]
    scales = d['scales'] if scales is None else scales.to(DEV)
    ho, wo = FC.out_hw(c)
    shape = (c.N, c.O, ho, wo)
    y_plain = torch.full(shape, SENT_Y, dtype=torch.float32, device=DEV)
    hip.xnor_conv2d(*args, y_plain, **epi)
    y = torch.full(shape, SENT_Y, dtype=torch.float32, device=DEV)
    words = c.N * (c.O // 64) * (ho + 2 * c.next_pad[0]) * (wo + 2 * c.next_pad[1])
    nplanes = torch.zeros((c.k * words,), dtype=torch.int64, device=DEV)        # (the caller zeroes the halo)
    nxt = hip.NextFixed(nplanes.data_ptr(), c.k, scales.data_ptr(), hip.ptr(d['s']), hip.ptr(d['t']), c.alpha, *c.next_pad)
    assert hip.xnor_conv2d_chain_fixed(*args, y, nxt, **epi)
    # what lsq_act_quant writes for the same y and scales (the layout needs no kernel size)
    g2 = hip.make_geom(c.N, c.O, ho, wo, 64, 1, 1, (1, 1), c.next_pad, (1, 1), 1)
    qplanes = torch.zeros_like(nplanes)
    qscales = torch.empty((c.k, c.N), dtype=torch.float32, device=DEV)
    hip.act_quant(y, g2, FC.SCHEMES[c.scheme][0], c.k, 3, c.alpha, qplanes, qscales, scales, None if d['s'] is None else (d['s'], d['t']))
    torch.cuda.synchronize()
    ref = FC.reference(cid)
    err = float((y.cpu().double() - ref).abs().max() / ref.abs().max())
    s, t = (None, None) if d['s'] is None else (d['s'].cpu(), d['t'].cpu())
    model = FC.model_words(y.cpu(), s, t, c.alpha, scales.cpu(), c.next_pad)
    got = _words(nplanes, c)
    print(f'CHAIN-FIXED {cid} y_rel_err={err:.3e} words={got.size} differ_model={int((got != model).sum())} '
          f'differ_act_quant={int((got != _words(qplanes, c)).sum())}')
    assert torch.equal(y, y_plain) and err <= TOL, (cid, err)                   # (a)
    assert np.array_equal(got, model), cid                                      # (b) halo included: zero
    assert np.array_equal(got, _words(qplanes, c)), cid                         # (c)
    return FC.pre_quant(y.cpu(), s, t, c.alpha), got


@pytest.mark.parametrize('cid', [c.id for c in FC.CASES if c.id != 'anchor'])
def test_planes_and_y(cid):
    _check(cid)


def test_anchor_zero_residuals_give_bit_one():
    """Scales set from the tensor's own values: element e's residual in front of plane 2 and element f's in front of plane 3
    are exactly zero, and both bits are 1."""
    c = FC.BY_ID['anchor']
    pre, _ = _check('anchor')                             # a first run: the values the scales are taken from
    scales, e, f = FC.anchor_scales(pre, FC.inputs('anchor')['scales'])
    bits = FC.model_bits(pre, None, None, -1.0, scales)
    assert bits[1][0].reshape(-1)[e] and bits[2][0].reshape(-1)[f]               # (the model: zero residual -> 1)
    _, words = _check('anchor', scales)
    ho, wo = FC.out_hw(c)
    for plane, idx in ((1, e), (2, f)):
        o, r = divmod(idx, ho * wo)
        h, w = divmod(r, wo)
        assert (int(words[plane, 0, o // 64, h + c.next_pad[0], w + c.next_pad[1]]) >> (o % 64)) & 1 == 1, (plane, idx)


REFUSALS = {                       # what to change of case two_samples -> the expected code
    'O32': -6, 'kernel5': -6, 'groups2': -6, 'k9': -3, 'kx3': -3, 'null_planes': -1, 'pre_scale_alone': -1, 'pre_shift_alone': -1}


@pytest.mark.parametrize('what', list(REFUSALS))
def test_refusals_write_nothing(what):
    hip = _hip()
    c = FC.BY_ID['two_samples']
    geom, d, planes, xscales, wbits, wsum = _prepared('two_samples')
    o = 32 if what == 'O32' else c.O
    ks = 5 if what == 'kernel5' else 3
    groups = 2 if what == 'groups2' else 1
    g = hip.make_geom(c.N, c.C, c.H, c.W, o, ks, ks, (1, 1), (ks // 2,) * 2, (1, 1), groups)
    y = torch.full((c.N, c.O, c.H, c.W), SENT_Y, dtype=torch.float32, device=DEV)
    nplanes = torch.full((8 * c.N * (c.H + 2) * (c.W + 2),), SENT_WORD, dtype=torch.int64, device=DEV)
    vec = torch.ones((c.O,), dtype=torch.float32, device=DEV)
    nxt = hip.NextFixed(None if what == 'null_planes' else nplanes.data_ptr(), 9 if what == 'k9' else 2, d['scales'].data_ptr(),
                        vec.data_ptr() if what == 'pre_scale_alone' else None,
                        vec.data_ptr() if what == 'pre_shift_alone' else None, 2.0, 1, 1)
    # (large enough for every variant: the call must not read them either)
    big = torch.zeros((1 << 16,), dtype=torch.int64, device=DEV)
    code = hip.conv_chain_lib().lsq_xnor_conv2d_chain_fixed(
        big.data_ptr(), 3 if what == 'kx3' else 1, xscales.data_ptr(), big.data_ptr(), big.data_ptr(), 1, d['wscales'].data_ptr(),
        None, ctypes.byref(g), 0, None, None, None, ctypes.byref(nxt), y.data_ptr(), hip.stream_ptr(y.device))
    torch.cuda.synchronize()
    assert code == REFUSALS[what], (what, code)
    assert bool((y == SENT_Y).all()) and bool((nplanes == SENT_WORD).all()), what
    assert hip.conv_chain_lib().lsq_xnor_conv2d_chain_fixed(
        big.data_ptr(), 1, xscales.data_ptr(), big.data_ptr(), big.data_ptr(), 1, d['wscales'].data_ptr(), None, ctypes.byref(g), 0,
        None, None, None, None, y.data_ptr(), hip.stream_ptr(y.device)) == -1      # next NULL
