"""tests/golden/chain_cases.py on the host (no GPU): the numpy model of lsq_xnor_conv2d_chain's epilogue against an independent
slow implementation, the conditions the shared inputs must meet, the unit's definition, and the 2^22 row limit of the chained
call on both sides of the binding (``_chain_target`` against a stubbed binding; the entry point's refusal, which returns before
any launch)."""

import ctypes
import fractions
import math
import types

import numpy as np
import pytest
import torch

import chain_cases as CC
from quant import _hip
from quant.binary import chain
from quant.binary.binary_conv import QuantConv2d


# ------------------------------------------------------------------------------------- the model against a slow restatement
def _slow_units(octets: np.ndarray, e: int) -> list:
    """Per octet: the fp32 chain with Python floats cast through np.float32, the rounding to a multiple of 2^e in rationals."""
    out = []
    for row in octets:
        acc = np.float32(row[0])
        for v in row[1:]:
            acc = np.float32(float(acc) + float(np.float32(v)))       # (the fp64 sum of two fp32 numbers rounds to fp32 once)
        out.append(round(fractions.Fraction(float(acc)) / fractions.Fraction(2) ** e))      # round(): ties to even
    return out


def _octets(alpha: float, e: int) -> np.ndarray:
    """A few hundred octets of |clamped| values: random ones at every magnitude down to below the unit, octets at the clamp,
    zeros, and sums that land exactly on a tie (an odd multiple of half a unit)."""
    rs = np.random.RandomState(int(alpha * 100) + 7)
    a = np.float32(alpha)
    rows = [np.minimum(np.abs(rs.standard_normal((200, 8)) * 0.8 * alpha), a)]
    rows.append(np.minimum(np.abs(rs.standard_normal((60, 8))) * alpha * 2.0 ** rs.randint(-40, 0, size=(60, 1)), a))
    rows.append(np.full((2, 8), a))
    rows.append(np.zeros((2, 8)))
    half = 2.0 ** (e - 1)
    ties = np.zeros((48, 8))
    for i in range(48):
        odd = 2 * i + 1                                   # sum = odd * half a unit: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, ...
        if i % 3 == 0:
            ties[i, i % 8] = odd * half
        elif i % 3 == 1:
            ties[i, 0], ties[i, 7] = (odd - 1) * half, half
        else:
            ties[i, 2], ties[i, 3], ties[i, 5] = half, (odd - 2) * half, half
    rows.append(ties)
    return np.concatenate(rows).astype(np.float32)


@pytest.mark.parametrize('alpha', CC.ALPHAS)
def test_model_equals_a_slow_exact_implementation(alpha):
    e = CC.unit_exponent(alpha)
    octs = _octets(alpha, e)
    sums = CC.octet_sums(octs.T.reshape(1, 8, -1))[0, 0]
    got = CC.round_to_units(sums, e)
    want = _slow_units(octs, e)
    assert got.tolist() == want
    ties = want[-48:]
    assert ties[0] == 0 and ties[3] == 4 and all(v % 2 == 0 for v in ties)     # half-way sums went to the even neighbour
    # and through the whole-tensor entry: one sample, 8 channels, one pixel per octet
    y = octs.T.reshape(1, 8, 1, -1) * np.where(np.arange(octs.shape[0]) % 2, -1.0, 1.0).astype(np.float32)
    assert int(CC.model_units(y, alpha)[0]) == sum(want)


@pytest.mark.parametrize('alpha', CC.ALPHAS)
def test_unit_is_the_power_of_two_at_or_above_the_clamp(alpha):
    """alpha = m 2^e2 with 0.5 <= m < 1: 2^e2 >= alpha > 2^(e2-1), except at an exact power of two, where 2^e2 = 2 alpha
    (NOT ceil(log2 alpha), which the documents used to give)."""
    e2 = CC.unit_exponent(alpha) + 31
    m = math.log2(alpha)
    if m == int(m):
        assert 2.0 ** e2 == 2 * alpha and e2 == math.ceil(m) + 1
    else:
        assert 2.0 ** e2 >= alpha > 2.0 ** (e2 - 1) and e2 == math.ceil(m)


def test_unit_of_the_alphas_every_other_test_uses():
    assert CC.unit_exponent(2.0) == CC.unit_exponent(3.0) == 2 - 31          # why alpha = 2 and 3 exercise ONE unit
    assert [CC.unit_exponent(a) + 31 for a in CC.ALPHAS] == [-1, 1, 1, 2, 3, 9]    # five units; 1.0 sits at its unit's lower edge


# ------------------------------------------------------------------------------------------------ the cases themselves
def test_case_list_covers_what_it_is_meant_to():
    cs = [c for c in CC.CASES if c.geom != 'g']
    assert len(cs) == 24 and {(c.geom, c.C) for c in cs} == {(g, C) for g in 'abcdef' for C in CC.CHANNELS}
    for attr, values in (('O', CC.OUTS), ('next_pad', CC.NEXT_PADS), ('wplanes', (1, 2, 3)), ('epilogue', tuple(CC.EPILOGUES)),
                         ('alpha', CC.ALPHAS), ('affine', (False, True))):
        for v in values:
            assert sum(getattr(c, attr) == v for c in cs) >= 2, (attr, v)
    assert any(c.act == 'relu' and not c.res_post and not c.affine for c in cs)
    assert [(c.Ho * c.Wo) for c in (CC.BY_ID['a64'], CC.BY_ID['b64'], CC.BY_ID['c64'], CC.BY_ID['f64'])] == [4, 16, 35, 196]
    assert CC.BY_ID['a64'].N * 4 % 32 == 20 and CC.BY_ID['e64'].dil == (2, 1) and CC.BY_ID['d64'].stride == (2, 1)
    g = CC.BY_ID['g64']
    assert (g.N * g.Ho * g.Wo + 31) // 32 == 784 > 64 * 12 and g.O == 128 and g.C == 64
    for c in cs:                                          # the affine's exact-zero channels: one of each sign of zero
        if c.affine:
            d = CC.inputs(c.id)
            zero = d['s'] == 0
            assert int(zero.sum()) == 4 and {math.copysign(1.0, float(v)) for v in d['t'][zero]} == {1.0, -1.0}
            assert bool((d['s'] > 0).any()) and bool((d['s'] < 0).any())


@pytest.mark.parametrize('cid', [c.id for c in CC.CASES])
def test_inputs_meet_their_conditions_and_the_model_scale_is_the_mean(cid):
    c, d = CC.BY_ID[cid], CC.inputs(cid)
    y = CC.reference(cid).numpy().astype(np.float32)
    s, t = (None, None) if d['s'] is None else (d['s'].numpy(), d['t'].numpy())
    a = float(np.float32(c.alpha))
    v = np.clip(CC.pre_clamp64(y, s, t), -a, a)
    at_clamp, small, zeros = float((np.abs(v) == a).mean()), float((np.abs(v) < a / 16).mean()), float((v == 0).mean())
    assert 0.05 <= at_clamp <= 0.40, (cid, at_clamp)
    assert small >= 0.02, (cid, small)
    if c.act == 'relu' and not c.res_post and not c.affine:
        assert zeros >= 0.30, (cid, zeros)
    # the model's bits: 1 unless the value is negative (+-0 give 1; the clamp and the rounding of the fma keep the sign)
    bits = CC.model_bits(y, s, t, c.alpha)
    assert np.array_equal(bits, ~(v < 0))
    if s is not None:
        assert bits[:, s == 0].all()
    if s is None:
        units = CC.model_units(y, c.alpha)
        scale = CC.model_scale(units, c.alpha, c.M)
        mean = CC.mean64(y, None, None, c.alpha)
        assert np.all(np.abs(scale.astype(np.float64) - mean) <= 1e-6 * mean), (cid, scale, mean)
    words = CC.model_words(bits, c.next_pad)
    assert words.shape == (c.N, c.O // 64, c.Ho + 2 * c.next_pad[0], c.Wo + 2 * c.next_pad[1])


# ------------------------------------------------------------------------------------------------------ the row limit
def _pair():
    clamp = {'kind': 'symmetric', 'alpha': 1.3}
    producer = QuantConv2d('ls-1', 'ls-1', 64, 64, 3, clamp, padding=1).eval()
    consumer = QuantConv2d('ls-1', 'ls-1', 64, 64, 3, clamp, padding=1).eval()
    return producer, consumer


def test_chain_target_declines_a_consumer_row_above_2_22_elements():
    stub = types.SimpleNamespace(NextLs1=_hip.NextLs1, stream_ptr=lambda device=None: 0)
    dev = torch.device('cpu')
    assert chain.MAX_ROW_ELEMENTS == 1 << 22
    producer, consumer = _pair()
    got = producer._chain_target((None, consumer), 1, 256, 256, dev, stub)              # 64 * 256 * 256 = 2^22 exactly
    assert got is not None and got[1].shape == (1, 64, 256, 256) and got[0].clamp_alpha == pytest.approx(1.3)
    assert any(isinstance(k, tuple) and k[0] == 'pre' for k in consumer._hip_cache)
    assert producer._chain_target((None, consumer), 2, 256, 256, dev, stub) is not None  # two such rows: 2^23 in all
    producer, consumer = _pair()
    assert producer._chain_target((None, consumer), 1, 256, 257, dev, stub) is None
    assert producer._chain_target((None, consumer), 1, 260, 260, dev, stub) is None
    assert producer._chain_target((None, consumer), 2, 260, 260, dev, stub) is None      # (the 2^23 cap declines this one anyway)
    assert not any(isinstance(k, tuple) and k[0] == 'pre' for k in consumer._hip_cache)  # no workspace was allocated
    assert producer._chain_target((None, consumer), 3, 256, 256, dev, stub) is None      # chain.MAX_ELEMENTS still holds


def test_entry_point_refuses_rows_above_2_22_before_any_launch():
    """The refusal comes before any launch and before any pointer is read, so on a machine without a GPU it can be called
    with made-up addresses (with a GPU, tests/test_gpu_chain.py makes the same calls on real buffers)."""
    if torch.cuda.is_available():
        return
    if not _hip.available():
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.lib()
    fake = 0x1000

    def call(h, w, c=64, o=64, x_units=None, xscales=fake, nxt=True, alpha=1.3):
        g = _hip.make_geom(1, c, h, w, o, 3, 3, (1, 1), (1, 1), (1, 1), 1)
        n = _hip.NextLs1(fake, fake, None, None, alpha, 1, 1) if nxt else None
        return lib.lsq_xnor_conv2d_chain(fake, xscales, x_units, 1.3, fake, fake, 1, fake, None, ctypes.byref(g), 0, None, None,
                                         None, None if n is None else ctypes.byref(n), fake, None)

    assert call(260, 260) == _hip.E_UNSUPPORTED                        # next: O Ho Wo = 64 * 260 * 260 > 2^22
    assert call(256, 257) == _hip.E_UNSUPPORTED
    assert call(128, 128, o=320) == _hip.E_UNSUPPORTED                 # 320 * 2^14 > 2^22
    assert call(260, 260, x_units=fake, xscales=None, nxt=False) == _hip.E_UNSUPPORTED      # x_units: C H W > 2^22
    assert call(128, 128, c=512, x_units=fake, xscales=None, nxt=False) == _hip.E_UNSUPPORTED       # 512 * 2^14 = 2^23
    assert call(16, 16, x_units=fake, xscales=fake) == -3             # both sources of the scale: LSQ_E_SCHEME
    assert call(16, 16, alpha=0.0) == _hip.E_UNSUPPORTED and call(16, 16, alpha=-1.0) == _hip.E_UNSUPPORTED
