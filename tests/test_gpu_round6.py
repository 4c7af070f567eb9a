"""Round-6 GPU tests: the single-launch quantizer against the exact oracle and against its own forced fall-back, the fused
batch-256 network layer by layer, non-finite rows in the windowed solve, and the fp4 convolution at the extremes of its
integer range."""

import numpy as np
import pytest
import torch

from oracle import lsq_exact as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _hip():
    from quant import _hip
    return _hip


def _quantize(x, alpha, ternary=False, pre=None, mode=0):
    hip = _hip()
    n, c, h, w = x.shape
    geom = hip.make_geom(n, c, h, w, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    planes = torch.zeros((2 * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    scales = torch.empty((2, n), dtype=torch.float32, device=DEV)
    with hip.debug_switches(fused_mode=mode):
        hip.act_quant(x.to(DEV), geom, hip.SCHEME_LST if ternary else hip.SCHEME_LS2, 2, 3, alpha, planes, scales, None, pre)
        torch.cuda.synchronize()
    return planes.cpu(), scales.cpu()


@pytest.mark.parametrize('ternary', [False, True])
def test_quantizer_equals_the_exact_oracle_and_its_forced_fall_back(ternary):
    """lsq_act_quant on the four ResNet row shapes and three short ones, odd batch sizes: v1 == the exact oracle bit for bit, and
    -- with and without the folded batch norm -- planes, v1 and v2 of the forced fall-back of the windowed solve
    (lsq_debug_fused_mode 8) == those of the windowed solve itself."""
    rs = np.random.RandomState(6)
    for (n, c, h) in [(3, 64, 56), (5, 128, 28), (4, 256, 14), (7, 512, 7), (2, 64, 28), (2, 64, 14), (3, 128, 7)]:
        x = torch.from_numpy((rs.standard_normal((n, c, h, h)) * 1.3).astype(np.float32))
        for pre in (None, 'bn'):
            p = None
            if pre:
                sc = torch.from_numpy((0.5 + rs.random_sample(c)).astype(np.float32))
                sh = torch.from_numpy((0.3 * rs.standard_normal(c)).astype(np.float32))
                p = (sc.to(DEV), sh.to(DEV))
            want_p, want_s = _quantize(x, 3.0, ternary, p)
            got_p, got_s = _quantize(x, 3.0, ternary, p, mode=8)
            assert torch.equal(got_s, want_s), (n, c, h, pre, got_s, want_s)
            assert torch.equal(got_p, want_p), (n, c, h, pre)
            if not pre:
                exact = E.solve_rows(x.clamp(-3, 3).reshape(n, -1).numpy(), ternary, 3)
                assert np.array_equal(want_s[0].numpy(), exact)


# ---------------------------------------------------------------------------------------------- the path bench.py times, layer by layer
@pytest.mark.parametrize('act', ['ls-2', 'ls-T'])
def test_full_size_fused_network_every_layer(act):
    """The FUSED batch-256 forward -- what bench.py times -- checked layer by layer on three rows of the batch (round 5's
    test_full_size_whole_network does this on the module-by-module path and compared the two paths by a hand-set cosine):
    every QuantConv2d.fused_forward call is recorded in place, and for each of the 16 layers
      * the solved v1 equals the exact oracle on the very tensor the layer quantized (the eval batch norm folded as ONE fma
        per element, as the kernel's read does),
      * the layer's output is within north_star's 1e-4 of max|y| of an fp64 convolution of that quantized input with the
        GPU's own scales, the block's epilogue (residual before / after the non-linearity, ReLU or PReLU) included."""
    import bench
    from oracle import ref_port as P
    from quant.binary.binary_conv import QuantConv2d
    model = bench.build_model(bench.imagenet_arch(act, 3 if act == 'ls-2' else 2), DEV)
    x = torch.randn(256, 3, 224, 224, generator=torch.Generator().manual_seed(0)).to(DEV)
    rows = [0, 131, 255]
    seen = []
    orig = QuantConv2d.fused_forward

    def spy(self, xin, pre_bn=None, relu=False, res_pre=None, res_post=None, prelu=None, next_q=None, res_ready=None):
        out = orig(self, xin, pre_bn, relu, res_pre, res_post, prelu, next_q, res_ready)
        pick = lambda t: None if t is None else t[rows].clone()        # noqa: E731
        seen.append((self, pre_bn, relu, None if prelu is None else prelu.detach().clone(), pick(xin), pick(res_pre), pick(res_post),
                     pick(out), self.last_act_scales[:, rows].clone()))
        return out
    QuantConv2d.fused_forward = spy
    try:
        with torch.no_grad():
            model(x)
    finally:
        QuantConv2d.fused_forward = orig
    assert len(seen) == 16
    ternary = act == 'ls-T'
    for li, (conv, bn, relu, slope, xin, rpre, rpost, yout, scales) in enumerate(seen):
        alpha = conv._alpha()
        s, t = conv._folded_bn(bn)
        xb = (xin.double() * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1)).float()     # one rounding: the kernel's fma
        xc = xb.clamp(-alpha, alpha)
        want = E.solve_rows(xc.reshape(len(rows), -1).cpu().numpy(), ternary, 3)
        assert np.array_equal(scales[0].cpu().numpy(), want), (li, scales[0], want)
        xq = P.quant_lst(xc, scales[0])[1] if ternary else P.quant_ls2(xc, scales[0], scales[1])[2]
        wq = conv.w_approximate.v1.view(-1, 1, 1, 1) * P.pm1(conv.weight)
        ref = torch.nn.functional.conv2d(xq.double(), wq.double(), conv.bias.double(), conv.stride, 1)
        if rpre is not None:
            ref = ref + rpre.double()
        if relu:
            ref = ref.clamp_min(0)
        if slope is not None:
            ref = torch.where(ref > 0, ref, ref * slope.double().view(1, -1, 1, 1))
        if rpost is not None:
            ref = ref + rpost.double()
        err = float((yout.double() - ref).abs().max() / ref.abs().max())
        assert err <= 1e-4, (li, err)


def test_non_finite_rows_stay_contained_in_the_windowed_solve():
    """a row with NaN / +-Inf activations under a symmetric clamp (Inf clamps to alpha, a NaN to -alpha: the
    windowed histogram's index stays inside its 8192 bins -- now also bounded explicitly) must neither fault nor touch its
    neighbours: the finite rows of the batch come out exactly as they do alone, and the Inf row as its clamped self."""
    rs = np.random.RandomState(8)
    for (c, h) in [(64, 56), (128, 28), (512, 7)]:
        x = torch.from_numpy((rs.standard_normal((4, c, h, h)) * 1.5).astype(np.float32))
        bad = x.clone()
        bad[1].view(-1)[::7] = float('nan')
        bad[1].view(-1)[3::11] = float('inf')
        bad[2].view(-1)[5::13] = float('-inf')              # no NaN in row 2: it equals its clamped self
        for ternary in (False, True):
            p_bad, s_bad = _quantize(bad, 3.0, ternary)
            p_ok, s_ok = _quantize(x, 3.0, ternary)
            p_cl, s_cl = _quantize(bad.clamp(-3, 3).nan_to_num(0.0), 3.0, ternary)
            words = p_ok.numel() // 2 // 4
            for row in (0, 3):
                assert s_bad[0, row] == s_ok[0, row] and s_bad[1, row] == s_ok[1, row], (c, h, ternary, row)
                for plane in (0, 1):
                    a = p_bad.view(2, 4, words)[plane, row]
                    assert torch.equal(a, p_ok.view(2, 4, words)[plane, row]), (c, h, ternary, row, plane)
            assert s_bad[0, 2] == s_cl[0, 2] and torch.equal(p_bad.view(2, 4, words)[:, 2], p_cl.view(2, 4, words)[:, 2])


@pytest.mark.parametrize('cin', [64, 128, 256, 512])
def test_fp4_convolution_at_the_extremes_of_its_integer_range(cin):
    """The fp4 matrix-core kernel's accumulator holds (b * s) as an fp32 integer: at most 9 * C = 4608 in magnitude.  All-(+1) and
    all-(-1) activations against all-(+1) weights reach the extremes on interior pixels (and every border pattern's correction on
    the rim): the output is the closed form, and equal to the popcount and int8 kernels bit for bit; fp4 codes of every slot
    (0.5 / 1 / 2 / 0.5 against 4 / 2 / 1 / 4) are exercised by single-channel impulses."""
    hip = _hip()
    n, h, o = 3, 9, 64
    geom = hip.make_geom(n, cin, h, h, o, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    wt = torch.ones(o, cin, 3, 3, device=DEV)
    wt[1::2] = -1.0                                           # odd out-channels: all -1
    wsc = torch.full((1, o), 0.5, device=DEV)
    wbits, wsum = hip.pack_weight(wt, geom, wsc)
    bias = torch.arange(o, dtype=torch.float32, device=DEV)
    planes = torch.zeros((2 * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    scales = torch.empty((2, n), dtype=torch.float32, device=DEV)
    cases = {'plus': torch.full((n, cin, h, h), 2.0), 'minus': torch.full((n, cin, h, h), -2.0)}
    imp = torch.full((n, cin, h, h), -2.0)
    for c in range(0, cin, 5):
        imp[:, c, (c // 5) % h, (c // 3) % h] = 2.0           # single +1 bits in every channel slot
    cases['impulses'] = imp
    for tag, x in cases.items():
        # planes with given scales (v1 = 1, v2 = 0.25): plane 1 = sign(x), plane 2 = sign(x - v1 b1) = sign(x) for |x| = 2
        forced = torch.tensor([[1.0] * n, [0.25] * n], device=DEV)
        hip.act_quant(x.to(DEV), geom, hip.SCHEME_LS2, 2, 3, 3.0, planes, scales, forced)
        outs = []
        for impl in (1, 0, 2):
            with hip.debug_switches(xnor_popcount=impl):
                y = torch.empty((n, o, h, h), device=DEV)
                hip.xnor_conv2d(planes, 2, scales, wbits, wsum, wsc, bias, geom, y)
                outs.append(y.clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (cin, tag)
        if tag != 'impulses':
            taps = torch.nn.functional.conv2d(torch.ones(1, 1, h, h), torch.ones(1, 1, 3, 3), padding=1).view(h, h).to(DEV)   # taps inside the image
            s1 = 1.0 if tag == 'plus' else -1.0
            sign_o = torch.where(torch.arange(o, device=DEV) % 2 == 0, 1.0, -1.0)
            want = bias.view(1, o, 1, 1) + 0.5 * sign_o.view(1, o, 1, 1) * (1.0 * s1 + 0.25 * s1) * cin * taps.view(1, 1, h, h)
            assert torch.equal(outs[1], want.expand(n, o, h, h).contiguous()), (cin, tag, float((outs[1] - want).abs().max()))
