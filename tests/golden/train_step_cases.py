"""Cases, inputs and the fp64 reference of QuantConv2d's train step on the kernels (quant/binary/hip_train.py), shared by
tests/test_train_step_cases_host.py (the reference against fp32 autograd through the torch formulation, the conditions the
table must meet) and tests/test_gpu_train_geometries.py (the kernels).  Plain Python on the CPU; nothing here touches a GPU.

``chain`` is the quantizer chain in torch with the straight-through gradient's closed form (tests/test_training.py pins the
formula to autograd through the reference-equal torch formulation; tests/test_gpu_round4.py pins lsq_quant_values to its
value bit for bit).  ``step64`` is the whole step in fp64 for GIVEN activation and weight scales: every decision of the
chains (sign of d_i, |d_i| <= 1, inside the clamp) is made in fp32 exactly as the kernels make it, every value is fp64.

``transposed_kernel`` restates the dispatch of lsq_signw_conv2d (patch_plan of csrc/lsq_signw_conv_core.h) for the role the convolution plays in the backward pass: input
channels = the layer's O, out-channels = the layer's C, unit stride over the zero-inserted gradient, padding k-1-p, a
pre-scale always present and no prepared weights (so never the 3x3 fast path).
"""

import collections
import functools

import torch

import detgen

Case = collections.namedtuple('Case', 'id xs ws clamp C O KH KW stride pad_h pad_w N H W bias')

IDENT = {'kind': 'identity'}
SYM2 = {'kind': 'symmetric', 'alpha': 2}
SYM15 = {'kind': 'symmetric', 'alpha': 1.5}

# Transposed role per case: (kernel, wide = C > 64, many = more than 9 taps), by hand from the dispatch; PLr = the patch
# rows rounded up to 128 (<= 512 for the patch kernel), Hp x Wp = the padded (zero-inserted) gradient.
CASES = [
    # baseline: 6x5 gradient, pad 1 -> 8x7, PLr 512: patch, narrow (64 x 256), 9 taps
    Case('base3x3', 'ls-1', 'ls-1', SYM2, 8, 16, 3, 3, 1, 1, 1, 2, 6, 5, True),
    # C = 72 > 64: wide patch (128 x 128); gradient 5x11, transposed pad (2, 0) -> 9x11, PLr 256; two planes through res_post
    Case('wide_patch', 'fp', 'ls-2', IDENT, 72, 16, 3, 3, 1, 0, 2, 2, 7, 9, False),
    # O = 520 rounds to 528 > 512 input channels under a pre-scale: tiled, narrow (64 out-channels), three planes
    Case('o520_tiled', 'fp', 'gf-3', IDENT, 8, 520, 3, 3, 1, 1, 1, 1, 6, 5, True),
    # projection shortcut 1x1 stride 2: tiled, wide (128); rows 6 and column 5 of x are never read (7x6, zero insertion to 7x6)
    Case('o520_proj', 'fp', 'ls-1', IDENT, 72, 520, 1, 1, 2, 0, 0, 2, 7, 6, False),
    # the same tiled wide route with binary activations: lsq_train_wgrad at 1x1 stride 2 over 520 out-channels
    Case('o520_proj_b', 'ls-2', 'ls-1', SYM2, 72, 520, 1, 1, 2, 0, 0, 2, 7, 6, True),
    # a row of 260: 255 + 2 * 260 + 1 rows of patch -> PLr 896 > 512: tiled narrow although O = 16
    Case('long_row', 'fp', 'ls-1', IDENT, 8, 16, 3, 1, 1, 2, 0, 1, 3, 260, True),
    # 25 taps: 16x16 gradient, pad 2 -> 20x20, 255 + 16 * 4 + 80 + 85 = 484 -> PLr 512: patch narrow, many (three tap groups;
    # on 9x8 the patch of 256 pixels spans four images and their gaps, 628 rows, and the layer goes to the tiled kernel)
    Case('k5_many', 'ls-2', 'ls-T', SYM2, 20, 50, 5, 5, 1, 2, 2, 2, 16, 16, False),
    # O = 1: ONE input channel in a 16-channel chunk, 49 taps, wide (C = 130: two out-channel tiles, the second of 2 rows);
    # stride 2 over 13x12 -> gradient 7x6 zero-inserted to 13x12, pad 3 -> 19x18, PLr 512: patch wide many
    Case('k7_o1', 'ls-1', 'gf-3', SYM2, 130, 1, 7, 7, 2, 3, 3, 1, 13, 12, True),
    # pad = k-1 on both axes: transposed padding 0; gradient 11x10 unpadded, 255 + 32 * 2 + 4 * 30 + 33 = 472 -> PLr 512:
    # patch narrow many (12 taps)
    Case('k4x3_padfull', 'gf-2', 'ls-2', SYM15, 16, 33, 4, 3, 1, 3, 2, 2, 8, 8, True),
    # 8x8, the largest kernel of the XNOR forward: gradient 27x5, transposed pad (0, 7) -> 27x19; only the wide kernel's 128
    # pixels keep seven rows of taps inside 512 rows (127 + 11 * 7 + 133 + 141 = 478), so C = 72: patch wide many (64 taps)
    Case('k8x8', 'ls-T', 'ls-1', SYM2, 72, 8, 8, 8, 1, 7, 0, 1, 20, 12, False),
    # stem-like: 3 -> 64, fp activations under the symmetric clamp; gradient 8x8 zero-inserted to 16x16, pad 3 -> 22x22:
    # 255 + 22 rows of gap 6 + 6 * 22 + 6 + 1 > 512: tiled narrow, 49 taps, 3 out-channels
    Case('stem7x7', 'fp', 'ls-1', SYM2, 3, 64, 7, 7, 2, 3, 3, 2, 16, 16, True),
    # stride 2, (H + 2p - k) = 11 odd on rows, 6 even on columns: the last row of x (padded) is never read; gradient 6x4
    # zero-inserted to 12x7, transposed pad (0, 4) -> 12x15, PLr 512: patch narrow many (15 taps)
    Case('s2_3x5', 'ls-2', 'ls-1', SYM2, 20, 50, 3, 5, 2, 2, 0, 2, 10, 11, True),
    # even kernel 2x2 stride 2: rows even (6), columns odd (9): the last padded column unread; gradient 4x5 zero-inserted to
    # 7x10, transposed pad (1, 0) -> 9x10, PLr 256: patch wide (C = 100), 4 taps
    Case('s2_2x2', 'ls-T', 'ls-2', SYM2, 100, 96, 2, 2, 2, 0, 1, 2, 8, 9, False),
    # output 1x1 (H = k - 2p), three samples: gradient 1x1, pad 3 -> 7x7; 256 pixels are 29 images and their gaps: tiled
    # narrow, 25 taps
    Case('out1x1', 'gf-2', 'ls-T', SYM2, 20, 24, 5, 5, 1, 1, 1, 3, 3, 3, True),
    # 64 -> 64 3x3 on 7x7, binary activations: the forward takes the matrix-core XNOR kernel; backward patch narrow, 9 taps
    Case('xnor64', 'ls-1', 'ls-1', SYM2, 64, 64, 3, 3, 1, 1, 1, 3, 7, 7, False),
    # the baseline's kernel at stride 2 with pad 0 (a full transposed convolution), ls-T weights: planes that cancel
    Case('s2_pad0', 'ls-2', 'ls-T', SYM15, 8, 16, 3, 3, 2, 0, 0, 2, 8, 7, False),
    # fp activations under the symmetric clamp on the wide patch kernel, 1x3 kernel with pad (0, 2)
    Case('k1x3_wide', 'fp', 'gf-3', SYM2, 72, 24, 1, 3, 1, 0, 2, 2, 4, 9, True),
]
BY_ID = {c.id: c for c in CASES}


# ----------------------------------------------------------------------------------------------------------- geometry
def planes(scheme: str) -> int:
    """Sign planes of a scheme (0 for fp)."""
    return int(scheme[3:]) if scheme.startswith('gf-') else {'fp': 0, 'ls-1': 1, 'ls-2': 2, 'ls-T': 2}[scheme]


def alpha_of(clamp: dict) -> float:
    return float(clamp.get('alpha', 2)) if clamp['kind'] == 'symmetric' else -1.0


def out_hw(c: Case):
    return (c.H + 2 * c.pad_h - c.KH) // c.stride + 1, (c.W + 2 * c.pad_w - c.KW) // c.stride + 1


def transposed_kernel(c: Case):
    """(kernel, wide, many) of lsq_signw_conv2d in the backward pass of ``c``: 'patch' or 'tiled'."""
    ho, wo = out_hw(c)
    hin, win = (ho, wo) if c.stride == 1 else (c.H + 2 * c.pad_h - c.KH + 1, c.W + 2 * c.pad_w - c.KW + 1)
    ph, pw = c.KH - 1 - c.pad_h, c.KW - 1 - c.pad_w
    hp, wp = hin + 2 * ph, win + 2 * pw
    assert (hp - c.KH + 1, wp - c.KW + 1) == (c.H, c.W)
    wide = c.C > 64                                   # out-channels of the transposed pass
    pbn = 128 if wide else 256                        # unit stride
    row_gap = wp - c.W
    img_gap = (hp - c.H) * wp
    patch = (pbn - 1) + ((pbn - 1) // c.W + 1) * max(row_gap, 0) + ((pbn - 1) // (c.H * c.W) + 1) * max(img_gap, 0) \
        + (c.KH - 1) * wp + (c.KW - 1) + 1
    plr = (patch + 127) // 128 * 128
    use_patch = plr <= 512 and (c.O + 15) // 16 * 16 <= 512          # (a pre-scale is always given)
    return ('patch' if use_patch else 'tiled'), wide, c.KH * c.KW > 9


def unread(c: Case):
    """(rows, columns) at the end of x that no tap of the forward reaches: (H + 2p - k) % stride beyond the padding."""
    ho, wo = out_hw(c)
    last_r = (ho - 1) * c.stride + c.KH - 1 - c.pad_h
    last_c = (wo - 1) * c.stride + c.KW - 1 - c.pad_w
    return max(0, c.H - 1 - last_r), max(0, c.W - 1 - last_c)


def kinds(c: Case) -> set:
    """The kinds of geometry the table must contain, as predicates of a case."""
    kern, wide, many = transposed_kernel(c)
    ho, wo = out_hw(c)
    fp_bare = c.xs == 'fp' and c.clamp['kind'] == 'identity'
    out = set()
    if (c.KH, c.KW, c.stride, c.pad_h, c.pad_w) == (3, 3, 1, 1, 1) and (kern, wide, many) == ('patch', False, False) and c.C < 64:
        out.add('baseline')
    if kern == 'patch' and wide and planes(c.ws) >= 2:
        out.add('wide_patch_two_planes')
    if c.O > 512 and kern == 'tiled' and not wide and planes(c.ws) == 3:
        out.add('o_above_512_tiled_narrow')
    if c.O > 512 and kern == 'tiled' and wide and (c.KH, c.KW, c.stride, c.pad_h, c.pad_w) == (1, 1, 2, 0, 0) and max(unread(c)) > 0:
        out.add('o_above_512_projection')
    if c.O <= 496 and kern == 'tiled' and c.W > 256:
        out.add('long_row')
    if kern == 'patch' and many:
        out.add('many_taps_wide' if wide else 'many_taps')
    if many and c.O == 1:
        out.add('single_out_channel')
    if many and c.pad_h == c.KH - 1 and c.pad_w == c.KW - 1:
        out.add('pad_k_minus_1')
    if max(c.KH, c.KW) == 8 and c.xs != 'fp':
        out.add('kernel_8')
    if (c.C, c.KH, c.KW, c.stride, c.pad_h, c.pad_w) == (3, 7, 7, 2, 3, 3) and c.xs == 'fp' and c.clamp['kind'] == 'symmetric':
        out.add('stem')
    if c.stride == 2 and c.KH != c.KW and (c.H + 2 * c.pad_h - c.KH) % 2 != (c.W + 2 * c.pad_w - c.KW) % 2:
        out.add('stride2_odd_even_nonsquare')
    if c.stride == 2 and c.KH % 2 == 0 and c.KW % 2 == 0 and c.pad_h != c.pad_w:
        out.add('stride2_even_kernel')
    if (ho, wo) == (1, 1) and c.N == 3:
        out.add('output_1x1')
    if (c.C, c.O, c.KH, c.KW, c.H, c.W) == (64, 64, 3, 3, 7, 7) and c.xs != 'fp':
        out.add('xnor_matrix_core_forward')
    if c.ws == 'ls-T':
        out.add('lsT_weights')
    if fp_bare:
        out.add('bare_transposed')
    if c.stride == 2 and c.pad_h == 0 and c.pad_w == 0 and c.KH > 1:
        out.add('pad0_full_transposed')
    return out


REQUIRED_KINDS = ('baseline', 'wide_patch_two_planes', 'o_above_512_tiled_narrow', 'o_above_512_projection', 'long_row',
                  'many_taps', 'many_taps_wide', 'single_out_channel', 'pad_k_minus_1', 'kernel_8', 'stem', 'stride2_odd_even_nonsquare',
                  'stride2_even_kernel', 'output_1x1', 'xnor_matrix_core_forward', 'lsT_weights', 'bare_transposed')


# ------------------------------------------------------------------------------------------------------------- inputs
def make_module(c: Case):
    """The case's QuantConv2d on the CPU in train mode, weight and bias from detgen."""
    from quant.binary.binary_conv import QuantConv2d
    conv = QuantConv2d(c.xs, c.ws, c.C, c.O, (c.KH, c.KW), dict(c.clamp), stride=c.stride, padding=(c.pad_h, c.pad_w),
                       bias=c.bias)
    d = inputs(c.id)
    with torch.no_grad():
        conv.weight.copy_(d['w'])
        if c.bias:
            conv.bias.copy_(d['b'])
    return conv.train()


def act_scales_cpu(c: Case, x: torch.Tensor) -> list:
    """The per-sample plane scales [kx] x [N] the torch formulation's activation quantizer computes for ``x`` (fp32, CPU)."""
    if c.xs == 'fp':
        return []
    import quant.binary.quantization as Q
    alpha = alpha_of(c.clamp)
    xc = x if alpha < 0 else Q.clamp_symmetric(x, alpha)
    if c.xs == 'ls-1':
        return [Q.quantizer_ls_1(xc)[0]]
    if c.xs == 'ls-2':
        return list(Q.quantizer_ls_2(xc)[:2])
    if c.xs == 'ls-T':
        v1 = Q.quantizer_ls_ternary(xc)[0]
        return [v1, v1]
    return list(Q.quantizer_gf(xc, planes(c.xs))[0])


@functools.lru_cache(maxsize=None)
def inputs(cid: str) -> dict:
    """CPU tensors of a case (nothing writes into them afterwards): x, w, b (or None), gy.  x holds +-0, +-alpha (on the clamp:
    inside it), +-1 (the edge |d| = 1 of the first sign's estimator) and, with two or more activation planes, in sample 0 the
    value e with |e - v_1[0]| = 1, the edge of the second sign's: 1 + v_1 where the clamp leaves that alone, else v_1 - 1 (when
    v_1 > 1).  v_1 depends on x, so the value is set and the scale recomputed a few times; where the GPU's scale differs from
    this one by an ulp the element sits an ulp off the edge instead, and the reference still decides it as the kernel does
    (from the scales of the step)."""
    c = BY_ID[cid]
    tag = f'tstep.{cid}'
    ho, wo = out_hw(c)
    x = detgen.normal(tag + '.x', (c.N, c.C, c.H, c.W), scale=1.2)
    flat = x.view(-1)
    flat[::11] = 0.0
    flat[3::13] = -0.0
    alpha = alpha_of(c.clamp)
    if alpha >= 0:
        flat[5::17] = alpha
        flat[7::19] = -alpha
    flat[2::31] = 1.0
    flat[4::37] = -1.0
    if planes(c.xs) >= 2:
        row0 = x[0].view(-1)
        for _ in range(6):
            v1 = float(act_scales_cpu(c, x)[0][0])
            e = 1.0 + v1 if alpha < 0 or 1.0 + v1 <= alpha else v1 - 1.0
            if e <= 0:
                break
            row0[9::23] = e
            row0[10::29] = -e
    fan = c.C * c.KH * c.KW
    w = detgen.normal(tag + '.w', (c.O, c.C, c.KH, c.KW), scale=1.5 * fan ** -0.5)
    b = detgen.normal(tag + '.b', (c.O,), scale=0.1) if c.bias else None
    gy = detgen.normal(tag + '.gy', (c.N, c.O, ho, wo))
    return {'x': x, 'w': w, 'b': b, 'gy': gy}


# ---------------------------------------------------------------------------------------------------- quantizer chain
def _decisions(x, scales, alpha):
    """The chain in the dtype of ``x``: (inside the clamp, clamped value c, chain value r, [d_i])."""
    inside = (x >= -alpha) & (x <= alpha) if alpha >= 0 else torch.ones_like(x, dtype=torch.bool)
    c = x.clamp(-alpha, alpha) if alpha >= 0 else x
    shape = (-1,) + (1,) * (x.dim() - 1)
    r, d = torch.zeros_like(c), []
    for v in scales:
        di = c - r
        d.append(di)
        r = r + v.view(shape) * torch.where(di >= 0, 1.0, -1.0)
    return inside, c, r, d


def chain(x, scales, alpha):
    """The quantizer chain in torch: value and the straight-through gradient's closed form (tests/test_training.py pins
    this formula to autograd through the reference-equal torch formulation)."""
    inside, c, r, d = _decisions(x, scales, alpha)
    shape = (-1,) + (1,) * (x.dim() - 1)

    def grad(g):
        G, acc = g.clone(), torch.zeros_like(g)
        for v, di in zip(reversed(scales), reversed(d)):
            t = torch.where(di.abs() <= 1, G * v.view(shape), torch.zeros_like(G))
            acc = acc + t
            G = G - t
        return torch.where(inside, acc if len(scales) else g, torch.zeros_like(g))
    return (r if len(scales) else c), grad


def chain64(x, scales, alpha):
    """``chain`` with every decision (d_i >= 0, |d_i| <= 1, inside the clamp) taken from the fp32 chain on fp32 ``x`` and
    ``scales``, and the value and the gradient's closed form computed from those decisions in fp64."""
    assert x.dtype == torch.float32 and all(v.dtype == torch.float32 for v in scales)
    inside, c, _, d = _decisions(x, scales, alpha)
    shape = (-1,) + (1,) * (x.dim() - 1)
    v64 = [v.double().view(shape) for v in scales]
    value = c.double()
    if scales:
        value = torch.zeros_like(value)
        for v, di in zip(v64, d):
            value = value + v * torch.where(di >= 0, 1.0, -1.0).double()
    is_open = [di.abs() <= 1 for di in d]

    def grad(g):
        assert g.dtype == torch.float64
        G, acc = g.clone(), torch.zeros_like(g)
        for v, op in zip(reversed(v64), reversed(is_open)):
            t = torch.where(op, G * v, torch.zeros_like(G))
            acc = acc + t
            G = G - t
        return torch.where(inside, acc if scales else g, torch.zeros_like(g))
    return value, grad


# ------------------------------------------------------------------------------------------------- the step in fp64
def step64(x, w, b, gy, xscales, wscales, alpha, stride, padding) -> dict:
    """One train step of QuantConv2d in fp64 on the CPU for given scales: ``xscales`` [kx][N] (an empty list or None: fp
    activations, the clamp alone), ``wscales`` [kw][O]; rows of x under the clamp ``alpha`` (-1: none), rows of w
    unclamped.  Returns y, gx, gw, gb and the magnitudes of the error bounds: mag_x, mag_w, m_x, m_w."""
    x, w, gy = x.detach().cpu().float(), w.detach().cpu().float(), gy.detach().cpu()
    xs = [] if xscales is None else [v.detach().cpu().float() for v in xscales]
    ws = [u.detach().cpu().float() for u in wscales]
    stride = (stride, stride) if isinstance(stride, int) else tuple(stride)
    padding = tuple(padding)
    xq, gradx = chain64(x, xs, alpha)
    wq, gradw = chain64(w, ws, -1.0)
    gy64 = gy.double()
    b64 = None if b is None else b.detach().cpu().double()
    y = torch.nn.functional.conv2d(xq, wq, b64, stride, padding)
    assert y.shape == gy64.shape, (y.shape, gy64.shape)
    gxq = torch.nn.grad.conv2d_input(x.shape, wq, gy64, stride, padding)
    gwq = torch.nn.grad.conv2d_weight(xq, w.shape, gy64, stride, padding)
    ones_w = torch.ones_like(wq)
    mag_x = torch.zeros_like(xq)
    for u in ws:                                      # one pass of the kernel per weight plane: planes that cancel still round
        mag_x = mag_x + torch.nn.grad.conv2d_input(x.shape, ones_w, gy64.abs() * u.double().view(1, -1, 1, 1), stride, padding)
    mag_w = torch.nn.grad.conv2d_weight(xq.abs(), w.shape, gy64.abs(), stride, padding)
    return {'y': y, 'gx': gradx(gxq), 'gw': gradw(gwq), 'gb': gy64.sum((0, 2, 3)), 'gxq': gxq, 'gwq': gwq,
            'mag_x': mag_x, 'mag_w': mag_w, 'm_x': gradx(torch.ones_like(xq)), 'm_w': gradw(torch.ones_like(wq))}
