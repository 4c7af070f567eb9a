"""Cases, inputs and the fp64 reference of QuantConv2d's input gradient on its own kernel (lsq_signw_conv2d_dgrad,
quant/binary/hip_train.py with DGRAD_KERNEL), shared by tests/test_conv_dgrad_host.py (the plan, the reference against fp32
autograd through the torch formulation, the conditions the table must meet) and tests/test_gpu_conv_dgrad.py (the kernel and
the step).  Plain Python on the CPU; nothing here touches a GPU.

The table is the 17 cases of tests/golden/train_step_cases.py (same ids, same tensors: ``inputs`` hands out that module's)
lifted into a ``Case`` with per-axis strides, dilation and groups, plus the smallest shapes at which the kernel can go wrong
where the old route did not go at all.  ``step64`` is train_step_cases.step64 with dilation and groups; the quantizer chain
(``chain64``) is that module's.

``classes`` restates the residue classes of the kernel: pixel (h, w) belongs to class ((h + pad_h) % stride_h,
(w + pad_w) % stride_w) and tap (i, j) reaches only class ((i dil_h) % stride_h, (j dil_w) % stride_w).
"""

import collections
import functools

import torch

import detgen
import train_step_cases as T

Case = collections.namedtuple('Case', 'id xs ws clamp C O KH KW stride_h stride_w pad_h pad_w dil_h dil_w groups N H W bias')

IDENT, SYM2, SYM15 = T.IDENT, T.SYM2, T.SYM15


def _lift(c) -> Case:
    return Case(c.id, c.xs, c.ws, c.clamp, c.C, c.O, c.KH, c.KW, c.stride, c.stride, c.pad_h, c.pad_w, 1, 1, 1, c.N, c.H, c.W, c.bias)


LIFTED = [_lift(c) for c in T.CASES]

NEW = [
    # groups 2 with cg = 36, og = 20: padded out-channel slots (20 -> 32 a group) and a channel tail (36 of the 64-tile)
    Case('g2_tails', 'ls-1', 'ls-2', SYM2, 72, 40, 3, 3, 1, 1, 1, 1, 1, 1, 2, 2, 6, 5, True),
    # depthwise: groups = C = O = 24, K = 1 out-channel a group
    Case('depthwise', 'ls-2', 'ls-1', SYM2, 24, 24, 3, 3, 1, 1, 1, 1, 1, 1, 24, 2, 7, 6, False),
    # groups 3 with cg = 66 on the wide tile, stride 2, ls-T weights (planes that cancel)
    Case('g3_wide_s2', 'fp', 'ls-T', IDENT, 198, 48, 3, 3, 2, 2, 1, 1, 1, 1, 3, 2, 9, 8, True),
    # dilation 2, pad 2
    Case('dil2', 'ls-1', 'ls-1', SYM2, 8, 16, 3, 3, 1, 1, 2, 2, 2, 2, 1, 2, 9, 8, False),
    # dilation (2, 1) with stride 2: every row tap has (2 i) % 2 == 0, so the row class 1 is dead: rows with h + pad_h odd are 0
    Case('dil2x1_s2', 'fp', 'ls-2', SYM2, 8, 16, 3, 3, 2, 2, 2, 1, 2, 1, 1, 2, 10, 9, True),
    # stride 3 under 3 x 3: nine classes of one tap each
    Case('s3_3x3', 'ls-2', 'ls-1', SYM2, 8, 16, 3, 3, 3, 3, 1, 1, 1, 1, 1, 2, 10, 11, False),
    # stride 3 under 2 x 2: residues {0, 1} x {0, 1} are live, five classes are dead
    Case('s3_2x2', 'ls-1', 'ls-2', SYM15, 8, 16, 2, 2, 3, 3, 0, 0, 1, 1, 1, 2, 8, 9, True),
    # non-square strides
    Case('s2x1', 'fp', 'ls-1', IDENT, 8, 16, 3, 3, 2, 1, 1, 1, 1, 1, 1, 2, 9, 6, False),
    Case('s1x2', 'ls-T', 'ls-1', SYM2, 8, 16, 3, 3, 1, 2, 1, 1, 1, 1, 1, 2, 6, 9, True),
    # padding above k - 1
    Case('pad3x1', 'ls-1', 'ls-1', SYM2, 8, 16, 3, 3, 1, 1, 3, 1, 1, 1, 1, 2, 6, 5, True),
    Case('pad0x3', 'fp', 'ls-2', IDENT, 8, 16, 3, 3, 1, 1, 0, 3, 1, 1, 1, 2, 6, 5, False),
    # C = O = 130 with gf-3 weights: three words of o with a tail of 2, two 128-channel tiles (the second of 2 channels),
    # three planes in one accumulator
    Case('c130_gf3', 'fp', 'gf-3', SYM2, 130, 130, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 5, 4, False),
    # C = O = 1 on a 1 x 1 image: a single product
    Case('one', 'fp', 'ls-1', IDENT, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1, True),
    # H = 1 at stride 2: the row class 1 has no pixels
    Case('h1_s2', 'ls-1', 'ls-1', SYM2, 8, 16, 1, 3, 2, 2, 0, 1, 1, 1, 1, 2, 1, 8, False),
]

CASES = LIFTED + NEW
BY_ID = {c.id: c for c in CASES}
NEW_IDS = tuple(c.id for c in NEW)

planes, alpha_of, chain64, act_scales_cpu = T.planes, T.alpha_of, T.chain64, T.act_scales_cpu


# ----------------------------------------------------------------------------------------------------------- geometry
def out_hw(c: Case):
    return ((c.H + 2 * c.pad_h - c.dil_h * (c.KH - 1) - 1) // c.stride_h + 1,
            (c.W + 2 * c.pad_w - c.dil_w * (c.KW - 1) - 1) // c.stride_w + 1)


def conv_args(c: Case):
    """(stride, padding, dilation, groups) as torch takes them."""
    return (c.stride_h, c.stride_w), (c.pad_h, c.pad_w), (c.dil_h, c.dil_w), c.groups


def classes(c: Case) -> dict:
    """{(rh, rw): number of taps that reach the class} over all stride_h * stride_w classes, tap by tap."""
    out = {(rh, rw): 0 for rh in range(c.stride_h) for rw in range(c.stride_w)}
    for i in range(c.KH):
        for j in range(c.KW):
            out[((i * c.dil_h) % c.stride_h, (j * c.dil_w) % c.stride_w)] += 1
    return out


def class_pixels(c: Case, rh: int, rw: int) -> int:
    """Pixels of one sample in class (rh, rw)."""
    return (sum(1 for h in range(c.H) if (h + c.pad_h) % c.stride_h == rh)
            * sum(1 for w in range(c.W) if (w + c.pad_w) % c.stride_w == rw))


def wide(c: Case) -> bool:
    return c.C // c.groups > 64


MAX_PATCH_POSITIONS = 222           # staged positions of the patch kernel (two LDS row sets of 144 bytes a position in 64 KiB)


def patch_positions(c: Case):
    """The patch rule of lsq_signw_conv2d_dgrad restated: the fewest positions (NS samples x (TH + dH) x (TW + dW), NS TH TW =
    128 in powers of two) a tile's taps read in the class with the most taps, over every split; None when no split stays
    within MAX_PATCH_POSITIONS (the gather kernel).  dH = the spread of that class's row shifts (h0 + pad_h - i dil_h) / stride_h."""
    import math
    per_h, per_w = c.stride_h // math.gcd(c.dil_h, c.stride_h), c.stride_w // math.gcd(c.dil_w, c.stride_w)
    dh = (c.KH - 1) // per_h * per_h * c.dil_h // c.stride_h
    dw = (c.KW - 1) // per_w * per_w * c.dil_w // c.stride_w
    fits = [(128 >> (lw + lh)) * ((1 << lh) + dh) * ((1 << lw) + dw) for lw in range(8) for lh in range(8 - lw)]
    fits = [n for n in fits if n <= MAX_PATCH_POSITIONS]
    return min(fits) if fits else None


def kinds(c: Case) -> set:
    """The kinds of geometry the table must contain, as predicates of a case."""
    cg, og = c.C // c.groups, c.O // c.groups
    cl = classes(c)
    dead = sum(1 for n in cl.values() if n == 0)
    out = set()
    if c.groups == 2 and og % 16 and cg % 64 and cg < 64:
        out.add('groups_padded_slots_channel_tail')
    if c.groups == c.C == c.O and c.groups > 1:
        out.add('depthwise')
    if c.groups == 3 and cg > 64 and cg % 64 and (c.stride_h, c.stride_w) == (2, 2) and c.ws == 'ls-T':
        out.add('groups_wide_stride2_ternary')
    if (c.dil_h, c.dil_w, c.pad_h, c.pad_w) == (2, 2, 2, 2):
        out.add('dilation2_pad2')
    if (c.dil_h, c.dil_w) == (2, 1) and (c.stride_h, c.stride_w) == (2, 2) and dead == 2 and c.H > 4:
        out.add('dilation_kills_a_row_class')
    if (c.stride_h, c.stride_w, c.KH, c.KW) == (3, 3, 3, 3) and set(cl.values()) == {1}:
        out.add('stride3_nine_single_tap_classes')
    if (c.stride_h, c.stride_w, c.KH, c.KW) == (3, 3, 2, 2) and dead == 5:
        out.add('stride3_five_dead_classes')
    if (c.stride_h, c.stride_w) == (2, 1):
        out.add('stride_2x1')
    if (c.stride_h, c.stride_w) == (1, 2):
        out.add('stride_1x2')
    if (c.KH, c.KW) == (3, 3) and c.pad_h > c.KH - 1 and (c.dil_h, c.dil_w) == (1, 1):
        out.add('pad_above_k_minus_1_rows')
    if (c.KH, c.KW) == (3, 3) and c.pad_w > c.KW - 1 and c.pad_h == 0 and (c.dil_h, c.dil_w) == (1, 1):
        out.add('pad_above_k_minus_1_columns')
    if c.C == c.O == 130 and c.ws == 'gf-3' and c.groups == 1:
        out.add('c130_three_planes')
    if (c.C, c.O, c.H, c.W, c.KH, c.KW, c.N) == (1, 1, 1, 1, 1, 1, 1):
        out.add('single_product')
    if c.H == 1 and c.stride_h == 2 and any(class_pixels(c, rh, rw) == 0 for rh, rw in cl):
        out.add('class_without_pixels')
    if c.W == 260 and c.H == 3:
        out.add('long_row')
    if c.N * c.H * c.W > 2 * 128 and (c.stride_h, c.stride_w) == (1, 1):
        out.add('several_pixel_tiles')
    if c.O // c.groups > 64:
        out.add('several_out_channel_words')
    out.add(('wide' if wide(c) else 'narrow') + ('_patch' if patch_positions(c) is not None else '_gather'))
    return out


REQUIRED_KINDS = ('groups_padded_slots_channel_tail', 'depthwise', 'groups_wide_stride2_ternary', 'dilation2_pad2',
                  'dilation_kills_a_row_class', 'stride3_nine_single_tap_classes', 'stride3_five_dead_classes', 'stride_2x1',
                  'stride_1x2', 'pad_above_k_minus_1_rows', 'pad_above_k_minus_1_columns', 'c130_three_planes', 'single_product',
                  'class_without_pixels', 'long_row', 'several_pixel_tiles', 'several_out_channel_words', 'wide_patch', 'narrow_patch',
                  'wide_gather', 'narrow_gather')


# ------------------------------------------------------------------------------------------------------------- inputs
def make_module(c: Case):
    """The case's QuantConv2d on the CPU in train mode, weight and bias from ``inputs``."""
    from quant.binary.binary_conv import QuantConv2d
    stride, padding, dilation, groups = conv_args(c)
    conv = QuantConv2d(c.xs, c.ws, c.C, c.O, (c.KH, c.KW), dict(c.clamp), stride=stride, padding=padding, dilation=dilation,
                       groups=groups, bias=c.bias)
    d = inputs(c.id)
    with torch.no_grad():
        conv.weight.copy_(d['w'])
        if c.bias:
            conv.bias.copy_(d['b'])
    return conv.train()


@functools.lru_cache(maxsize=None)
def inputs(cid: str) -> dict:
    """CPU tensors of a case (nothing writes into them afterwards): x, w, b (or None), gy.  A lifted case has the tensors of
    train_step_cases.inputs; a new one is made by the same recipe (+-0, +-alpha, +-1 and the edge of the second sign in x)
    with a weight of [O, C / groups, KH, KW]."""
    if cid in T.BY_ID:
        return T.inputs(cid)
    c = BY_ID[cid]
    tag = f'cdgrad.{cid}'
    ho, wo = out_hw(c)
    x = detgen.normal(tag + '.x', (c.N, c.C, c.H, c.W), scale=1.2)
    flat = x.view(-1)
    alpha = alpha_of(c.clamp)
    if flat.numel() >= 64:                            # (the single-product case keeps its one random value)
        flat[::11] = 0.0
        flat[3::13] = -0.0
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
    cg = c.C // c.groups
    fan = cg * c.KH * c.KW
    w = detgen.normal(tag + '.w', (c.O, cg, c.KH, c.KW), scale=1.5 * fan ** -0.5)
    b = detgen.normal(tag + '.b', (c.O,), scale=0.1) if c.bias else None
    gy = detgen.normal(tag + '.gy', (c.N, c.O, ho, wo))
    return {'x': x, 'w': w, 'b': b, 'gy': gy}


# ------------------------------------------------------------------------------------------------- the step in fp64
def step64(c: Case, x, w, b, gy, xscales, wscales) -> dict:
    """train_step_cases.step64 with the case's dilation and groups: one train step of QuantConv2d in fp64 on the CPU for
    given scales (``xscales`` [kx][N], empty or None for fp activations; ``wscales`` [kw][O]).  Returns y, gx, gw, gb, gxq,
    gwq and the magnitudes of the error bounds: mag_x = sum_q conv2d_input(ones, |gy| u_q), mag_w, m_x, m_w."""
    from torch.nn.grad import conv2d_input, conv2d_weight
    alpha = alpha_of(c.clamp)
    stride, padding, dilation, groups = conv_args(c)
    x, w, gy = x.detach().cpu().float(), w.detach().cpu().float(), gy.detach().cpu()
    xs = [] if xscales is None else [v.detach().cpu().float() for v in xscales]
    ws = [u.detach().cpu().float() for u in wscales]
    xq, gradx = chain64(x, xs, alpha)
    wq, gradw = chain64(w, ws, -1.0)
    gy64 = gy.double()
    b64 = None if b is None else b.detach().cpu().double()
    y = torch.nn.functional.conv2d(xq, wq, b64, stride, padding, dilation, groups)
    assert y.shape == gy64.shape, (y.shape, gy64.shape)
    gxq = conv2d_input(x.shape, wq, gy64, stride, padding, dilation, groups)
    gwq = conv2d_weight(xq, w.shape, gy64, stride, padding, dilation, groups)
    ones_w = torch.ones_like(wq)
    mag_x = torch.zeros_like(xq)
    for u in ws:                                      # every plane's products round, also where the planes cancel
        mag_x = mag_x + conv2d_input(x.shape, ones_w, gy64.abs() * u.double().view(1, -1, 1, 1), stride, padding, dilation, groups)
    mag_w = conv2d_weight(xq.abs(), w.shape, gy64.abs(), stride, padding, dilation, groups)
    return {'y': y, 'gx': gradx(gxq), 'gw': gradw(gwq), 'gb': gy64.sum((0, 2, 3)), 'gxq': gxq, 'gwq': gwq,
            'mag_x': mag_x, 'mag_w': mag_w, 'm_x': gradx(torch.ones_like(xq)), 'm_w': gradw(torch.ones_like(wq))}
