"""Cases, inputs and the fp64 reference of lsq_signw_conv2d_half (include/lsq_hip_conv_half.h), shared by
tests/test_conv_half_host.py (the table against lsq_signw_conv2d_half_plan, the reference against an independent
restatement and against fp32 arithmetic) and tests/test_gpu_conv_half.py (the kernels).  Plain Python on the CPU; nothing
here touches a GPU.

Every case names the kernel it is there for (``plan``: the bits lsq_signw_conv2d_half_plan returns); the host test asserts
that the library agrees.  ``fp32_patch`` restates patch_plan (csrc/lsq_signw_conv_core.h), the one rule by which both
lsq_signw_conv2d and lsq_signw_conv2d_half choose between their patch and tiled kernels, without a pre-scale -- independently,
in Python: it is the check on that function.  Where it is true lsq_signw_conv2d takes its patch kernel or its 3x3 fast path,
the two paths DESIGN 4.4 states to be bit-identical.

Sizes.  The patch of a workgroup is bounded for its full tile of pixels, whatever the batch: at stride 2 x 2 the 128 pixels
of a NARROW tile (O / groups <= 64) need 254 entries for the pixels and (127 // Wo + 1) row gaps of 2 (Wp - Wo) entries.  Over
13 x 12 with pad 1 that is 254 + 22 * 16 entries, past the 640 the kernel holds, and the call takes the general kernel; over
13 x 7 (Wp = 9, Wo = 4) it is 254 + 32 * 10 + 5 image gaps of 9 + 21 for the taps = 640 exactly, so the narrow stride-2 x 2
patch case runs over 13 x 7, and its many-taps variant (2x5, ten taps) over 6 x 17.  The stride-(2, 1) cases over 13 x 12 are
extras.  The general kernel's wide case needs a row of 600 pixels: a shorter one fits the patch.
"""

import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import detgen
from oracle import ref_port as P

PATCH, WIDE, UNIT, MANY = 1, 2, 4, 8              # LSQ_CONV_HALF_* of include/lsq_hip_conv_half.h
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
ALPHAS = (-1.0, 2.0, 1.3)     # identity, a bound both types hold, a bound neither holds (bf16: 1.296875, fp16: 1.2998046875)

Case = collections.namedtuple('Case', 'id N C H W O KH KW stride pad dil groups ws alpha bias plan')

CASES = [
    # 3 x 64 x 9 x 9 -> 20, 3x3, pad 1: 243 pixels fill no tile of 256; four chunks of one weight word (bits 0, 16, 32, 48)
    Case('p1_narrow', 3, 64, 9, 9, 20, 3, 3, (1, 1), (1, 1), (1, 1), 1, 'ls-1', 0, True, PATCH | UNIT),
    # C = 72 -> O = 70, two planes: a last chunk of 8 channels in the second weight word, O % 16 = 6, 162 pixels = a full tile
    # of 128 over two samples and a partial one
    Case('p1_wide', 2, 72, 9, 9, 70, 3, 3, (1, 1), (1, 1), (1, 1), 1, 'ls-2', 1, False, PATCH | UNIT | WIDE),
    # stride 2 over 13 x 12 with pad 1, wide: the last padded column is never read
    Case('s2_wide', 2, 20, 13, 12, 70, 3, 3, (2, 2), (1, 1), (1, 1), 1, 'ls-T', 2, True, PATCH | WIDE),
    # the narrow strided tile at stride 2 x 2: 13 x 7 with pad 1 (see "Sizes" above), 140 pixels = a full tile of 128 over
    # five samples and a partial one
    Case('s2_narrow', 5, 20, 13, 7, 24, 3, 3, (2, 2), (1, 1), (1, 1), 1, 'ls-2', 1, True, PATCH),
    # the same tile with ten taps (2x5: a tap group of one after the nine) over 6 x 17
    Case('k2x5_s2_narrow', 5, 20, 6, 17, 24, 2, 5, (2, 2), (1, 1), (1, 1), 1, 'ls-1', 0, False, PATCH | MANY),
    # extras: the narrow strided tile at stride (2, 1) over 13 x 12
    Case('s21_narrow', 2, 20, 13, 12, 24, 3, 3, (2, 1), (1, 1), (1, 1), 1, 'gf-3', 0, False, PATCH),
    # 3x3 stride 2 without padding over 12 x 12: the last row and column of x itself are never read
    Case('s2_pad0', 2, 8, 12, 12, 130, 3, 3, (2, 2), (0, 0), (1, 1), 1, 'ls-1', 1, True, PATCH | WIDE),
    # 25 taps: three tap groups, narrow and wide
    Case('k5_narrow', 2, 20, 16, 16, 50, 5, 5, (1, 1), (2, 2), (1, 1), 1, 'ls-T', 2, False, PATCH | UNIT | MANY),
    Case('k5_wide', 1, 20, 12, 12, 70, 5, 5, (1, 1), (2, 2), (1, 1), 1, 'ls-1', 0, True, PATCH | UNIT | WIDE | MANY),
    # more than 9 taps on the strided tiles: 5x5 stride 2 (wide), 4x3 stride (2, 1) (narrow, 12 taps: a group of 3 after 9)
    Case('k5_s2_wide', 2, 16, 13, 12, 70, 5, 5, (2, 2), (2, 2), (1, 1), 1, 'ls-2', 1, False, PATCH | WIDE | MANY),
    Case('k4x3_s21', 2, 20, 13, 12, 24, 4, 3, (2, 1), (1, 1), (1, 1), 1, 'ls-1', 2, True, PATCH | MANY),
    # a non-square 1x3 kernel with per-axis padding (0, 2)
    Case('k1x3', 2, 72, 4, 9, 24, 1, 3, (1, 1), (0, 2), (1, 1), 1, 'gf-3', 1, True, PATCH | UNIT),
    # a row of 260 pixels: two rows of taps are 524 entries apart -> the general kernel, narrow; C = 8: half a chunk
    Case('long_row', 1, 8, 2, 260, 16, 3, 3, (1, 1), (1, 1), (1, 1), 1, 'ls-2', 2, True, 0),
    # 1x1 stride 2 over a row of 600: the general kernel, wide; 40 channels = one chunk of 32 and one of 8, O = 130 = two
    # out-channel tiles (the second of 2 rows), the last row of x (H = 4) is never read
    Case('proj_wide', 1, 40, 4, 600, 130, 1, 1, (2, 2), (0, 0), (1, 1), 1, 'ls-1', 0, False, WIDE),
    # groups = 2 with dilation 2 (12 channels and 20 out-channels a group)
    Case('groups_dil', 2, 24, 10, 10, 40, 3, 3, (1, 1), (2, 2), (2, 2), 2, 'ls-2', 1, True, 0),
    # groups = 3 on the patch kernel, wide: 66 out-channels a group, padded to 80 in the planes
    Case('groups3_patch', 1, 48, 8, 8, 198, 3, 3, (1, 1), (1, 1), (1, 1), 3, 'ls-1', 2, False, PATCH | UNIT | WIDE),
    # 1 x 1 output (H = k - 2 p), three samples: every pixel is its own sample
    Case('out1x1', 3, 20, 3, 3, 24, 5, 5, (1, 1), (1, 1), (1, 1), 1, 'gf-3', 0, True, 0),
    # depthwise: one channel a group
    Case('cg1', 2, 6, 7, 7, 12, 3, 3, (1, 1), (1, 1), (1, 1), 6, 'ls-1', 1, True, PATCH | UNIT),
    # eight planes: one launch each, the workspace route for a 16-bit y; on a patch and on the general kernel
    Case('gf8_patch', 2, 16, 6, 6, 10, 3, 3, (1, 1), (1, 1), (1, 1), 1, 'gf-8', 2, True, PATCH | UNIT),
    Case('gf8_general', 1, 16, 2, 260, 10, 3, 3, (1, 1), (1, 1), (1, 1), 1, 'gf-8', 1, False, 0),
]
BY_ID = {c.id: c for c in CASES}


# ----------------------------------------------------------------------------------------------------------- geometry
def planes(scheme: str) -> int:
    """Sign planes of a weight scheme."""
    return int(scheme[3:]) if scheme.startswith('gf-') else {'ls-1': 1, 'ls-2': 2, 'ls-T': 2}[scheme]


def out_hw(c: Case):
    return ((c.H + 2 * c.pad[0] - c.dil[0] * (c.KH - 1) - 1) // c.stride[0] + 1,
            (c.W + 2 * c.pad[1] - c.dil[1] * (c.KW - 1) - 1) // c.stride[1] + 1)


def tile_pixels(c: Case) -> int:
    """Output pixels per workgroup of the patch kernel (both libraries)."""
    wide, unit = c.O // c.groups > 64, c.stride == (1, 1)
    return (128 if wide else 256) if unit else (64 if wide else 128)


def fp32_patch(c: Case) -> bool:
    """True where lsq_signw_conv2d, called without a pre-scale, takes its patch kernel or 3x3 fast path for ``c``: patch_plan
    of csrc/lsq_signw_conv_core.h, restated."""
    ho, wo = out_hw(c)
    hp, wp = c.H + 2 * c.pad[0], c.W + 2 * c.pad[1]
    pbn = tile_pixels(c)
    pmax = 512 if c.stride == (1, 1) else 640
    row_gap = c.stride[0] * wp - wo * c.stride[1]
    img_gap = (hp - ho * c.stride[0]) * wp
    patch = (pbn - 1) * c.stride[1] + ((pbn - 1) // wo + 1) * max(row_gap, 0) + ((pbn - 1) // (ho * wo) + 1) * max(img_gap, 0) \
        + (c.KH - 1) * c.dil[0] * wp + (c.KW - 1) * c.dil[1] + 1
    return (patch + 127) // 128 * 128 <= pmax          # (the 2^30 / 2^31 index limits are far from every case here)


def unread(c: Case):
    """(rows, columns) at the end of x that no tap reaches."""
    ho, wo = out_hw(c)
    last_r = (ho - 1) * c.stride[0] + (c.KH - 1) * c.dil[0] - c.pad[0]
    last_c = (wo - 1) * c.stride[1] + (c.KW - 1) * c.dil[1] - c.pad[1]
    return max(0, c.H - 1 - last_r), max(0, c.W - 1 - last_c)


def kinds(c: Case) -> set:
    """The kinds of call the table must contain, as predicates of a case."""
    ho, wo = out_hw(c)
    cg, og = c.C // c.groups, c.O // c.groups
    patch, wide, unit, many = bool(c.plan & PATCH), bool(c.plan & WIDE), bool(c.plan & UNIT), bool(c.plan & MANY)
    pixels = c.N * ho * wo
    out = set()
    if patch:
        out.add('patch_' + ('unit' if unit else 'strided') + ('_wide' if wide else '_narrow') + ('_many' if many else ''))
    else:
        out.add('general_wide' if wide else 'general_narrow')
    if (c.N, c.C, c.H, c.W, c.O, c.KH, c.KW, c.pad) == (3, 64, 9, 9, 20, 3, 3, (1, 1)) and patch and unit and not wide:
        out.add('baseline_3x64x9x9')
    if patch and unit and wide and cg % 16 == 8 and cg > 64 and og % 16 and planes(c.ws) == 2:
        out.add('wide_ragged_two_planes')
    if patch and not unit and not wide and c.stride == (2, 2):
        out.add('patch_strided_narrow_s2x2' + ('_many' if many else ''))
    if patch and c.stride == (2, 2) and (c.H, c.W, c.pad) == (13, 12, (1, 1)):
        out.add('stride2_13x12')
    if patch and not unit and max(unread(c)) > 0 and min(unread(c)) > 0:
        out.add('strided_rows_and_columns_unread')
    if patch and many and (c.KH, c.KW, c.pad, c.H, c.W) == (5, 5, (2, 2), 16, 16):
        out.add('k5_on_16x16')
    if patch and many and (c.KH * c.KW) % 9:
        out.add('last_tap_group_partial')
    if (c.KH, c.KW, c.pad) == (1, 3, (0, 2)):
        out.add('k1x3_pad_0_2')
    if not patch and not wide and c.W == 260 and c.C == 8 and c.O == 16:
        out.add('row_of_260')
    if not patch and wide and (c.KH, c.KW, c.stride, c.C, c.O) == (1, 1, (2, 2), 40, 130):
        out.add('projection_40_130')
    if c.groups == 2 and c.dil == (2, 2):
        out.add('groups_dilation')
    if c.groups > 1 and patch:
        out.add('groups_patch')
    if (ho, wo) == (1, 1) and c.N == 3 and c.H == c.KH - 2 * c.pad[0]:
        out.add('out_1x1')
    if cg == 1:
        out.add('cg_1')
    if patch and pixels < tile_pixels(c):
        out.add('fills_no_tile')
    if patch and pixels > tile_pixels(c) and ho * wo < tile_pixels(c):
        out.add('samples_share_a_tile')
    if cg >= 64:
        out.add('every_16_bits_of_a_word')
    out.add({'ls-1': 'planes_ls1', 'ls-2': 'planes_ls2', 'ls-T': 'planes_lsT'}.get(c.ws, 'planes_' + c.ws.replace('-', '')))
    if planes(c.ws) == 8:
        out.add('eight_planes_patch' if patch else 'eight_planes_general')
    out.add(('clamp_identity', 'clamp_exact', 'clamp_rounded')[c.alpha])
    out.add('bias' if c.bias else 'no_bias')
    return out


REQUIRED_KINDS = {
    'patch_unit_narrow', 'patch_unit_wide', 'patch_strided_narrow', 'patch_strided_wide',
    'patch_unit_narrow_many', 'patch_unit_wide_many', 'patch_strided_narrow_many', 'patch_strided_wide_many',
    'patch_strided_narrow_s2x2', 'patch_strided_narrow_s2x2_many', 'general_narrow', 'general_wide',
    'baseline_3x64x9x9', 'wide_ragged_two_planes', 'stride2_13x12', 'strided_rows_and_columns_unread', 'k5_on_16x16',
    'last_tap_group_partial', 'k1x3_pad_0_2', 'row_of_260', 'projection_40_130', 'groups_dilation', 'groups_patch', 'out_1x1',
    'cg_1', 'fills_no_tile', 'samples_share_a_tile', 'every_16_bits_of_a_word',
    'planes_ls1', 'planes_ls2', 'planes_lsT', 'planes_gf3', 'planes_gf8', 'eight_planes_patch', 'eight_planes_general',
    'clamp_identity', 'clamp_exact', 'clamp_rounded', 'bias', 'no_bias',
}


# ------------------------------------------------------------------------------------------------------------- inputs
def alpha_in(alpha: float, dtype: torch.dtype) -> float:
    """The bound as Tensor.clamp rounds it into ``dtype``: what the caller of the kernel passes."""
    return float(torch.tensor(alpha, dtype=dtype)) if alpha >= 0 else alpha


@functools.lru_cache(maxsize=None)
def weights(cid: str):
    """(w fp32 [O, C / groups, KH, KW], scales [kw, O] of the planes lsq_pack_weight writes, the oracle's scale list, bias)."""
    c = BY_ID[cid]
    w = detgen.uniform(f'convhalf.w.{cid}', (c.O, c.C // c.groups, c.KH, c.KW), -0.5, 0.5)
    sc = P.weight_scales(w, c.ws)
    wsc = torch.stack([sc[0], sc[0]] if c.ws == 'ls-T' else list(sc)).contiguous()       # ls-T: two planes of one scale
    b = detgen.normal(f'convhalf.b.{cid}', (c.O,), scale=0.5) if c.bias else None
    return w, wsc, sc, b


@functools.lru_cache(maxsize=None)
def batch(cid: str, dt: str) -> torch.Tensor:
    c = BY_ID[cid]
    return detgen.normal(f'convhalf.x.{cid}', (c.N, c.C, c.H, c.W), scale=1.2).to(DTYPES[dt])


def clamped(cid: str, dt: str) -> torch.Tensor:
    """The batch as Tensor.clamp leaves it (the bound rounded into the type), still 16-bit."""
    c, x = BY_ID[cid], batch(cid, dt)
    a = ALPHAS[c.alpha]
    xc = x.clamp(-a, a) if a >= 0 else x
    assert xc.dtype == x.dtype
    return xc


@functools.lru_cache(maxsize=None)
def reference(cid: str, dt: str) -> torch.Tensor:
    """fp64: F.conv2d(x16.clamp(+-a).double(), w_q.double(), bias.double(), ...)."""
    c = BY_ID[cid]
    w, _, sc, b = weights(cid)
    wq = P.quantize_weight(w, c.ws, sc)
    return F.conv2d(clamped(cid, dt).double(), wq.double(), None if b is None else b.double(), c.stride, c.pad, c.dil, c.groups)


def im2col64(x, w, b, c: Case):
    """y[n, o, ho, wo] = b[o] + sum over (channel of o's group, kh, kw) of xpad[n, ch, ho s + kh d, wo s + kw d] w[o, ch, kh, kw]
    in fp64 (numpy arrays), tap by tap with strided slices: no convolution routine."""
    ho, wo = out_hw(c)
    cg, og = c.C // c.groups, c.O // c.groups
    xp = np.zeros((c.N, c.C, c.H + 2 * c.pad[0], c.W + 2 * c.pad[1]))
    xp[:, :, c.pad[0]:c.pad[0] + c.H, c.pad[1]:c.pad[1] + c.W] = x
    y = np.zeros((c.N, c.O, ho, wo))
    for g in range(c.groups):
        for kh in range(c.KH):
            for kw in range(c.KW):
                r0, c0 = kh * c.dil[0], kw * c.dil[1]
                win = xp[:, g * cg:(g + 1) * cg, r0:r0 + (ho - 1) * c.stride[0] + 1:c.stride[0],
                         c0:c0 + (wo - 1) * c.stride[1] + 1:c.stride[1]]
                y[:, g * og:(g + 1) * og] += np.einsum('nchw,oc->nohw', win, w[g * og:(g + 1) * og, :, kh, kw])
    return y if b is None else y + b[None, :, None, None]
