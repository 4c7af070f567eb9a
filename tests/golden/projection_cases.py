"""Cases and launch arithmetic of the projection-shortcut tests, shared by tests/test_projection_cases_host.py (which proves on
the host what the cases reach), tests/test_gpu_pointwise_variants.py (lsq_pointwise_conv) and tests/test_gpu_proj_fused.py
(lsq_xnor_conv2d_proj).

A GPU test cannot observe which kernel instantiation a call launched.  ``pointwise_variant`` and ``proj_grid`` therefore RESTATE
the host-side selection code of the two entry points, and the host test holds every case to the variant it was chosen for: that
mirror is the evidence of coverage.  When the selection code changes, these two functions change with it, and the host test
says which cases no longer reach their variant.

Exact operands: ``grid_operands`` gives integer-valued fp32 tensors.  With x in [-8, 8], w in [-4, 4], bias in [-16, 16] and at
most 512 channels every partial sum of sum_c w x + b is an integer of magnitude at most 8 * 4 * 512 + 16 < 2^15, far below 2^24:
every fp32 fma of the chain is exact whatever the order, and the fp64 result cast to fp32 is THE answer.  The comparison is
torch.equal, and it does not have to reproduce the matrix core's summation order."""

import detgen

X_RANGE, W_RANGE, B_RANGE = (-8, 8), (-4, 4), (-16, 16)
MAX_CHANNELS = 512
MAX_TENSOR_BYTES = 64 << 20


def grid_operands(tag: str, shape, lo: int, hi: int):
    """Integer-valued fp32 tensor in [lo, hi] from detgen's seeded generator (uniform, rounded)."""
    return detgen.uniform(tag, shape, float(lo), float(hi)).round()


def out_size(size: int, stride: int) -> int:
    """Output rows / columns of a 1x1 convolution without padding."""
    return (size - 1) // stride + 1


# ------------------------------------------------------------------------------------------------------ lsq_pointwise_conv
def generic_routes(n, c, h, w, o, stride) -> frozenset:
    """Which conditions of lsq_pointwise_conv's `if (n_ot <= 8 && (n_ot & (n_ot - 1)) == 0 && pair_ok)` fail (csrc/lsq_pointwise.hip,
    the entry point, lines 313-315): any of 'o_gt_512', 'not_pow2', 'pair_refused'.  Empty: pointwise_all_kernel serves the call."""
    n_ot = o // 64
    wo = out_size(w, stride)
    pair_ok = stride != 2 or (wo & 1) == 1 or (w & 1) == 0
    out = set()
    if n_ot > 8:
        out.add('o_gt_512')
    if n_ot & (n_ot - 1):
        out.add('not_pow2')
    if not pair_ok:
        out.add('pair_refused')
    return frozenset(out)


def pointwise_variant(n, c, h, w, o, stride):
    """The kernel lsq_pointwise_conv launches for x [n, c, h, w] -> o channels: ('all', NOT, PAIRS, VEC4) for
    pointwise_all_kernel<NOT, PAIRS, VEC4>, or ('generic',) for pointwise_conv_kernel.

    Mirrors device-side selection code, csrc/lsq_pointwise.hip:
      * the entry point lsq_pointwise_conv, lines 306-331: Ho, Wo, P, `blocks = (P + 63) / 64`, `n_ot = O / 64`, `pair_ok`
        (stride 2 with an even Wo needs an even W: the pair's 16-byte load ends at the row's end at the latest), the choice
        between the two kernels, and `while (per_wg > 1 && blocks * (n_ot / per_wg) < min_wgs) per_wg >>= 1` with min_wgs = 256;
      * launch_all<NOT>, lines 279-289: PAIRS = stride 2, even Wo and P >= 2; VEC4 = Ho * Wo a multiple of 4."""
    ho, wo = out_size(h, stride), out_size(w, stride)
    p = n * ho * wo
    blocks = (p + 63) // 64
    n_ot = o // 64
    if generic_routes(n, c, h, w, o, stride):
        return ('generic',)
    per_wg = n_ot
    while per_wg > 1 and blocks * (n_ot // per_wg) < 256:
        per_wg >>= 1
    pairs = stride == 2 and (wo & 1) == 0 and p >= 2
    vec4 = (ho * wo) % 4 == 0
    return ('all', per_wg, pairs, vec4)


ALL_VARIANTS = frozenset(('all', n_ot, pairs, vec4) for n_ot in (1, 2, 4, 8) for pairs in (True, False) for vec4 in (True, False)) \
    | {('generic',)}

# ((N, C, H, W, O, stride), the variant the case was chosen for).  NOT = 8 needs 256 pixel tiles at O = 512 -- more than 16320
# output pixels, a 34 MB output --, NOT = 4 at O = 512 at least 128, NOT = 2 at least 64; the NOT = 1 and generic cases are tiny.
# C = 64, 128, 192, 320, 512: one, two, an odd number of and eight 64-channel chunks (the weight tile's double buffer flips
# NOT times per chunk).
PW_CASES = (
    ((5, 64, 116, 116, 512, 2), ('all', 8, True, True)),
    ((5, 64, 114, 116, 512, 2), ('all', 8, True, False)),
    ((5, 64, 120, 114, 512, 2), ('all', 8, False, True)),
    ((5, 64, 114, 117, 512, 2), ('all', 8, False, False)),
    ((5, 64, 58, 58, 512, 1), ('all', 8, False, True)),          # stride 1
    ((3, 128, 116, 116, 512, 2), ('all', 4, True, True)),
    ((3, 64, 114, 116, 512, 2), ('all', 4, True, False)),
    ((3, 64, 120, 114, 512, 2), ('all', 4, False, True)),
    ((3, 192, 114, 117, 512, 2), ('all', 4, False, False)),
    ((5, 64, 116, 116, 256, 2), ('all', 4, True, True)),         # NOT = 4 because O = 256: one workgroup row
    ((5, 64, 60, 60, 512, 2), ('all', 2, True, True)),
    ((5, 64, 58, 60, 512, 2), ('all', 2, True, False)),
    ((5, 64, 64, 58, 512, 2), ('all', 2, False, True)),
    ((5, 320, 58, 62, 512, 2), ('all', 2, False, False)),
    ((1, 512, 70, 70, 512, 1), ('all', 2, False, True)),         # eight chunks through two weight tiles each, stride 1
    ((3, 64, 8, 8, 64, 2), ('all', 1, True, True)),
    ((3, 64, 6, 12, 128, 2), ('all', 1, True, False)),
    ((2, 512, 6, 12, 128, 2), ('all', 1, True, False)),          # eight chunks of pair loads
    ((3, 64, 8, 6, 64, 2), ('all', 1, False, True)),
    ((2, 128, 10, 6, 256, 2), ('all', 1, False, False)),
    ((3, 64, 8, 7, 128, 2), ('generic',)),                       # pair_ok refuses: even Wo = 4 on an odd W = 7
    ((2, 64, 9, 9, 192, 2), ('generic',)),                       # O / 64 = 3
    ((2, 64, 9, 9, 640, 2), ('generic',)),                       # O > 512 (and 10 tiles: no power of two either)
    ((2, 64, 9, 9, 1024, 2), ('generic',)),                      # O > 512 alone
    ((1, 128, 7, 5, 192, 3), ('generic',)),                      # (the case of test_pointwise_conv_kernel)
)


def pw_id(case) -> str:
    return 'x'.join(str(v) for v in case[:5]) + f's{case[5]}'


def pw_bytes(n, c, h, w, o, stride) -> dict:
    """fp32 bytes of a case's tensors."""
    return {'x': 4 * n * c * h * w, 'w': 4 * o * c, 'y': 4 * n * o * out_size(h, stride) * out_size(w, stride)}


# ---------------------------------------------------------------------------------------------------- lsq_xnor_conv2d_proj
PROJ_WAVES = 8          # LSQ_PROJ_SHAPE: waves per workgroup


def proj_grid(n, ho, wo, o):
    """(tiles, waves, fewest tiles of a wave, most tiles of a wave) of the lsq_xnor_conv2d_proj launch that writes y [n, o, ho, wo].

    Mirrors device-side selection code, csrc/lsq_xnor_mfma.hip:
      * launch_proj<GG>, lines 689-702: `ntiles = (N * Ho * Wo + 31) >> 5`, `n_ot = O / 32`, `gx = (256 + n_ot - 1) / n_ot`,
        capped `if (gx * NWAVES > ntiles) gx = (ntiles + NWAVES - 1) / NWAVES`, NWAVES = 8 (LSQ_PROJ_SHAPE), grid (gx, n_ot);
      * xnor_mfma_kernel, lines 95 and 150-153 and the tile loop's `nxt = tile + tstride`: wave `wid` of workgroup `blockIdx.x` starts
        at tile `wid * gridDim.x + blockIdx.x` (wave-major) and steps by `tstride = gridDim.x * NWAVES` tiles."""
    ntiles = (n * ho * wo + 31) >> 5
    n_ot = o // 32
    gx = (256 + n_ot - 1) // n_ot
    if gx * PROJ_WAVES > ntiles:
        gx = (ntiles + PROJ_WAVES - 1) // PROJ_WAVES
    waves = gx * PROJ_WAVES
    counts = [len(range(first, ntiles, waves)) for first in range(waves)]       # first = wid * gx + blockIdx.x covers 0 .. waves - 1
    return ntiles, waves, min(counts), max(counts)


def fused_out_hw(case):
    """(Ho, Wo) of the 3x3, pad-1 consumer of a fused case."""
    n, c, (h, w), s, o, cp, (hx, wx) = case
    return (h + 2 - 3) // s + 1, (w + 2 - 3) // s + 1


def fused_bytes(case) -> dict:
    """Bytes of a fused case's tensors: consumer input (fp32) and its two bit planes with halo, output, projection operands."""
    n, c, (h, w), s, o, cp, (hx, wx) = case
    ho, wo = fused_out_hw(case)
    return {'x': 4 * n * c * h * w, 'planes': 2 * 8 * n * (c // 64) * (h + 2) * (w + 2), 'y': 4 * n * o * ho * wo,
            'px': 4 * n * cp * hx * wx, 'pw': 4 * o * cp, 'w': 4 * o * c * 9}


# name: (N, consumer C, consumer input H x W, consumer stride, O, projection Cp, projection input H x W) -- the layout of CASES in
# tests/test_gpu_proj_fused.py; 3 x 3 consumer, pad 1, projection stride 2
FUSED_CASES = {
    'o512_140t': (70, 256, (16, 16), 2, 512, 256, (16, 16)),       # 140 tiles on 128 waves; a wave's step of 4096 pixels = 64 whole images
    'o512_274t': (3, 256, (108, 108), 2, 512, 64, (108, 108)),     # 274 tiles: two or three per wave, partial last tile, Cp != C
    'o256_264t': (3, 128, (105, 105), 2, 256, 128, (105, 105)),    # 264 tiles on 256 waves, odd Wo = 53
    'o128_526t': (5, 64, (116, 116), 2, 128, 64, (116, 116)),      # 526 tiles on 512 waves
    'o512_c512_s1': (90, 512, (7, 7), 1, 512, 256, (14, 14)),      # stride-1 consumer (GG = 8: the largest static LDS), 138 tiles
}
FUSED_BOTH_SCHEMES = 'o256_264t'          # the case that also runs ls-T
FUSED_PARTIAL = 'o512_274t'               # partial last tile: the guard run and the repeated-run test
FUSED_ANCHORED = ('o512_274t', 'o512_c512_s1')

# every Cp the entry point admits (odd numbers of 64-channel steps in the ping-pong gather: 192, 320, 448), and the largest LDS
# request: GG = 8 fragments (74 KB static) + 32 x 516 floats of projection weights (66 KB dynamic)
CP_CASES = {f'cp{cp}': (2, 64, (12, 12), 2, 128, cp, (12, 12)) for cp in range(64, 513, 64)}
CP_CASES['c512_cp512'] = (1, 512, (8, 8), 2, 64, 512, (8, 8))
