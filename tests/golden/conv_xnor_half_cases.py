"""The cases of lsq_xnor_conv2d_half (include/lsq_hip_conv_xnor_half.h) as data: geometries, plane counts and epilogues of
tests/test_gpu_conv_xnor_half.py, with the host-side arithmetic that says which kernel a geometry takes and what its launch
looks like (csrc/lsq_xnor_mfma.hip: eligibility and launch()).  tests/test_conv_xnor_half_host.py holds the table to its limits."""

import collections

Geom = collections.namedtuple('Geom', 'id N C H W O k stride pad dil groups')


def _g(id, N, C, H, W, O, k, stride, pad, dil=1, groups=1):
    two = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    return Geom(id, N, C, H, W, O, k, two(stride), two(pad), two(dil), groups)


#: the matrix-core kernel (3x3, groups 1, 64 / 128 / 256 / 512 channels, O a multiple of 32)
MFMA = (
    _g('m64_tail', 1, 64, 5, 7, 32, 3, 1, 1),            # 35 pixels: one tile plus a 3-lane tail
    _g('m128_s2', 2, 128, 9, 9, 64, 3, 2, 1),            # stride 2
    _g('m256_o96', 1, 256, 6, 6, 96, 3, 1, 1),           # three out-channel tiles
    _g('m512_small', 1, 512, 4, 4, 64, 3, 1, 1),         # less than one tile
    _g('m64_nopad', 1, 64, 6, 6, 32, 3, 1, 0),           # no border
    _g('m64_multi', 8, 64, 28, 28, 512, 3, 1, 1),        # 196 tiles on 16 workgroups x 12 waves: four waves take a second tile
)
#: the popcount kernel (every other geometry)
POPCOUNT = (
    _g('p1x1_s2', 2, 64, 7, 7, 48, 1, 2, 0),
    _g('p24_o20', 3, 24, 6, 5, 20, 3, 1, 1),             # C not a multiple of 64, O not a multiple of 16
    _g('pgroups', 2, 32, 9, 9, 32, 3, (1, 2), (2, 1), (2, 1), 2),
    _g('p7x7', 2, 3, 12, 12, 16, 7, 2, 3),
)
GEOMS = MFMA + POPCOUNT
BY_ID = {g.id: g for g in GEOMS}
MULTI_TILE = 'm64_multi'

#: (activation planes, weight planes) every geometry runs with, under the full epilogue
PLANES = ((1, 1), (2, 1), (3, 2))
#: the geometries that also run every epilogue of EPILOGUES at EPILOGUE_PLANES
EPILOGUE_GEOMS = ('m64_tail', 'm128_s2', 'p24_o20')
EPILOGUE_PLANES = ((2, 1), (2, 2))
#: name: (bias, res_pre, act, res_post); act: None | 'relu' | 'prelu1' (one slope) | 'prelu' (one per channel)
EPILOGUES = {
    'none': (False, False, None, False),
    'bias': (True, False, None, False),
    'relu_pre': (False, True, 'relu', False),
    'prelu1_post': (False, False, 'prelu1', True),
    'both': (False, True, None, True),
}
FULL = (True, True, 'prelu', True)

#: the one large case: residual plus output exceed the 256 MiB Infinity Cache in 16-bit (non-temporal residual loads)
STREAM = _g('stream', 336, 64, 56, 56, 64, 3, 1, 1)
INFINITY_CACHE_BYTES = 256 << 20

#: limits of a quick case: elements of x and of y
MAX_ELEMENTS = 1 << 22

MFMA_WAVES = 12             # csrc/lsq_xnor_mfma.hip, launch(): one workgroup of twelve waves per CU
CUS = 256


def out_hw(g):
    ho = (g.H + 2 * g.pad[0] - g.dil[0] * (g.k - 1) - 1) // g.stride[0] + 1
    wo = (g.W + 2 * g.pad[1] - g.dil[1] * (g.k - 1) - 1) // g.stride[1] + 1
    return ho, wo


def outputs(g):
    ho, wo = out_hw(g)
    return g.N * g.O * ho * wo


def mfma_eligible(g, kx_launch=1):
    """xnor_conv_mfma_eligible of csrc/lsq_xnor_mfma.hip for one launch of ``kx_launch`` (1 or 2) activation planes."""
    ho, wo = out_hw(g)
    return (g.groups == 1 and g.k == 3 and g.dil[1] == 1 and g.O % 32 == 0 and g.N * ho * wo * g.O < 1 << 30
            and g.C in (64, 128, 256, 512) and kx_launch in (1, 2))


def launches(kx, kw):
    return kw * ((kx + 1) // 2)


def workspace_bytes(g, kx, kw):
    return 4 * outputs(g) if launches(kx, kw) > 1 else 0


def mfma_launch(g):
    """(pixel tiles, workgroups per out-channel tile, waves) of launch() in csrc/lsq_xnor_mfma.hip."""
    ho, wo = out_hw(g)
    tiles = (g.N * ho * wo + 31) // 32
    n_ot = g.O // 32
    gx = max(1, (CUS + n_ot - 1) // n_ot)
    if gx * MFMA_WAVES > tiles:
        gx = (tiles + MFMA_WAVES - 1) // MFMA_WAVES
    return tiles, gx, gx * MFMA_WAVES
