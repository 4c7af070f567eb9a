"""liblsq_hip_conv_xnor_gen_half.so without a GPU: lsq_xnor_conv2d_gen_half_supported on both sides of each limit, and the
argument errors of lsq_xnor_conv2d_gen_half, which come before any launch (include/lsq_hip_conv_xnor_gen_half.h)."""

import ctypes

import pytest
import torch

from quant import _hip as hip

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
# (N, C, H, W, O, KH, KW, stride, pad, dilation, groups), kx, kw_planes, dtype -> supported
GEOMS = {
    'c192_1x1_bf16': ((2, 192, 9, 9, 64, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 1, BF16, True),
    'c192_1x1_f16': ((2, 192, 9, 9, 64, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 1, F16, True),
    'c192_1x1_f32': ((2, 192, 9, 9, 64, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 1, F32, False),
    'groups1': ((2, 128, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, 1, BF16, True),
    'groups2': ((2, 128, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 2), 1, 1, BF16, False),
    'c96': ((2, 96, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, 1, BF16, False),
    'o32': ((2, 128, 8, 8, 32, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, 1, F16, True),
    'o48': ((2, 128, 8, 8, 48, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, 1, F16, False),
    '8x8': ((1, 64, 16, 16, 32, 8, 8, (1, 1), (0, 0), (1, 1), 1), 2, 2, BF16, True),
    '9x1': ((2, 64, 16, 16, 32, 9, 1, (1, 1), (0, 0), (1, 1), 1), 1, 1, BF16, False),
    '9x9_65_taps_and_more': ((2, 64, 16, 16, 32, 9, 9, (1, 1), (0, 0), (1, 1), 1), 1, 1, BF16, False),
    'planes_8x8': ((2, 64, 8, 8, 32, 1, 1, (1, 1), (0, 0), (1, 1), 1), 8, 8, F16, True),
    'kx9': ((2, 64, 8, 8, 32, 1, 1, (1, 1), (0, 0), (1, 1), 1), 9, 1, BF16, False),
    'kx0': ((2, 64, 8, 8, 32, 1, 1, (1, 1), (0, 0), (1, 1), 1), 0, 1, BF16, False),
    'kw9': ((2, 64, 8, 8, 32, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 9, BF16, False),
    'kw0': ((2, 64, 8, 8, 32, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 0, BF16, False),
}


@pytest.mark.parametrize('gid', list(GEOMS))
def test_supported(gid):
    g, kx, kw, dtype, want = GEOMS[gid]
    geom = hip.make_geom(*g)
    assert hip.xnor_conv2d_gen_half_supported(geom, kx, kw, dtype) is want
    if dtype != F32:                                  # the 16-bit kernel takes what the fp32 one takes
        assert hip.xnor_conv2d_gen_supported(geom, kx, kw) is want


def test_abi_version_and_argument_errors_before_any_launch():
    lib = hip.conv_xnor_gen_half_lib()
    assert lib.lsq_conv_xnor_gen_half_abi_version() == hip.CONV_XNOR_GEN_HALF_ABI_VERSION == 1
    assert lib.lsq_xnor_conv2d_gen_half_supported(None, 1, 1, 1) == 0
    good = ctypes.byref(hip.make_geom(*GEOMS['c192_1x1_bf16'][0]))
    p = 4096                                          # (never dereferenced: every call below is refused on the host)
    args = [p, 1, p, p, p, 1, p, None, good, 0, None, None, None, 1, p, None]
    for i in (0, 2, 3, 4, 6, 8, 14):                  # xplanes, xscales, wbits, wsum, wscales, g, y
        assert lib.lsq_xnor_conv2d_gen_half(*[None if j == i else v for j, v in enumerate(args)]) == -1, i
    for i, v, code in ((1, 0, -3), (5, 9, -3), (9, 4, -3), (9, 2, -3),        # plane counts, unknown act, PReLU without slopes
                       (13, 0, hip.E_UNSUPPORTED), (13, 3, hip.E_UNSUPPORTED),   # the fp32 code, an unknown dtype
                       (8, ctypes.byref(hip.make_geom(*GEOMS['groups2'][0])), hip.E_UNSUPPORTED),
                       (8, ctypes.byref(hip.make_geom(*GEOMS['c96'][0])), hip.E_UNSUPPORTED)):
        assert lib.lsq_xnor_conv2d_gen_half(*[v if j == i else w for j, w in enumerate(args)]) == code, (i, code)
