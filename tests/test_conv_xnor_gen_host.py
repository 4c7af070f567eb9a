"""liblsq_hip_conv_xnor_gen.so without a GPU: lsq_xnor_conv2d_gen_supported over accepted and refused geometries, and the
argument errors of lsq_xnor_conv2d_gen, which come before any launch (include/lsq_hip_conv_xnor_gen.h)."""

import ctypes

import pytest

from quant import _hip as hip

# (N, C, H, W, O, KH, KW, stride, pad, dilation, groups), kx, kw_planes -> supported
GEOMS = {
    'c192_1x1': ((2, 192, 9, 9, 64, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 1, True),
    'c2048_1x1_o32': ((256, 2048, 7, 7, 32, 1, 1, (1, 1), (0, 0), (1, 1), 1), 2, 1, True),
    '5x5_planes8': ((2, 64, 7, 7, 32, 5, 5, (1, 1), (2, 2), (1, 1), 1), 8, 8, True),
    '8x8_dilated_strided': ((1, 64, 40, 40, 96, 8, 8, (3, 2), (5, 0), (2, 3), 1), 1, 1, True),
    '1x7': ((2, 64, 6, 12, 64, 1, 7, (1, 2), (0, 3), (1, 1), 1), 1, 1, True),
    'tuned_3x3_c256': ((2, 256, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1), 2, 1, True),
    'groups2': ((2, 128, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 2), 1, 1, False),
    'c96': ((2, 96, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, 1, False),
    'o48': ((2, 128, 8, 8, 48, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, 1, False),
    '9x1': ((2, 64, 16, 16, 32, 9, 1, (1, 1), (0, 0), (1, 1), 1), 1, 1, False),
    'kx9': ((2, 64, 8, 8, 32, 1, 1, (1, 1), (0, 0), (1, 1), 1), 9, 1, False),
    'kw0': ((2, 64, 8, 8, 32, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 0, False),
    'empty_output': ((2, 64, 4, 4, 32, 5, 5, (1, 1), (0, 0), (2, 2), 1), 1, 1, False),
    'outputs_2p30': ((1024, 64, 64, 64, 256, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 1, False),
    'k_2p23': ((1, 1 << 17, 8, 8, 32, 8, 8, (1, 1), (0, 0), (1, 1), 1), 1, 1, False),
}


@pytest.mark.parametrize('gid', list(GEOMS))
def test_supported(gid):
    g, kx, kw, want = GEOMS[gid]
    assert hip.xnor_conv2d_gen_supported(hip.make_geom(*g), kx, kw) is want


def test_abi_version_and_argument_errors_before_any_launch():
    lib = hip.conv_xnor_gen_lib()
    assert lib.lsq_conv_xnor_gen_abi_version() == hip.CONV_XNOR_GEN_ABI_VERSION == 1
    assert lib.lsq_xnor_conv2d_gen_supported(None, 1, 1) == 0
    good = ctypes.byref(hip.make_geom(*GEOMS['c192_1x1'][0]))
    p = 4096                                          # (never dereferenced: every call below is refused on the host)
    args = [p, 1, p, p, p, 1, p, None, good, 0, None, None, None, p, None]
    for i in (0, 2, 3, 4, 6, 8, 13):                  # xplanes, xscales, wbits, wsum, wscales, g, y
        assert lib.lsq_xnor_conv2d_gen(*[None if j == i else v for j, v in enumerate(args)]) == -1, i
    for i, v, code in ((1, 0, -3), (5, 9, -3), (9, 4, -3), (9, 2, -3),        # plane counts, unknown act, PReLU without slopes
                       (8, ctypes.byref(hip.make_geom(*GEOMS['groups2'][0])), hip.E_UNSUPPORTED),
                       (8, ctypes.byref(hip.make_geom(*GEOMS['c96'][0])), hip.E_UNSUPPORTED)):
        assert lib.lsq_xnor_conv2d_gen(*[v if j == i else w for j, w in enumerate(args)]) == code, (i, code)
