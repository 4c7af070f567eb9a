"""liblsq_hip_conv_xnor_narrow.so without a GPU: lsq_xnor_conv2d_narrow_supported over accepted and refused geometries, and the
argument errors of lsq_xnor_conv2d_narrow, which come before any launch (include/lsq_hip_conv_xnor_narrow.h)."""

import ctypes

import pytest

from quant import _hip as hip

# (N, C, H, W, O, KH, KW, stride, pad, dilation, groups), kx, kw_planes, pool -> supported
GEOMS = {
    'lenet_conv2_pooled': ((64, 20, 12, 12, 50, 5, 5, (1, 1), (0, 0), (1, 1), 1), 2, 1, 2, True),
    'c1_o1': ((1, 1, 4, 4, 1, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 1, 1, True),
    'c96_3x3_planes8': ((2, 96, 6, 6, 96, 3, 3, (1, 1), (1, 1), (1, 1), 1), 8, 8, 1, True),
    'c64_8x8_128_units': ((1, 64, 40, 40, 33, 8, 8, (3, 2), (5, 0), (2, 3), 1), 1, 1, 1, True),
    'c4096_1x1_128_units': ((2, 4096, 7, 7, 40, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 1, 2, True),
    'c65_8x8_192_units': ((1, 65, 40, 40, 33, 8, 8, (1, 1), (0, 0), (1, 1), 1), 1, 1, 1, False),
    'c96_7x7_147_units': ((2, 96, 8, 8, 96, 7, 7, (1, 1), (3, 3), (1, 1), 1), 1, 1, 1, False),
    'groups2': ((2, 96, 6, 6, 96, 3, 3, (1, 1), (1, 1), (1, 1), 2), 1, 1, 1, False),
    '9x1': ((2, 16, 16, 16, 32, 9, 1, (1, 1), (0, 0), (1, 1), 1), 1, 1, 1, False),
    'pool3': ((2, 96, 6, 6, 96, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, 1, 3, False),
    'pool2_of_one_row': ((2, 16, 3, 8, 16, 3, 3, (1, 1), (0, 0), (1, 1), 1), 1, 1, 2, False),
    'kx9': ((2, 16, 8, 8, 32, 1, 1, (1, 1), (0, 0), (1, 1), 1), 9, 1, 1, False),
    'outputs_2p30': ((1024, 16, 64, 64, 256, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 1, 1, False),
}


@pytest.mark.parametrize('gid', list(GEOMS))
def test_supported(gid):
    g, kx, kw, pool, want = GEOMS[gid]
    assert hip.xnor_conv2d_narrow_supported(hip.make_geom(*g), kx, kw, pool) is want


def test_abi_version_and_argument_errors_before_any_launch():
    lib = hip.conv_xnor_narrow_lib()
    assert lib.lsq_conv_xnor_narrow_abi_version() == hip.CONV_XNOR_NARROW_ABI_VERSION == 1
    assert lib.lsq_xnor_conv2d_narrow_supported(None, 1, 1, 1) == 0
    good = ctypes.byref(hip.make_geom(*GEOMS['c96_3x3_planes8'][0]))
    p = 4096                                          # (never dereferenced: every call below is refused on the host)
    args = [p, 1, p, p, p, 1, p, None, good, 0, None, None, None, 1, p, None]
    for i in (0, 2, 3, 4, 6, 8, 14):                  # xplanes, xscales, wbits, wsum, wscales, g, y
        assert lib.lsq_xnor_conv2d_narrow(*[None if j == i else v for j, v in enumerate(args)]) == -1, i
    for change, code in (({1: 0}, -3), ({5: 9}, -3), ({9: 4}, -3), ({9: 2}, -3),      # plane counts, unknown act, PReLU without slopes
                         ({8: ctypes.byref(hip.make_geom(*GEOMS['groups2'][0]))}, hip.E_UNSUPPORTED),
                         ({8: ctypes.byref(hip.make_geom(*GEOMS['c96_7x7_147_units'][0]))}, hip.E_UNSUPPORTED),
                         ({13: 3}, hip.E_UNSUPPORTED), ({13: 2, 11: p}, hip.E_UNSUPPORTED), ({13: 2, 12: p}, hip.E_UNSUPPORTED)):
        assert lib.lsq_xnor_conv2d_narrow(*[change.get(j, v) for j, v in enumerate(args)]) == code, (change, code)
