"""liblsq_hip_stem_gen.so without a GPU: lsq_stem_conv_gen_supported on both sides of each limit, the argument errors of
lsq_stem_conv_gen (before any launch) and those of the Python wrapper (include/lsq_hip_stem_gen.h)."""

import ctypes

import pytest
import torch

from quant import _hip as hip

# (N, C, H, W, O, KH, KW, stride, pad, dilation, groups), pool -> supported
GEOMS = {
    'cifar': ((100, 3, 32, 32, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, True),
    'lenet': ((64, 1, 28, 28, 20, 5, 5, (1, 1), (0, 0), (1, 1), 1), 2, True),
    'c4_7x7_s2_o256': ((2, 4, 64, 64, 256, 7, 7, (2, 2), (3, 3), (1, 1), 1), 2, True),
    'imagenet_shape': ((2, 3, 224, 224, 64, 7, 7, (2, 2), (3, 3), (1, 1), 1), 1, True),
    'o1_1x1': ((1, 1, 2, 2, 1, 1, 1, (1, 1), (0, 0), (1, 1), 1), 2, True),
    'pad_kernel_minus_1': ((1, 2, 5, 5, 8, 3, 5, (1, 1), (2, 4), (1, 1), 1), 1, True),
    'c5': ((2, 5, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, False),
    'o257': ((2, 3, 8, 8, 257, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, False),
    'kw8': ((2, 3, 16, 16, 64, 3, 8, (1, 1), (1, 1), (1, 1), 1), 1, False),
    'stride3': ((2, 3, 16, 16, 64, 3, 3, (3, 3), (1, 1), (1, 1), 1), 1, False),
    'stride_1_2': ((2, 3, 16, 16, 64, 3, 3, (1, 2), (1, 1), (1, 1), 1), 1, False),
    'pad_equals_kernel': ((2, 3, 16, 16, 64, 3, 3, (1, 1), (3, 1), (1, 1), 1), 1, False),
    'dilation2': ((2, 3, 16, 16, 64, 3, 3, (1, 1), (1, 1), (2, 2), 1), 1, False),
    'groups2': ((2, 2, 16, 16, 64, 3, 3, (1, 1), (1, 1), (1, 1), 2), 1, False),
    'pool3': ((2, 3, 16, 16, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1), 3, False),
    'conv_output_below_pool': ((2, 3, 3, 9, 64, 3, 3, (1, 1), (0, 0), (1, 1), 1), 2, False),
    'x_2p31': ((1 << 15, 4, 128, 128, 8, 1, 1, (2, 2), (0, 0), (1, 1), 1), 1, False),
}


@pytest.mark.parametrize('gid', list(GEOMS))
def test_supported(gid):
    g, pool, want = GEOMS[gid]
    assert hip.stem_conv_gen_supported(hip.make_geom(*g), pool) is want


def test_abi_version_and_argument_errors_before_any_launch():
    lib = hip.stem_gen_lib()
    assert lib.lsq_stem_gen_abi_version() == hip.STEM_GEN_ABI_VERSION == 1
    assert lib.lsq_stem_conv_gen_supported(None, 1) == 0
    good = ctypes.byref(hip.make_geom(*GEOMS['cifar'][0]))
    p = 4096                                          # (never dereferenced: every call below is refused on the host)
    args = [p, p, None, good, 1, None, None, 1, p, None]
    for i in (0, 1, 3, 8):                            # x, w, g, y
        assert lib.lsq_stem_conv_gen(*[None if j == i else v for j, v in enumerate(args)]) == -1, i
    bad_shape = ctypes.byref(hip.make_geom(2, 3, 0, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1))
    for i, v, code in ((5, p, -1), (6, p, -1), (4, 2, -3), (3, bad_shape, -2), (7, 0, hip.E_UNSUPPORTED),
                       (3, ctypes.byref(hip.make_geom(*GEOMS['c5'][0])), hip.E_UNSUPPORTED)):
        assert lib.lsq_stem_conv_gen(*[v if j == i else w for j, w in enumerate(args)]) == code, (i, code)


def test_wrapper_argument_errors():
    x, w, b = torch.zeros(2, 3, 8, 8), torch.zeros(16, 3, 3, 3), torch.zeros(16)
    with pytest.raises(TypeError, match='lsq_stem_conv_gen: x'):
        hip.stem_conv_gen(x.half(), w, b, 1, 1, True)
    with pytest.raises(ValueError, match='contiguous'):
        hip.stem_conv_gen(x.transpose(2, 3), w, b, 1, 1, True)
    with pytest.raises(ValueError, match='not a convolution'):
        hip.stem_conv_gen(x, torch.zeros(16, 2, 3, 3), b, 1, 1, True)
    with pytest.raises(ValueError, match='post is a pair'):
        hip.stem_conv_gen(x, w, b, 1, 1, True, post=(b, None))
    with pytest.raises(ValueError, match='bias has 3 elements'):
        hip.stem_conv_gen(x, w, torch.zeros(3), 1, 1, True)
    with pytest.raises(ValueError, match='same cuda device'):
        hip.stem_conv_gen(x, w, b, 1, 1, True)
