"""liblsq_hip_stem_u8.so without a GPU: lsq_stem_conv_u8_supported on both sides of each limit, the argument errors of
lsq_stem_conv_u8 (before any launch), and what a uint8 input means to QResNet and QLeNet5 on the CPU
(include/lsq_hip_stem_u8.h)."""

import ctypes

import pytest
import torch

from quant import _hip as hip

# (N, C, H, W, O, KH, KW, stride, pad, dilation, groups), pool, layout -> supported
GEOMS = {
    'imagenet': ((256, 3, 224, 224, 64, 7, 7, (2, 2), (3, 3), (1, 1), 1), 3, 0, True),
    'imagenet_channels_last': ((64, 3, 224, 224, 64, 7, 7, (2, 2), (3, 3), (1, 1), 1), 3, 1, True),
    'cifar': ((100, 3, 32, 32, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, 1, True),
    'lenet': ((64, 1, 28, 28, 20, 5, 5, (1, 1), (0, 0), (1, 1), 1), 2, 0, True),
    'o256_pool3_3x3_output': ((1, 2, 3, 3, 256, 1, 1, (1, 1), (0, 0), (1, 1), 1), 3, 0, True),
    'pad_kernel_minus_1': ((1, 2, 5, 5, 8, 3, 5, (1, 1), (2, 4), (1, 1), 1), 1, 1, True),
    'c4': ((2, 4, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, 0, False),
    'o257': ((2, 3, 8, 8, 257, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, 0, False),
    'kh8': ((2, 3, 16, 16, 64, 8, 3, (1, 1), (1, 1), (1, 1), 1), 1, 0, False),
    'stride3': ((2, 3, 16, 16, 64, 3, 3, (3, 3), (1, 1), (1, 1), 1), 1, 0, False),
    'stride_2_1': ((2, 3, 16, 16, 64, 3, 3, (2, 1), (1, 1), (1, 1), 1), 1, 0, False),
    'pad_equals_kernel': ((2, 3, 16, 16, 64, 3, 3, (1, 1), (1, 3), (1, 1), 1), 1, 0, False),
    'dilation2': ((2, 3, 16, 16, 64, 3, 3, (1, 1), (1, 1), (2, 2), 1), 1, 0, False),
    'pool4': ((2, 3, 16, 16, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1), 4, 0, False),
    'layout2': ((2, 3, 16, 16, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1), 1, 2, False),
    'conv_output_below_pool3': ((2, 3, 4, 9, 64, 3, 3, (1, 1), (0, 0), (1, 1), 1), 3, 0, False),
    'y_2p31': ((1 << 14, 1, 64, 64, 64, 1, 1, (1, 1), (0, 0), (1, 1), 1), 1, 0, False),
}


@pytest.mark.parametrize('gid', list(GEOMS))
def test_supported(gid):
    g, pool, layout, want = GEOMS[gid]
    assert hip.stem_conv_u8_supported(hip.make_geom(*g), pool, layout) is want


def test_abi_version_and_argument_errors_before_any_launch():
    lib = hip.stem_u8_lib()
    assert lib.lsq_stem_u8_abi_version() == hip.STEM_U8_ABI_VERSION == 1
    assert lib.lsq_stem_conv_u8_supported(None, 1, 0) == 0
    good = ctypes.byref(hip.make_geom(*GEOMS['cifar'][0]))
    p = 4096                                          # (never dereferenced: every call below is refused on the host)
    args = [p, 0, p, None, p, p, good, 1, None, None, 1, p, None]
    for i in (0, 2, 4, 5, 6, 11):                     # x, w, in_scale, in_shift, g, y
        assert lib.lsq_stem_conv_u8(*[None if j == i else v for j, v in enumerate(args)]) == -1, i
    bad_shape = ctypes.byref(hip.make_geom(2, 3, 0, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1))
    for i, v, code in ((8, p, -1), (9, p, -1), (7, 2, -3), (6, bad_shape, -2), (10, 0, hip.E_UNSUPPORTED), (1, 2, hip.E_UNSUPPORTED),
                       (6, ctypes.byref(hip.make_geom(*GEOMS['c4'][0])), hip.E_UNSUPPORTED)):
        assert lib.lsq_stem_conv_u8(*[v if j == i else w for j, w in enumerate(args)]) == code, (i, code)


def _resnet(golden):
    from quant.models.resnet import QResNet
    return QResNet(loss_fn=None, **golden('f6_models').json('imagenet_ls1w_ls2a_arch')), (2, 3, 32, 32), ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])


def _lenet(golden):
    from quant.models.lenet import QLeNet5
    return QLeNet5(torch.nn.functional.nll_loss, x_quant='fp', w_quant='fp'), (2, 1, 28, 28), ([0.1307], [0.3081])


@pytest.mark.parametrize('make', [_resnet, _lenet], ids=['resnet', 'lenet'])
def test_uint8_input_on_the_cpu(make, golden):
    torch.manual_seed(3)
    model, shape, (mean, std) = make(golden)
    model.train()
    x = torch.randint(0, 256, shape, dtype=torch.uint8)
    with pytest.raises(ValueError, match='set_input_norm'):
        model(x)
    keys = list(model.state_dict())
    model.set_input_norm(mean, std)
    assert list(model.state_dict()) == keys
    with torch.no_grad():
        model(x.float())                                # (a train-mode forward caches the weight scales)
        model.eval()
        xn = x.float().div(255).sub(torch.tensor(mean).view(1, -1, 1, 1)).div(torch.tensor(std).view(1, -1, 1, 1))
        want = model(xn)
        assert torch.equal(model(x), want)
        assert torch.equal(model(x.contiguous(memory_format=torch.channels_last)), want)
    with pytest.raises(ValueError, match='elements each'):
        model.set_input_norm(mean + [0.5], std)
