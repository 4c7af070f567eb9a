"""lsq_stem_conv_u8 (include/lsq_hip_stem_u8.h, csrc/stem_u8): input normalisation + conv + bias + ReLU + per-channel affine +
max-pool 1 / 2 / 3 on uint8 pixels in one kernel, NCHW and channels-last, against the fp64 composition on the CPU by the
criterion of the fp32-class stems (<= 1e-6 of max |y| and <= 2 x torch's own fp32 error + 1e-7); exact integer anchors; its
refusals; and the ``resnet.STEM_U8`` switch in QResNet's stem and in LeNet.

Measured on an MI355X (rel. error new kernel / torch fp32): see DESIGN 4.39."""

import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import detgen
from test_gpu_parity import rel_err

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENT = 12345.0

# id: (N, C, H, W), O, kernel, stride, pad, post ('neg': some negative scales), pool
CASES = {
    'imagenet_18x34': ((2, 3, 18, 34), 64, (7, 7), 2, (3, 3), None, 3),
    'imagenet_odd_19x37': ((2, 3, 19, 37), 64, (7, 7), 2, (3, 3), None, 3),
    'imagenet_two_pool3_chunks_10x70': ((2, 3, 10, 70), 64, (7, 7), 2, (3, 3), None, 3),
    'cifar_9x33': ((2, 3, 9, 33), 64, (3, 3), 1, (1, 1), None, 1),
    'lenet_12x12': ((2, 1, 12, 12), 20, (5, 5), 1, (0, 0), 'neg', 2),
    'c2_o33_3x5_s2': ((2, 2, 11, 23), 33, (3, 5), 2, (1, 2), None, 1),
}


def _hip():
    from quant import _hip
    return _hip


def _bytes(tag, shape):
    x = (detgen.uniform(tag, shape) * 256).clamp(0, 255).to(torch.uint8)
    x.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)
    return x


def _compose(x, in_scale, in_shift, w, b, stride, pad, post, pool):
    """The composition in the dtype of ``w``; x uint8."""
    xn = x.to(w.dtype) * in_scale.to(w.dtype).view(1, -1, 1, 1) + in_shift.to(w.dtype).view(1, -1, 1, 1)
    y = torch.relu(F.conv2d(xn, w, None if b is None else b.to(w.dtype), stride, pad))
    if post is not None:
        y = y * post[0].to(w.dtype).view(1, -1, 1, 1) + post[1].to(w.dtype).view(1, -1, 1, 1)
    return y if pool == 1 else F.max_pool2d(y, 2, 2) if pool == 2 else F.max_pool2d(y, 3, 2, 1)


def _run(x, in_scale, in_shift, w, b, stride, pad, post, pool, channels_last):
    dev = lambda t: None if t is None else t.to(DEV)        # noqa: E731
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last) if channels_last else x.to(DEV)
    return _hip().stem_conv_u8(xd, dev(w), dev(b), dev(in_scale), dev(in_shift), stride, pad, True,
                               None if post is None else (dev(post[0]), dev(post[1])), pool).cpu()


@pytest.mark.parametrize('cid', list(CASES))
def test_stem_conv_u8_kernel_both_layouts(cid):
    shape, o, kernel, stride, pad, post_kind, pool = CASES[cid]
    c = shape[1]
    x = _bytes(f'gpu.stemu8.x.{cid}', shape)
    w = detgen.normal(f'gpu.stemu8.w.{cid}', (o, c, *kernel), scale=(c * kernel[0] * kernel[1]) ** -0.5)
    b = detgen.normal(f'gpu.stemu8.b.{cid}', (o,), scale=0.3)
    std, mean = detgen.uniform(f'gpu.stemu8.std.{cid}', (c,), 0.2, 0.3), detgen.uniform(f'gpu.stemu8.mean.{cid}', (c,), 0.4, 0.5)
    in_scale, in_shift = 1 / (255 * std), -mean / std
    post = None
    if post_kind is not None:
        scale = detgen.uniform(f'gpu.stemu8.s.{cid}', (o,), 0.5, 1.5)
        scale[::3] *= -1
        post = (scale, detgen.normal(f'gpu.stemu8.t.{cid}', (o,), scale=0.2))
    ref = _compose(x, in_scale, in_shift, w.double(), b, stride, pad, post, pool).float()
    err32 = rel_err(_compose(x, in_scale, in_shift, w, b, stride, pad, post, pool), ref)
    y = {cl: _run(x, in_scale, in_shift, w, b, stride, pad, post, pool, cl) for cl in (False, True)}
    for cl in y:
        assert y[cl].shape == ref.shape
        err = rel_err(y[cl], ref)
        print('stem_u8', cid, 'channels_last' if cl else 'nchw', err, 'torch fp32', err32)
        assert err <= 1e-6 and err <= 2 * err32 + 1e-7, (cl, err, err32)
    assert torch.equal(y[True], y[False])


@pytest.mark.parametrize('pool', [1, 3])
@pytest.mark.parametrize('shift', [0.0, -128.0])
def test_exact_integer_anchor(pool, shift):
    # integers everywhere: every product and sum is exact below 2^24; the shift must not reach the padded pixels
    shape, o = (2, 3, 18, 34), 64
    x = _bytes(f'gpu.stemu8.anchor.x.{pool}', shape)
    w = (detgen.uniform(f'gpu.stemu8.anchor.w.{pool}', (o, 3, 7, 7)) * 9).floor().clamp(0, 8) - 4
    b = (detgen.uniform(f'gpu.stemu8.anchor.b.{pool}', (o,)) * 200).floor() - 100
    in_scale, in_shift = torch.ones(3), torch.full((3,), shift)
    ref = _compose(x, in_scale, in_shift, w.double(), b, 2, 3, None, pool).float()
    for cl in (False, True):
        assert torch.equal(_run(x, in_scale, in_shift, w, b, 2, 3, None, pool, cl), ref), cl


# what differs from an accepted call (geometry fields, pool) -> the code
REFUSALS = {'c4': ({'C': 4}, 1), 'pool4': ({}, 4), 'dilation2': ({'dil_h': 2, 'dil_w': 2}, 1)}


@pytest.mark.parametrize('rid', list(REFUSALS))
def test_refusals_write_nothing(rid):
    hip = _hip()
    fields, pool = REFUSALS[rid]
    geom = hip.make_geom(2, 3, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    for name, v in fields.items():
        setattr(geom, name, v)
    geom._key = None
    x = torch.ones((2, 4, 8, 8), dtype=torch.uint8, device=DEV)      # (large enough, should a refusal fail to refuse)
    w = torch.ones((64, 4, 3, 3), device=DEV)
    s = torch.ones((64,), device=DEV)
    y = torch.full((2, 64, 8, 8), SENT, device=DEV)
    got = hip.stem_u8_lib().lsq_stem_conv_u8(x.data_ptr(), 0, w.data_ptr(), s.data_ptr(), s.data_ptr(), s.data_ptr(), ctypes.byref(geom),
                                             1, None, None, pool, y.data_ptr(), hip.stream_ptr(y.device))
    torch.cuda.synchronize()
    assert got == hip.E_UNSUPPORTED and bool((y == SENT).all())


def test_float_input_is_refused_by_the_wrapper():
    hip = _hip()
    x, w, s = torch.ones((2, 3, 8, 8), device=DEV), torch.ones((8, 3, 3, 3), device=DEV), torch.ones((3,), device=DEV)
    with pytest.raises(TypeError, match='lsq_stem_conv_u8: x must be a torch.uint8'):
        hip.stem_conv_u8(x, w, None, s, s, 1, 1, True)


def _resnet(golden):
    from quant.models.resnet import QResNet
    model = QResNet(loss_fn=None, **golden('f6_models').json('imagenet_ls1w_ls2a_arch'))
    model.set_input_norm([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    return model, (2, 3, 32, 32)


def _lenet(golden):
    from quant.models.lenet import QLeNet5
    model = QLeNet5(F.nll_loss, x_quant='fp', w_quant='fp')
    model.set_input_norm([0.1307], [0.3081])
    return model, (2, 1, 28, 28)


def _front(model):
    """(the module that holds the input norm, the stem as a callable)."""
    return (model.blocks[0], model.blocks[0]) if hasattr(model, 'blocks') else (model, model._front)


@pytest.mark.parametrize('make', [_resnet, _lenet], ids=['resnet', 'lenet'])
def test_stem_u8_switch(make, golden):
    hip = _hip()
    from quant.models import resnet
    model, shape = make(golden)
    detgen.fill_module(model, seed=5)
    model.eval()
    x = _bytes(f'gpu.stemu8.module.{make.__name__}', shape)
    owner, _ = _front(model)
    with torch.no_grad():
        xn = (x.double() / 255 - owner.input_mean.double().view(1, -1, 1, 1)) / owner.input_std.double().view(1, -1, 1, 1)
        ref = _front(copy.deepcopy(model).double())[1](xn).float()
    model.to(DEV)
    owner, front = _front(model)
    out, tags = {}, {}
    before = resnet.STEM_U8
    try:
        for key, on, inp in (('off', False, x.to(DEV)), ('on', True, x.to(DEV)), ('fp32', True, resnet._normalise_u8(owner, x.to(DEV)))):
            resnet.STEM_U8 = on
            hip.enable_timing(True)
            with torch.no_grad():
                out[key] = front(inp).cpu()
            torch.cuda.synchronize()
            tags[key] = hip.drain_timing()
    finally:
        resnet.STEM_U8 = before
        hip.enable_timing(False)
    assert 'lsq_stem_conv_u8' not in tags['off'] and 'lsq_stem_conv_u8' not in tags['fp32']
    assert tags['on']['lsq_stem_conv_u8'][0] == 1
    err = {key: rel_err(out[key], ref) for key in out}
    print('stem_u8 switch', make.__name__, err)
    assert err['on'] <= 1e-6 and err['on'] <= 2 * err['off'] + 1e-7, err
