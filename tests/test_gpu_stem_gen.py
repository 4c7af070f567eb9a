"""lsq_stem_conv_gen (include/lsq_hip_stem_gen.h, csrc/stem_gen): conv + bias + ReLU + per-channel affine + 2x2 max-pool in
one kernel against the fp64 composition on the CPU, by the criterion of test_stem_conv_pool_kernel for the three-term split;
its refusals; and the ``resnet.STEM_GENERAL`` switch in the CIFAR stem and in LeNet."""

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

# id: (N, C, H, W), O, kernel, stride, pad, bias, relu, post (None / 'pos' / 'neg': some negative scales), pool
CASES = {
    'cifar_stem': ((3, 3, 32, 32), 64, (3, 3), 1, (1, 1), True, True, None, 1),
    'lenet_front': ((2, 1, 28, 28), 20, (5, 5), 1, (0, 0), True, True, 'pos', 2),
    'odd_floor_pool': ((1, 3, 9, 13), 64, (3, 3), 1, (1, 1), True, True, 'neg', 2),
    '7x7_stride2': ((2, 3, 17, 22), 32, (7, 7), 2, (3, 3), True, True, None, 1),
    '3x5_strips_chunks_o96': ((1, 2, 40, 70), 96, (3, 5), 1, (1, 2), False, False, None, 1),
    '1x1_c4_o8': ((2, 4, 6, 6), 8, (1, 1), 1, (0, 0), True, False, None, 2),
}


def _hip():
    from quant import _hip
    return _hip


def _compose(x, w, b, stride, pad, relu, post, pool):
    y = F.conv2d(x, w, b, stride, pad)
    y = torch.relu(y) if relu else y
    if post is not None:
        y = y * post[0].view(1, -1, 1, 1) + post[1].view(1, -1, 1, 1)
    return F.max_pool2d(y, 2, 2) if pool == 2 else y


@pytest.mark.parametrize('cid', list(CASES))
def test_stem_conv_gen_kernel(cid):
    hip = _hip()
    shape, o, kernel, stride, pad, has_bias, relu, post_kind, pool = CASES[cid]
    x = detgen.normal(f'gpu.stemgen.x.{cid}', shape, scale=1.3)
    w = detgen.normal(f'gpu.stemgen.w.{cid}', (o, shape[1], *kernel), scale=(shape[1] * kernel[0] * kernel[1]) ** -0.5)
    b = detgen.normal(f'gpu.stemgen.b.{cid}', (o,), scale=0.3) if has_bias else None
    post = None
    if post_kind is not None:
        scale = detgen.uniform(f'gpu.stemgen.s.{cid}', (o,), 0.5, 1.5)
        if post_kind == 'neg':
            scale[::3] *= -1
        post = (scale, detgen.normal(f'gpu.stemgen.t.{cid}', (o,), scale=0.2))
    dbl = lambda t: None if t is None else t.double()       # noqa: E731
    ref = _compose(x.double(), w.double(), dbl(b), stride, pad, relu, None if post is None else (post[0].double(), post[1].double()),
                   pool).float()
    f32 = _compose(x, w, b, stride, pad, relu, post, pool)
    dev = lambda t: None if t is None else t.to(DEV)        # noqa: E731
    y = hip.stem_conv_gen(x.to(DEV), w.to(DEV), dev(b), stride, pad, relu, None if post is None else (dev(post[0]), dev(post[1])),
                          pool).cpu()
    assert y.shape == ref.shape
    err, err32 = rel_err(y, ref), rel_err(f32, ref)
    print('stem_gen', cid, err, 'torch fp32', err32)
    assert err <= 1e-6 and err <= 2 * err32 + 1e-7, (err, err32)
    if post is None:                                         # an image of zeros gives relu(bias) (the bias, 0) everywhere, exactly
        y0 = hip.stem_conv_gen(torch.zeros(shape, device=DEV), w.to(DEV), dev(b), stride, pad, relu, None, pool).cpu()
        want = torch.zeros(o) if b is None else (torch.relu(b) if relu else b)
        assert torch.equal(y0, want.view(1, -1, 1, 1).expand_as(y0))


# what differs from an accepted call (geometry fields, pool, post_shift given) -> the code
REFUSALS = {
    'c5': ({'C': 5}, 1, True, -6),
    'kh8': ({'KH': 8, 'H': 12}, 1, True, -6),
    'dilation2': ({'dil_h': 2, 'dil_w': 2}, 1, True, -6),
    'groups2': ({'C': 2, 'groups': 2}, 1, True, -6),
    'pool3': ({}, 3, True, -6),
    'stride_1_2': ({'stride_w': 2}, 1, True, -6),
    'scale_without_shift': ({}, 1, False, -1),
}


@pytest.mark.parametrize('rid', list(REFUSALS))
def test_stem_conv_gen_refusals_write_nothing(rid):
    hip = _hip()
    fields, pool, with_shift, code = REFUSALS[rid]
    geom = hip.make_geom(2, 3, 8, 8, 64, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    for name, v in fields.items():
        setattr(geom, name, v)
    geom._key = None
    x = torch.ones((2, 5, 12, 8), device=DEV)                # (large enough for every case, should a refusal fail to refuse)
    w = torch.ones((64, 5, 8, 3), device=DEV)
    s = torch.ones((64,), device=DEV)
    y = torch.full((2, 64, 12, 8), SENT, device=DEV)
    got = hip.stem_gen_lib().lsq_stem_conv_gen(x.data_ptr(), w.data_ptr(), s.data_ptr(), ctypes.byref(geom), 1, s.data_ptr(),
                                               s.data_ptr() if with_shift else None, pool, y.data_ptr(), hip.stream_ptr(y.device))
    torch.cuda.synchronize()
    assert got == code and bool((y == SENT).all())


def _cifar_stem():
    from quant.models import resnet
    stem = resnet._Stem(torch.nn.Conv2d(3, 64, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(64), torch.nn.ReLU(inplace=True),
                        torch.nn.Identity())
    return stem, stem[0], (2, 3, 32, 32)


def _lenet():
    from quant.models.lenet import QLeNet5
    model = QLeNet5(F.nll_loss, x_quant='fp', w_quant='fp')
    return model, model.conv1, (2, 1, 28, 28)


@pytest.mark.parametrize('make', [_cifar_stem, _lenet], ids=['cifar_stem', 'lenet'])
def test_stem_general_switch(make, monkeypatch):
    hip = _hip()
    from quant.models import resnet
    model, conv, shape = make()
    detgen.fill_module(model, seed=5)
    model.eval()
    x = detgen.normal(f'gpu.stemgen.module.{make.__name__}', shape, scale=1.2)
    with torch.no_grad():
        ref = copy.deepcopy(model).double()(x.double()).float()
    model.to(DEV)
    seen = []                                                # weight shapes of the torch convolutions of a forward
    conv2d = F.conv2d
    monkeypatch.setattr(F, 'conv2d', lambda inp, weight, *a, **k: (seen.append(tuple(weight.shape)), conv2d(inp, weight, *a, **k))[1])
    out, tags, convs = {}, {}, {}
    before = resnet.STEM_GENERAL
    try:
        for on in (False, True):
            resnet.STEM_GENERAL = on
            del seen[:]
            hip.enable_timing(True)
            with torch.no_grad():
                out[on] = model(x.to(DEV)).cpu()
            torch.cuda.synchronize()
            tags[on] = hip.drain_timing()
            convs[on] = seen.count(tuple(conv.weight.shape))
    finally:
        resnet.STEM_GENERAL = before
        hip.enable_timing(False)
    assert 'lsq_stem_conv_gen' not in tags[False] and convs[False] == 1
    assert tags[True]['lsq_stem_conv_gen'][0] == 1 and convs[True] == 0
    err = {on: float((out[on] - ref).abs().max()) for on in out}
    print('stem_general', make.__name__, err)
    assert err[True] <= 2 * err[False] + 1e-6 * float(ref.abs().max()), err
