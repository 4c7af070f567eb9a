"""lsq_train_wgrad (liblsq_hip_train.so): the weight gradient of a binary-activation convolution read from the sign planes,
against the fp64 closed form, the torch formulation (lsq_quant_values + conv2d_weight) and in QuantConv2d's train step."""

import ctypes

import pytest
import torch

import detgen

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BOUND = 2e-6      # |g - g64| <= BOUND * sum |gy| |x_q|, per element

# (scheme code, planes) of the real quantizers
SCHEMES = {'ls-1': (1, 1), 'ls-2': (2, 2), 'ls-T': (3, 2), 'gf-3': (4, 3), 'gf-8': (4, 8)}


def _hip():
    from quant import _hip
    return _hip


def _planes(x, geom, scheme, alpha=2.0):
    """Sign planes and scales of ``x`` from lsq_act_quant (the forward pass's quantizer)."""
    hip = _hip()
    code, k = SCHEMES[scheme]
    planes = torch.zeros((k * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    scales = torch.empty((k, geom.N), dtype=torch.float32, device=DEV)
    hip.act_quant(x.to(DEV), geom, code, k, 3, alpha, planes, scales)
    return planes, scales, k


def _xq64(planes, scales, geom):
    """x_q = sum_p v_p[n] (2 bit_p - 1) in fp64 on the CPU, from the planes' interior (the halo is not part of x)."""
    n, c, h, w = geom.N, geom.C, geom.H, geom.W
    gt, hp, wp = (c + 63) // 64, h + 2 * geom.pad_h, w + 2 * geom.pad_w
    k = scales.shape[0]
    words = planes.cpu().view(k, n, gt, hp, wp)[:, :, :, geom.pad_h:geom.pad_h + h, geom.pad_w:geom.pad_w + w]
    bits = (words.unsqueeze(3) >> torch.arange(64).view(1, 1, 1, 64, 1, 1)) & 1          # [k, n, gt, 64, h, w]
    bits = bits.reshape(k, n, gt * 64, h, w)[:, :, :c].to(torch.float64)
    return ((2 * bits - 1) * scales.cpu().to(torch.float64).view(k, n, 1, 1, 1)).sum(0)


def _closed_form(xq64, gy, geom):
    gy64 = gy.cpu().to(torch.float64)
    wshape = (geom.O, geom.C, geom.KH, geom.KW)
    st, pad = (geom.stride_h, geom.stride_w), (geom.pad_h, geom.pad_w)
    g64 = torch.nn.grad.conv2d_weight(xq64, wshape, gy64, st, pad)
    mag = torch.nn.grad.conv2d_weight(xq64.abs(), wshape, gy64.abs(), st, pad)
    return g64, mag


def _check(g, g64, mag, what):
    err = (g.cpu().to(torch.float64) - g64).abs()
    ok = err <= BOUND * mag + 1e-30
    assert bool(ok.all()), (what, float((err / (mag + 1e-30)).max()))


def _geom(n, c, h, w, o, k, s, p):
    """``k`` and ``p``: one number for both axes or (rows, columns)."""
    kh, kw = k if isinstance(k, tuple) else (k, k)
    ph, pw = p if isinstance(p, tuple) else (p, p)
    return _hip().make_geom(n, c, h, w, o, kh, kw, (s, s), (ph, pw), (1, 1), 1)


def _case_list():
    cases, i = [], 0
    cs, os_, ns = (3, 20, 64, 100, 130), (1, 50, 64, 96), (1, 3, 8)
    schemes = ('ls-1', 'ls-2', 'ls-T', 'gf-3', 'gf-8')
    for k in (1, 3, 5, 7):
        for s in (1, 2):
            for p in range(k):
                # spatial sizes: odd / even, and (every other case) the size whose output is 1 x 1
                if i % 3 == 2:
                    h = w = k - 2 * p if k - 2 * p >= 1 else k
                else:
                    h, w = (9 + (i % 2), 8 + (i % 3))
                cases.append((cs[i % 5], os_[i % 4], ns[i % 3], h, w, k, s, p, schemes[i % 5]))
                i += 1
    return cases


@pytest.mark.parametrize('c,o,n,h,w,k,s,p,scheme', _case_list())
def test_wgrad_equals_the_fp64_closed_form(c, o, n, h, w, k, s, p, scheme):
    hip = _hip()
    geom = _geom(n, c, h, w, o, k, s, p)
    ho, wo = hip.out_hw(geom)
    x = detgen.normal(f'wg.x.{c}.{o}.{k}.{s}.{p}', (n, c, h, w), scale=1.3)
    gy = detgen.normal(f'wg.gy.{c}.{o}.{k}.{s}.{p}', (n, o, ho, wo), scale=1e-3).to(DEV)
    planes, scales, kx = _planes(x, geom, scheme)
    g = hip.wgrad(planes, kx, scales, gy, geom)
    torch.cuda.synchronize()
    g64, mag = _closed_form(_xq64(planes, scales, geom), gy, geom)
    _check(g, g64, mag, (c, o, n, h, w, k, s, p, scheme))


# kernels and paddings that differ between the axes: (C, O, N, H, W, (KH, KW), stride, (pad_h, pad_w), scheme)
NON_SQUARE = [(20, 50, 3, 9, 8, (1, 3), 1, (0, 1), 'ls-2'),
              (64, 33, 1, 8, 9, (3, 1), 1, (2, 0), 'ls-T'),
              (20, 50, 2, 10, 11, (3, 5), 2, (2, 0), 'ls-2'),        # (H + 2p - k) odd on rows, even on columns
              (16, 33, 2, 8, 8, (4, 3), 1, (3, 2), 'gf-3'),          # pad = k - 1 on both axes
              (100, 96, 2, 8, 9, (2, 2), 2, (0, 1), 'ls-T'),         # even kernel, stride 2
              (72, 8, 1, 20, 12, (8, 8), 1, (7, 0), 'ls-1'),         # the largest kernel: 64 taps
              (130, 1, 3, 5, 4, (5, 2), 2, (1, 1), 'gf-8')]          # output 2 x 2, one out-channel


@pytest.mark.parametrize('c,o,n,h,w,k,s,p,scheme', NON_SQUARE)
def test_wgrad_at_non_square_kernels_and_per_axis_padding(c, o, n, h, w, k, s, p, scheme):
    """The closed form reads KH, KW, pad_h and pad_w from the geometry: a kernel that swapped the axes, or took one padding for
    both, would differ from it at every tap."""
    hip = _hip()
    geom = _geom(n, c, h, w, o, k, s, p)
    ho, wo = hip.out_hw(geom)
    assert ho >= 1 and wo >= 1
    x = detgen.normal(f'wg.ns.x.{k}.{s}.{p}', (n, c, h, w), scale=1.3)
    gy = detgen.normal(f'wg.ns.gy.{k}.{s}.{p}', (n, o, ho, wo), scale=1e-3).to(DEV)
    planes, scales, kx = _planes(x, geom, scheme)
    g = hip.wgrad(planes, kx, scales, gy, geom)
    torch.cuda.synchronize()
    assert tuple(g.shape) == (o, c) + k
    g64, mag = _closed_form(_xq64(planes, scales, geom), gy, geom)
    _check(g, g64, mag, (c, o, n, h, w, k, s, p, scheme))


@pytest.mark.parametrize('k', [3, 5])
def test_halo_taps_contribute_nothing(k):
    """grad_y non-zero only on the border outputs, pad = k - 1: the taps that land on the halo must add 0, not -v."""
    hip = _hip()
    n, c, h, w, o = 2, 64, 6, 7, 32
    geom = _geom(n, c, h, w, o, k, 1, k - 1)
    ho, wo = hip.out_hw(geom)
    gy = detgen.normal(f'wg.halo.gy{k}', (n, o, ho, wo))
    inner = torch.zeros_like(gy, dtype=torch.bool)
    inner[:, :, 1:-1, 1:-1] = True
    gy[inner] = 0
    planes, scales, kx = _planes(detgen.normal(f'wg.halo.x{k}', (n, c, h, w)), geom, 'ls-2')
    g = hip.wgrad(planes, kx, scales, gy.to(DEV), geom)
    g64, mag = _closed_form(_xq64(planes, scales, geom), gy, geom)
    _check(g, g64, mag, ('halo', k))


def test_channel_tail_writes_nothing_outside_the_output():
    hip = _hip()
    n, c, h, w, o, k = 3, 100, 9, 8, 50, 3
    geom = _geom(n, c, h, w, o, k, 1, 1)
    ho, wo = hip.out_hw(geom)
    planes, scales, kx = _planes(detgen.normal('wg.tail.x', (n, c, h, w)), geom, 'ls-2')
    gy = detgen.normal('wg.tail.gy', (n, o, ho, wo)).to(DEV)
    size = o * c * k * k
    buf = torch.full((size + 4096,), 12345.0, dtype=torch.float32, device=DEV)
    tl = hip.train_lib()
    need = tl.lsq_train_wgrad_workspace_bytes(ctypes.byref(geom), kx)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=DEV)
    code = tl.lsq_train_wgrad(planes.data_ptr(), kx, scales.data_ptr(), gy.data_ptr(), ctypes.byref(geom), buf.data_ptr(),
                              ws.data_ptr(), ws.numel(), hip.stream_ptr(DEV))
    assert code == 0
    torch.cuda.synchronize()
    assert bool((buf[size:] == 12345.0).all())
    g64, mag = _closed_form(_xq64(planes, scales, geom), gy, geom)
    _check(buf[:size].view(o, c, k, k), g64, mag, 'tail')


def test_results_are_bitwise_deterministic_across_calls_and_streams():
    hip = _hip()
    n, c, h, w, o = 16, 64, 28, 28, 64
    geom = _geom(n, c, h, w, o, 3, 1, 1)
    planes, scales, kx = _planes(detgen.normal('wg.det.x', (n, c, h, w)), geom, 'ls-2')
    gy = detgen.normal('wg.det.gy', (n, o, h, w), scale=1e-2).to(DEV)
    g1 = hip.wgrad(planes, kx, scales, gy, geom)
    g2 = hip.wgrad(planes, kx, scales, gy, geom)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        g3 = hip.wgrad(planes, kx, scales, gy, geom)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert hip.train_lib().lsq_train_wgrad_workspace_bytes(ctypes.byref(geom), kx) > 0       # the K split is exercised
    assert torch.equal(g1, g2) and torch.equal(g1, g3)


# the 16 binary 3x3 convolutions of ResNet-18 (ImageNet): (C, O, H, stride)
RESNET18_LAYERS = ([(64, 64, 56, 1)] * 4 + [(64, 128, 56, 2)] + [(128, 128, 28, 1)] * 3 + [(128, 256, 28, 2)]
                   + [(256, 256, 14, 1)] * 3 + [(256, 512, 14, 2)] + [(512, 512, 7, 1)] * 3)
SHAPES = sorted(set(RESNET18_LAYERS), key=RESNET18_LAYERS.index)      # 7 distinct shapes among the 16 layers


@pytest.mark.parametrize('c,o,h,s', SHAPES)
def test_resnet18_shapes_batch16_against_fp64(c, o, h, s):
    hip = _hip()
    geom = _geom(16, c, h, h, o, 3, s, 1)
    ho, wo = hip.out_hw(geom)
    planes, scales, kx = _planes(detgen.normal(f'wg.r18.x{c}{o}{h}', (16, c, h, h)), geom, 'ls-2')
    gy = detgen.normal(f'wg.r18.gy{c}{o}{h}', (16, o, ho, wo), scale=1e-4).to(DEV)
    g = hip.wgrad(planes, kx, scales, gy, geom)
    g64, mag = _closed_form(_xq64(planes, scales, geom), gy, geom)
    _check(g, g64, mag, ('r18', c, o, h, s))


@pytest.mark.parametrize('c,o,h,s', SHAPES)
def test_resnet18_shapes_batch256_against_the_torch_formulation(c, o, h, s):
    hip = _hip()
    geom = _geom(256, c, h, h, o, 3, s, 1)
    ho, wo = hip.out_hw(geom)
    x = (torch.randn((256, c, h, h), generator=torch.Generator(device=DEV).manual_seed(c + o + h), device=DEV) * 1.2)
    planes, scales, kx = _planes(x, geom, 'ls-2')
    gy = torch.randn((256, o, ho, wo), generator=torch.Generator(device=DEV).manual_seed(7 * c + o), device=DEV) * 1e-4
    g = hip.wgrad(planes, kx, scales, gy, geom)
    xq = hip.quant_values(x, scales, 2.0)
    ref = torch.nn.grad.conv2d_weight(xq, (o, c, 3, 3), gy, (s, s), (1, 1))
    err = float((g - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, err


# ---- QuantConv2d's train step
BINARY_TRAIN_CASES = [('ls-2', 'ls-1', 1, True), ('ls-1', 'ls-1', 2, True), ('gf-2', 'ls-1', 1, False), ('ls-T', 'ls-1', 2, True),
                      ('ls-1', 'gf-2', 1, True), ('ls-1', 'ls-2', 2, False), ('ls-2', 'ls-T', 1, True),
                      ('gf-4', 'gf-3', 1, True), ('gf-4', 'gf-3', 2, False)]


@pytest.fixture
def wgrad_on(monkeypatch):
    from quant.binary import hip_train
    monkeypatch.setattr(hip_train, 'WGRAD_KERNEL', True)


def _module(xs, ws, stride, bias, hip_path):
    from quant.binary.binary_conv import QuantConv2d
    conv = QuantConv2d(xs, ws, 32, 48, 3, {'kind': 'symmetric', 'alpha': 2}, stride=stride, padding=1, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(detgen.normal('wg.train.w', conv.weight.shape, scale=0.3))
        if bias:
            conv.bias.copy_(detgen.normal('wg.train.b', conv.bias.shape, scale=0.1))
    conv.hip_train = hip_path
    return conv.to(DEV).train()


class _Spy:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self.fn(*a, **k)


def _spies(monkeypatch):
    hip = _hip()
    tl = hip.train_lib()
    kernel = _Spy(tl.lsq_train_wgrad)
    monkeypatch.setattr(tl, 'lsq_train_wgrad', kernel)
    miopen = _Spy(torch.nn.grad.conv2d_weight)
    monkeypatch.setattr(torch.nn.grad, 'conv2d_weight', miopen)
    return kernel, miopen


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('xs,ws,stride,bias', BINARY_TRAIN_CASES)
def test_train_step_takes_the_wgrad_kernel(monkeypatch, wgrad_on, xs, ws, stride, bias):
    from quant.binary import hip_train
    assert hip_train.WGRAD_KERNEL
    ref = _module(xs, ws, stride, bias, False)
    conv = _module(xs, ws, stride, bias, True)
    x = detgen.normal('wg.train.x', (4, 32, 13, 10), scale=1.2).to(DEV)
    gy_shape = (4, 48, (13 - 1) // stride + 1, (10 - 1) // stride + 1)
    gy = detgen.normal('wg.train.gy', gy_shape).to(DEV)
    ref(x).backward(gy)
    kernel, miopen = _spies(monkeypatch)
    conv(x).backward(gy)
    assert kernel.calls == 1 and miopen.calls == 0
    assert _rel(conv.weight.grad, ref.weight.grad) <= 1e-5


def test_fp_activations_keep_conv2d_weight(monkeypatch, wgrad_on):
    ref = _module('fp', 'ls-1', 1, True, False)
    conv = _module('fp', 'ls-1', 1, True, True)
    x = detgen.normal('wg.train.x', (4, 32, 13, 10), scale=1.2).to(DEV)
    gy = detgen.normal('wg.train.gy', (4, 48, 13, 10)).to(DEV)
    ref(x).backward(gy)
    kernel, miopen = _spies(monkeypatch)
    conv(x).backward(gy)
    assert kernel.calls == 0 and miopen.calls == 1
    assert _rel(conv.weight.grad, ref.weight.grad) <= 1e-5


def test_switch_restores_the_torch_weight_gradient(monkeypatch):
    from quant.binary import hip_train
    monkeypatch.setattr(hip_train, 'WGRAD_KERNEL', False)       # (the default; set here so the test holds either way)
    conv = _module('ls-2', 'ls-1', 1, True, True)
    x = detgen.normal('wg.train.x', (4, 32, 13, 10), scale=1.2).to(DEV)
    kernel, miopen = _spies(monkeypatch)
    conv(x).backward(detgen.normal('wg.train.gy', (4, 48, 13, 10)).to(DEV))
    assert kernel.calls == 0 and miopen.calls == 1


@pytest.mark.parametrize('xs', ['ls-2', 'ls-1'])
def test_backward_reads_the_planes_of_its_own_step(monkeypatch, wgrad_on, xs):
    """Two forwards of one module on different inputs, one backward of the combined loss: each step's weight gradient
    must come from its own planes (the module's shared plane workspace holds the second input's by then)."""
    ref = _module(xs, 'ls-1', 1, True, False)
    conv = _module(xs, 'ls-1', 1, True, True)
    x1 = detgen.normal('wg.two.x1', (4, 32, 13, 10), scale=1.2).to(DEV)
    x2 = detgen.normal('wg.two.x2', (4, 32, 13, 10), scale=0.7).to(DEV)
    g1 = detgen.normal('wg.two.g1', (4, 48, 13, 10)).to(DEV)
    g2 = detgen.normal('wg.two.g2', (4, 48, 13, 10)).to(DEV)
    ((ref(x1) * g1).sum() + (ref(x2) * g2).sum()).backward()
    kernel, _ = _spies(monkeypatch)
    ((conv(x1) * g1).sum() + (conv(x2) * g2).sum()).backward()
    assert kernel.calls == 2
    assert _rel(conv.weight.grad, ref.weight.grad) <= 1e-5
