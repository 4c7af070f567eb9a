"""lsq_pointwise_conv (csrc/lsq_pointwise.hip) at every kernel it can launch: the sixteen pointwise_all_kernel<NOT, PAIRS, VEC4>
instantiations and the one-tile-per-workgroup pointwise_conv_kernel by each of its three routes.  The shapes and the variant each
one reaches are tests/golden/projection_cases.py's PW_CASES, proved on the host by tests/test_projection_cases_host.py.

Per case: integer-grid operands, on which the fp64 result cast to fp32 is exact in any summation order (torch.equal, with and
without bias); the same call through the raw C ABI into a view in the middle of a NaN-filled buffer (nothing outside the view is
written, nothing inside is left: the partial last tile, the 16-byte group stores, a pixel pair at an image boundary); and one
Gaussian-input pass held to max(1e-6, 2 e32 + 1e-7) of max|y|, e32 being the error of torch's own fp32 conv2d against fp64."""

import pytest
import torch

import detgen
import projection_cases as PC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MARGIN = 256            # floats on either side of the guarded output


def _hip():
    from quant import _hip
    return _hip


def rel_err(y, ref):
    return float((y - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def conv64(x, w, b, stride):
    """fp64 [N, O, Ho, Wo] on the device: the strided slice, one matmul per image."""
    xs = x[:, :, ::stride, ::stride].double()
    n, c, ho, wo = xs.shape
    y = torch.matmul(w.double(), xs.reshape(n, c, ho * wo)).reshape(n, w.shape[0], ho, wo)
    return y if b is None else y + b.double().view(1, -1, 1, 1)


@pytest.mark.parametrize('case', [c for c, _ in PC.PW_CASES], ids=[PC.pw_id(c) for c, _ in PC.PW_CASES])
def test_pointwise_variant_exact_on_the_integer_grid(case):
    hip = _hip()
    n, c, h, w, o, stride = case
    tag = f'gpu.pwv.{PC.pw_id(case)}'
    x = PC.grid_operands(tag + '.x', (n, c, h, w), *PC.X_RANGE).to(DEV)
    wt = PC.grid_operands(tag + '.w', (o, c), *PC.W_RANGE).to(DEV)
    b = PC.grid_operands(tag + '.b', (o,), *PC.B_RANGE).to(DEV)
    ref64 = conv64(x, wt, b, stride)
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64) and float(ref.abs().max()) < 2 ** 15          # the reference is exact as fp32
    y = hip.pointwise_conv(x, wt, b, stride)
    assert y.shape == ref.shape
    assert torch.equal(y, ref), (PC.pointwise_variant(*case), float((y - ref).abs().max()))
    y0 = hip.pointwise_conv(x, wt, None, stride)
    assert torch.equal(y0, conv64(x, wt, None, stride).float()), PC.pointwise_variant(*case)

    # the raw C ABI into a 16-byte-aligned view inside a NaN-filled buffer
    buf = torch.full((ref.numel() + 2 * MARGIN,), float('nan'), device=DEV)
    inside = buf[MARGIN:MARGIN + ref.numel()]
    assert inside.data_ptr() % 16 == 0
    code = hip.lib().lsq_pointwise_conv(x.data_ptr(), n, c, h, w, wt.data_ptr(), b.data_ptr(), o, stride, inside.data_ptr(),
                                        hip.stream_ptr(x.device))
    assert code == 0
    assert torch.isnan(buf[:MARGIN]).all() and torch.isnan(buf[MARGIN + ref.numel():]).all(), 'written outside y'
    assert not torch.isnan(inside).any(), 'outputs left unwritten'
    assert torch.equal(inside.view(ref.shape), ref)


@pytest.mark.parametrize('case', [c for c, _ in PC.PW_CASES], ids=[PC.pw_id(c) for c, _ in PC.PW_CASES])
def test_pointwise_variant_gaussian_inputs(case):
    """The fp32 chain of C fmas against fp64, beside torch's own fp32 convolution of the same input (on the CPU): 1e-6 is the
    bound of test_pointwise_conv_kernel (C <= 256); the second term, the stem test's idiom, covers C = 320 and 512.
    Measured on the MI355X: at most 7.2e-7 for C <= 256; 7.8e-7 at C = 320 (torch 8.7e-7); 9.6e-7 at C = 512 (torch 1.0e-6)."""
    hip = _hip()
    n, c, h, w, o, stride = case
    x = detgen.normal(f'gpu.pwv.x{(n, c, h, w)}', (n, c, h, w), scale=1.1)
    wt = detgen.normal(f'gpu.pwv.w{(o, c)}', (o, c), scale=c ** -0.5)
    b = detgen.normal(f'gpu.pwv.b{o}', (o,), scale=0.2)
    f32 = torch.nn.functional.conv2d(x, wt.view(o, c, 1, 1), b, stride).to(DEV)
    x, wt, b = x.to(DEV), wt.to(DEV), b.to(DEV)
    ref = conv64(x, wt, b, stride).float()
    y = hip.pointwise_conv(x, wt, b, stride)
    err, e32 = rel_err(y, ref), rel_err(f32, ref)
    print('pointwise', PC.pointwise_variant(*case), case, err, 'torch fp32', e32)
    assert y.shape == ref.shape and err <= max(1e-6, 2 * e32 + 1e-7), (err, e32)
