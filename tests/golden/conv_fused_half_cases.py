"""Epilogue variants, folded batch norms and residuals of lsq_signw_conv2d_fused_half (include/lsq_hip_conv_fused_half.h),
shared by tests/test_conv_fused_half_host.py and tests/test_gpu_conv_fused_half.py.  The geometries, weights and batches are
those of conv_half_cases.py, imported as they are.  Plain Python on the CPU; nothing here touches a GPU.

The 20 cases get the six variants cyclically (case i takes variant i mod 6), so that every variant meets a patch and a
general kernel; ``check_coverage`` is the assertion of that."""

import collections
import functools

import torch

import conv_half_cases as C
import detgen

Variant = collections.namedtuple('Variant', 'id relu prelu res_pre res_post')      # prelu: None, 'one' or 'channel'

VARIANTS = [
    Variant('none', False, None, False, False),
    Variant('relu_pre', True, None, True, False),
    Variant('prelu1_post', False, 'one', False, True),
    Variant('preluC_both', False, 'channel', True, True),
    Variant('relu_both', True, None, True, True),
    Variant('id_pre', False, None, True, False),
]
VARIANT_BY_ID = {v.id: v for v in VARIANTS}
VARIANT_OF = {c.id: VARIANTS[i % len(VARIANTS)] for i, c in enumerate(C.CASES)}


CROSS = ('p1_wide', 'long_row')        # every variant on these two: a patch and a general kernel (five general cases, six variants)


def runs():
    """(case id, variant) of every contract run: the cyclic assignment and the full cross."""
    return [(c.id, VARIANT_OF[c.id]) for c in C.CASES] + [(cid, v) for cid in CROSS for v in VARIANTS]


def check_coverage():
    """Every variant on a patch and on a general kernel; the assignment alone gives every variant a patch kernel."""
    for v in VARIANTS:
        assert any(C.BY_ID[cid].plan & C.PATCH for cid, w in runs()[:len(C.CASES)] if w is v), v.id
        kinds = {bool(C.BY_ID[cid].plan & C.PATCH) for cid, w in runs() if w is v}
        assert kinds == {True, False}, (v.id, kinds)


@functools.lru_cache(maxsize=None)
def folded_bn(cid: str):
    """(scale, shift) fp32 [C]: scales of magnitude 0.5 .. 1.5 and both signs, non-zero shifts."""
    c = C.BY_ID[cid]
    mag = detgen.uniform(f'convfused.bn.s.{cid}', (c.C,), 0.5, 1.5)
    sign = torch.where(detgen.uniform(f'convfused.bn.g.{cid}', (c.C,), -1.0, 1.0) < 0, -1.0, 1.0)
    if c.C > 1:
        sign[0], sign[1] = 1.0, -1.0              # (both signs whatever the draw)
    shift = detgen.uniform(f'convfused.bn.b.{cid}', (c.C,), 0.1, 0.6) * torch.where(
        detgen.uniform(f'convfused.bn.h.{cid}', (c.C,), -1.0, 1.0) < 0, -1.0, 1.0)
    return (mag * sign).float().contiguous(), shift.float().contiguous()


def out_shape(cid: str):
    c = C.BY_ID[cid]
    return (c.N, c.O) + C.out_hw(c)


@functools.lru_cache(maxsize=None)
def residual(cid: str, which: str, dt: str) -> torch.Tensor:
    """N(0, 1) in the type, of the output's shape; ``which``: 'pre' or 'post'."""
    return detgen.normal(f'convfused.res.{which}.{cid}', out_shape(cid), scale=1.0).to(C.DTYPES[dt])


@functools.lru_cache(maxsize=None)
def slopes(cid: str, kind: str) -> torch.Tensor:
    """PReLU weight: one slope of 0.25, or one per out-channel in -0.5 .. 0.5 with a negative one for certain."""
    c = C.BY_ID[cid]
    if kind == 'one':
        return torch.tensor([0.25])
    s = detgen.uniform(f'convfused.slope.{cid}', (c.O,), -0.5, 0.5).float()
    s[0] = -0.3
    return s.contiguous()


def folded_input(x: torch.Tensor, pre) -> torch.Tensor:
    """t of the contract, in torch: two eager fp32 operations and one rounding into x's type."""
    s, b = pre
    return (x.float() * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)).to(x.dtype)


def compose(y32: torch.Tensor, v: Variant, res_pre, res_post, slope) -> torch.Tensor:
    """The epilogue on an fp32 (or fp64) convolution result, in its type: a separate operation each."""
    out = y32
    if v.res_pre:
        out = out + res_pre.to(out.dtype)
    if v.relu:
        out = torch.where(out > 0, out, torch.zeros_like(out))
    elif v.prelu is not None:
        sl = slope.to(out.dtype)
        out = torch.where(out > 0, out, (sl.view(1, -1, 1, 1) if sl.numel() > 1 else sl) * out)
    if v.res_post:
        out = out + res_post.to(out.dtype)
    return out
