"""Inputs and CPU references of the lsq_act_quant_half tests, shared by tests/test_conv_act_half_host.py (the packer against
the layout definition) and tests/test_gpu_conv_act_half.py (the kernel): the geometries, deterministic bf16 / fp16 NCHW
batches, the clamp bounds rounded into the type, a CPU fp32 restatement of the quantizer's chain and a CPU packer into the
convolution's plane layout (include/lsq_hip.h).  The exact v1 of the free-running ls-2 / ls-T cases is
``act_solve_half_cases.oracle_rows``."""

import functools

import numpy as np
import torch

import detgen
from act_solve_half_cases import clamped32, oracle_rows, rounded  # noqa: F401  (re-exported for the tests)

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
# (C, H, W, groups, (pad_h, pad_w)); numbered from 1 in the tests' docstrings
GEOMS = (
    (1, 1, 1, 1, (0, 0)),          # 1  one element
    (3, 5, 7, 1, (1, 1)),          # 2
    (63, 7, 7, 1, (1, 1)),         # 3
    (64, 8, 8, 1, (1, 1)),         # 4  H W % 8 == 0: the wide-load path
    (65, 7, 7, 1, (0, 0)),         # 5  second word of one bit
    (130, 4, 6, 2, (1, 2)),        # 6  two groups of 65: Gg = 2, unequal padding
    (64, 3, 3, 64, (1, 1)),        # 7  depthwise: one channel a word
    (128, 14, 14, 1, (1, 1)),      # 8  H W % 4 == 0 only
    (256, 2, 4, 1, (0, 0)),        # 9
    (64, 56, 56, 1, (1, 1)),       # 10 one real ResNet row, M = 200 704, past anything kept in LDS
)
BOUNDS = (-1, 2.0, 1.3, 0.5)      # none, one both types hold, one neither holds, one that clamps about two thirds of a sample
SKIPS = (1, 3)
OUT_CHANNELS, KERNEL = 64, 3      # the rest of the convolution's geometry: every group count above divides 64


def batch_size(gi: int) -> int:
    """N of geometry gi (0-based): rotating through 1, 3, 7; the ResNet row comes twice."""
    return 2 if gi == 9 else (1, 3, 7)[gi % 3]


@functools.lru_cache(maxsize=None)
def batch(gi: int, dt: str, n: int = 0) -> torch.Tensor:
    """x [N, C, H, W] of the type on the CPU (N = batch_size(gi) unless given); nothing writes into it."""
    c, h, w = GEOMS[gi][:3]
    n = n or batch_size(gi)
    return detgen.normal(f'convacthalf.x.{gi}.{n}', (n, c, h, w), seed=gi, scale=1.2).to(DTYPES[dt])


def plane_shape(gi: int, n: int):
    """(Gt, Hp, Wp) of geometry gi."""
    c, h, w, groups, (ph, pw) = GEOMS[gi]
    return groups * ((c // groups + 63) // 64), h + 2 * ph, w + 2 * pw


def chain(xf: torch.Tensor, alpha: float, scales: torch.Tensor):
    """CPU fp32 restatement of the quantizer's chain on xf [N, ...] fp32 with scales [k, N]: (bits [k, N, ...] bool,
    |res_q| [k, N, ...] fp32)."""
    c = xf.clamp(-alpha, alpha) if alpha >= 0 else xf
    result, res = torch.zeros_like(c), c.clone()
    bits, mags = [], []
    for q in range(scales.shape[0]):
        v = scales[q].view(-1, *([1] * (c.dim() - 1)))
        b = (c - result) >= 0
        bits.append(b)
        mags.append(res.abs())
        result = result + torch.where(b, v, -v)
        res = res - torch.where(res >= 0, v, -v)
    return torch.stack(bits), torch.stack(mags)


def pack(bits, groups: int, pad) -> np.ndarray:
    """bool [k, N, C, H, W] -> uint64 words [k, N, Gt, Hp, Wp]: bit b of word (n, grp Gg + j, h + pad_h, w + pad_w) is
    channel grp cg + 64 j + b at pixel (h, w), 0 for channels past cg; halo words are 0."""
    bits = np.asarray(bits, dtype=np.uint8)
    k, n, c, h, w = bits.shape
    cg = c // groups
    gg = (cg + 63) // 64
    padded = np.zeros((k, n, groups, gg * 64, h, w), dtype=np.uint8)
    padded[:, :, :, :cg] = bits.reshape(k, n, groups, cg, h, w)
    lanes = padded.reshape(k, n, groups * gg, 64, h, w).transpose(0, 1, 2, 4, 5, 3)        # the 64 channels of a word last
    words = np.packbits(lanes, axis=-1, bitorder='little').view('<u8')[..., 0]
    out = np.zeros((k, n, groups * gg, h + 2 * pad[0], w + 2 * pad[1]), dtype=np.uint64)
    out[..., pad[0]:pad[0] + h, pad[1]:pad[1] + w] = words
    return out
