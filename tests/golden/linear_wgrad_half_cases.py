"""Cases, inputs and the fp64 references of lsq_linear_signx_wgrad_half (liblsq_hip_linear_wgrad_half.so), shared by
tests/test_linear_wgrad_half_host.py and tests/test_gpu_linear_wgrad_half.py.  Plain Python on the CPU; nothing here touches
a GPU.

A case is (N, T, F, O, xs, ws): gy [M, O] and x [M, F] of a 16-bit type, M = N T rows, the activation scheme ``xs`` and -- for
contract (B) -- the weight scheme ``ws``, which rotates over ls-1, ls-2, ls-T and gf-3.  The table holds the smallest shapes
that reach each piece of the kernels; ``kernel`` names the class the tile rule of lsq_linear_signx_wgrad puts the case in
(``QuantLinear._tile_class`` on (O, F)).

``inputs(cid, dtype)``: x and gy from detgen rounded into the type, then the special values of x placed AGAIN (rounding moves
them): +-0, +-alpha, +-1, values beyond alpha and, with two or more activation planes, in sample 0 the two representable
neighbours of the second sign's edge (linear_train_half_cases._place_edges).  The activation scales are those of the torch
formulation's quantizer on x.float(); the weight scales are oracle.ref_port.weight_scales'.

References, both with every sign decision taken from the fp32 chain and the values in fp64:
  ref_a   gy64^T . x_q64                                     (linear_wgrad_cases.reference64)
  ref_b   the weight chain's estimator applied to ref_a      (train_step_cases.chain64 on the fp32 weight, no clamp)
``emulated64`` is the prescribed arithmetic of the kernel -- the 16-bit gy widened exactly, a = fl32(gy xs), hi + lo in bf16 --
summed exactly; tests/test_linear_wgrad_half_host.py holds it to half the bound at every case, which is what fixes SEED_BASE.
"""

import collections
import functools

import torch

import detgen
import linear_train_half_cases as L
import linear_wgrad_cases as C
import train_step_cases as T
from linear_train_half_cases import DTYPE_NAMES, DTYPES, shifted  # noqa: F401
from oracle import ref_port as P

BOUND = C.BOUND       # |out - ref| <= BOUND * max |ref|: the project's figure for the bf16 hi + lo split
ALPHA = 3.0           # symmetric clamp in front of the activation quantizer (exact in both types)
CLAMP = {'kind': 'symmetric', 'alpha': 3}
# The first of 0, 1000, 2000, ... at which the prescribed arithmetic, summed exactly, is within half the bound at every case
# in both types (tests/test_linear_wgrad_half_host.py asserts it; chosen on the CPU, never from the kernel).
SEED_BASE = 0

Case = collections.namedtuple('Case', 'id N T F O xs ws kernel clamp')
_WS = ('ls-1', 'ls-2', 'ls-T', 'gf-3')
_TABLE = [
    # ---- wgrad_split: fewer than 256 tiles of 64 x 64 in O x F
    ('one_product', 1, 1, 1, 1, 'ls-1', 'split'),
    ('ragged', 7, 1, 33, 65, 'ls-T', 'split'),                   # M < 64, ragged F and O
    ('odd_rows', 3, 1, 35, 63, 'ls-2', 'split'),                 # odd F and O: rows start on 2-byte, not 4-byte addresses
    ('lenet_fc1', 64, 1, 800, 500, 'gf-3', 'split'),             # one word, one unit per wave
    ('rows_per_sample', 3, 5, 64, 130, 'ls-2', 'split'),         # sample boundaries inside a 16-row step
    ('long_m', 4100, 1, 65, 130, 'ls-1', 'split'),               # 260 units over 8 ranges, M % 64 = 4
    ('eight_planes', 16, 1, 128, 40, 'gf-8', 'split'),
    # ---- 64 x 64 tiles: at least 256 of them, fewer than 256 of 128 x 128
    ('tiles64_ragged', 300, 1, 1000, 1033, 'gf-3', 'small'),     # element loads, ragged everywhere
    ('tiles64_vec', 65, 1, 1000, 1032, 'gf-2', 'small'),         # vector loads, one row past a word
    ('tiles64_t4', 33, 4, 1024, 1024, 'ls-2', 'small'),          # T = 4
    # ---- 128 x 128 tiles
    ('tiles128', 130, 1, 2048, 2048, 'ls-1', 'big'),
    ('tiles128_ragged', 130, 1, 2041, 2047, 'ls-T', 'big'),
]
CASES = [Case(t[0], *t[1:6], _WS[i % 4], t[6], CLAMP) for i, t in enumerate(_TABLE)]
BY_ID = {c.id: c for c in CASES}
PAIRS = [(c, t) for c in CASES for t in DTYPES]
SHAPES = [(1, 1, 1, 1, 'ls-1'), (7, 1, 33, 65, 'ls-T'), (3, 1, 35, 63, 'ls-2'), (64, 1, 800, 500, 'gf-3'), (3, 5, 64, 130, 'ls-2'),
          (4100, 1, 65, 130, 'ls-1'), (16, 1, 128, 40, 'gf-8'), (300, 1, 1000, 1033, 'gf-3'), (65, 1, 1000, 1032, 'gf-2'),
          (33, 4, 1024, 1024, 'ls-2'), (130, 1, 2048, 2048, 'ls-1'), (130, 1, 2041, 2047, 'ls-T')]      # the table, restated

planes = T.planes


def pair_id(p) -> str:
    return f'{p[0].id}-{DTYPE_NAMES[p[1]]}'


def tile_class(c: Case) -> str:
    """The kernel lsq_linear_signx_wgrad(_half) runs for the case: the tile rule on (O, F)."""
    from quant.binary.binary_linear import QuantLinear
    return QuantLinear._tile_class(c.O, c.F)


@functools.lru_cache(maxsize=None)
def inputs(cid: str, dtype, seed_base: int = None) -> dict:
    """CPU tensors of a (case, type) (nothing writes into them afterwards): gy [M, O] and x [M, F] in ``dtype``; xs [kx, N] fp32;
    w [O, F] and ws [kw, O] fp32; edge_idx: the positions in sample 0 of the second sign's edge neighbours."""
    c = BY_ID[cid]
    base = SEED_BASE if seed_base is None else seed_base
    seed = base + CASES.index(c)
    tag = f'lwhalf.{cid}'
    m = c.N * c.T
    gy = detgen.normal(tag + '.gy', (m, c.O), seed=seed).to(dtype)
    x = detgen.normal(tag + '.x', L.x_shape(c), seed=seed, scale=1.2).to(dtype).clone()
    flat = x.view(-1)
    if flat.numel() >= 64:                            # (the single-product case keeps its one value)
        flat[::11] = 0.0
        flat[3::13] = -0.0
        flat[5::17] = ALPHA
        flat[7::19] = -ALPHA
        flat[2::31] = 1.0
        flat[4::37] = -1.0
        flat[6::41] = ALPHA + 0.5                     # beyond the clamp
        flat[8::43] = -2 * ALPHA
    edge_idx = L._place_edges(c, x, dtype) if planes(c.xs) >= 2 else []
    xs = torch.stack([v.float().reshape(c.N) for v in L.act_scales_cpu(c, x.float())]).contiguous()
    w = detgen.normal(tag + '.w', (c.O, c.F), seed=seed, scale=1.5 * c.F ** -0.5)
    try:
        sc = P.weight_scales(w.view(c.O, c.F, 1, 1), c.ws)
    except RuntimeError:                              # (a row too short for the scale solve: F = 1)
        sc = [torch.full((c.O,), 0.25 * 0.5 ** q) for q in range(planes(c.ws))]
    sc = [sc[0], sc[0]] if c.ws == 'ls-T' else list(sc)
    ws = torch.stack([s.float().view(-1) for s in sc]).contiguous()
    return {'gy': gy, 'x': x.view(m, c.F), 'xs': xs, 'w': w, 'ws': ws, 'edge_idx': edge_idx}


def as_fp32_case(c: Case, d: dict) -> dict:
    """The case in the form linear_wgrad_cases takes: the exact fp32 values of the 16-bit operands and the chain's signs."""
    gy, x = d['gy'].float(), d['x'].float()
    return dict(gy=gy, x=x, xs=d['xs'], n=c.N, t=c.T, m=c.N * c.T, f=c.F, o=c.O, signs=C.chain_signs(x, d['xs'], c.T, ALPHA))


def ref_a(c: Case, d: dict, device='cpu') -> torch.Tensor:
    """gy64^T . x_q64 [O, F] with the sign decisions of the fp32 chain."""
    return C.reference64(as_fp32_case(c, d), device)


def ref_b(d: dict, a64: torch.Tensor) -> torch.Tensor:
    """The weight chain's straight-through estimator (decisions from the fp32 chain on w, no clamp) applied to ``a64`` in fp64."""
    _, grad = T.chain64(d['w'], list(d['ws']), -1.0)
    return grad(a64)


def emulated64(c: Case, d: dict, lo_pass: bool = True) -> torch.Tensor:
    """The kernel's prescribed operands summed exactly: linear_wgrad_cases.emulated64 on the widened 16-bit values."""
    return C.emulated64(as_fp32_case(c, d), lo_pass)
