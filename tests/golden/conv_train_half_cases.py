"""Cases, inputs and the fp64 reference of QuantConv2d's 16-bit train step (lsq_signw_conv2d_dgrad_half,
quant/binary/hip_train.py with ``hip_train_half``), shared by tests/test_conv_train_half_host.py and
tests/test_gpu_conv_train_half.py.  Plain Python on the CPU; nothing here touches a GPU.

The table is the 31 cases of tests/golden/conv_dgrad_cases.py (same ids, same weights and biases) in both 16-bit types, plus
``odd_planes``: 3 x 3, stride 1, N = 3, C = 5, 5 x 7 -- 35 elements a channel plane and 175 a sample, so with 2-byte elements
channel planes and samples start at addresses that are 2-byte- but not 4-byte-aligned.

``inputs(cid, dtype)``: x and gy of the fp32 case rounded into the type, then the special values of x placed AGAIN (rounding
moves them): +-0, +-alpha as the type rounds it, +-1 and, with two or more activation planes, in sample 0 the two
representable neighbours lo <= e < hi of the second sign's edge e = 1 + v_1 (v_1 - 1 where the clamp cuts 1 + v_1 off; no
edge where that is not positive), with v_1 computed from the rounded row; the placement and v_1 are iterated as in the fp32 table.  ``step64`` is
conv_dgrad_cases.step64 on the exact fp32 values of the rounded tensors.  ``shifted`` hands out a tensor as a view that
starts one element into its buffer.
"""

import functools

import torch

import conv_dgrad_cases as D
import detgen

Case = D.Case
DTYPES = (torch.bfloat16, torch.float16)
DTYPE_NAMES = {torch.bfloat16: 'bf16', torch.float16: 'fp16'}
# rounding unit of a type; fp16 also has half its smallest subnormal (2^-25) as an absolute term
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}

SYM3 = {'kind': 'symmetric', 'alpha': 3}          # (v_1 of the odd case is 1: under alpha = 2 the clamp would cut its edge's upper neighbour off)
ODD = Case('odd_planes', 'ls-2', 'ls-1', SYM3, 5, 7, 3, 3, 1, 1, 1, 1, 1, 1, 1, 3, 5, 7, True)
CASES = list(D.CASES) + [ODD]
BY_ID = {c.id: c for c in CASES}
PAIRS = [(c, t) for c in CASES for t in DTYPES]

planes, out_hw, conv_args, wide, patch_positions = D.planes, D.out_hw, D.conv_args, D.wide, D.patch_positions


def pair_id(p) -> str:
    return f'{p[0].id}-{DTYPE_NAMES[p[1]]}'


def alpha_in(c: Case, dtype) -> float:
    """The clamp bound as Tensor.clamp rounds it into ``dtype`` (-1: none).  Every bound of the table (2 and 1.5) is exact in
    both types, which is what lets ``step64`` be conv_dgrad_cases.step64 unchanged."""
    a = D.alpha_of(c.clamp)
    r = float(torch.tensor(a, dtype=dtype)) if a >= 0 else a
    assert r == a, (c.id, a, r)
    return r


def _fp32_inputs(c: Case) -> dict:
    """The fp32 tensors of the case: conv_dgrad_cases.inputs, or for the case added here the same recipe."""
    if c.id in D.BY_ID:
        return D.inputs(c.id)
    tag = f'cthalf.{c.id}'
    ho, wo = out_hw(c)
    cg = c.C // c.groups
    x = detgen.normal(tag + '.x', (c.N, c.C, c.H, c.W), scale=1.2)
    w = detgen.normal(tag + '.w', (c.O, cg, c.KH, c.KW), scale=1.5 * (cg * c.KH * c.KW) ** -0.5)
    b = detgen.normal(tag + '.b', (c.O,), scale=0.1) if c.bias else None
    gy = detgen.normal(tag + '.gy', (c.N, c.O, ho, wo))
    return {'x': x, 'w': w, 'b': b, 'gy': gy}


def neighbours(e: float, dtype, below: bool = False):
    """(lo, hi), adjacent values of ``dtype`` on either side of e: lo <= e < hi, or with ``below`` lo < e <= hi."""
    down, up = torch.tensor(float('-inf'), dtype=dtype), torch.tensor(float('inf'), dtype=dtype)
    t = torch.tensor(e, dtype=torch.float32).to(dtype)
    if float(t) > e or (below and float(t) == e):
        t = torch.nextafter(t, down)
    return float(t), float(torch.nextafter(t, up))


def edge_pair(c: Case, v1: float, dtype):
    """The two neighbours of the second sign's edge, one with the estimator open (|d_1| <= 1) and one with it closed: around
    1 + v1 the lower one is open, around v1 - 1 the upper one.  None where the clamp leaves no edge."""
    e = edge_of(c, v1, dtype)
    return None if e <= 0 else neighbours(e, dtype, below=e < v1)


def edge_of(c: Case, v1: float, dtype):
    """The edge of the second sign's estimator for a first scale v1: x > 0 with |x - v1| = 1 whose two neighbours in ``dtype``
    the clamp leaves alone: 1 + v1, else v1 - 1; <= 0 where neither exists (1 + v1 beyond the clamp and v1 <= 1)."""
    alpha = D.alpha_of(c.clamp)
    return 1.0 + v1 if alpha < 0 or neighbours(1.0 + v1, dtype)[1] <= alpha else v1 - 1.0


# positions in sample 0 of the edge's neighbours lo, hi, -lo, -hi: none is a multiple of 3, so the ls-2 / ls-T search of v_1,
# which reads every third element of the row (act_skip = 3), does not see them and the placement settles at once
EDGE_SLICES = (slice(10, None, 48), slice(34, None, 48), slice(11, None, 60), slice(41, None, 60))
assert all(sl.start % 3 and sl.step % 3 == 0 for sl in EDGE_SLICES)


def _place_edges(c: Case, x: torch.Tensor, dtype) -> list:
    """Place the edge's neighbours in sample 0 of ``x`` and return their positions.  v_1 depends on the row, so placement and
    v_1 are iterated until the neighbours placed are those of the row's own v_1 (gf-k: v_1 is a mean over the whole row and
    moves a little with every placement); where all positions of the slices do not settle, the first two of each are tried,
    then the first one."""
    base = x.clone()
    n = x[0].numel()
    for keep in (None, 2, 1):
        x.copy_(base)
        row0 = x[0].view(-1)
        idx = [list(range(n))[sl][:keep] for sl in EDGE_SLICES]
        placed = None
        for _ in range(8):
            pair = edge_pair(c, float(D.act_scales_cpu(c, x.float())[0][0]), dtype)
            if pair is None:                          # (no edge inside the clamp: nothing to place, as in the fp32 table)
                x.copy_(base)
                return []
            if pair == placed:
                return [i for part in idx for i in part]
            for part, val in zip(idx, (pair[0], pair[1], -pair[0], -pair[1])):
                row0[part] = val
            placed = pair
    raise AssertionError(f'{c.id}: the edge of the second sign does not settle')


@functools.lru_cache(maxsize=None)
def inputs(cid: str, dtype) -> dict:
    """CPU tensors of a (case, type) (nothing writes into them afterwards): x, gy in ``dtype``; w, b in fp32; alpha (the bound
    in the type); edge_idx: the positions in sample 0 of the second sign's edge neighbours; xscales: the per-sample plane scales [kx] x [N] of the torch formulation on x.float() (fp32)."""
    c = BY_ID[cid]
    d = _fp32_inputs(c)
    alpha = alpha_in(c, dtype)
    x = d['x'].to(dtype).clone()
    flat = x.view(-1)
    if flat.numel() >= 64:                            # (the single-product case keeps its one value)
        flat[::11] = 0.0
        flat[3::13] = -0.0
        if alpha >= 0:
            flat[5::17] = alpha
            flat[7::19] = -alpha
        flat[2::31] = 1.0
        flat[4::37] = -1.0
    edge_idx = _place_edges(c, x, dtype) if planes(c.xs) >= 2 else []
    xscales = [v.float().contiguous() for v in D.act_scales_cpu(c, x.float())]
    return {'x': x, 'w': d['w'], 'b': d['b'], 'gy': d['gy'].to(dtype), 'alpha': alpha, 'xscales': xscales, 'edge_idx': edge_idx}


def make_module(c: Case):
    """The case's QuantConv2d on the CPU in train mode (fp32 weight and bias)."""
    from quant.binary.binary_conv import QuantConv2d
    stride, padding, dilation, groups = conv_args(c)
    conv = QuantConv2d(c.xs, c.ws, c.C, c.O, (c.KH, c.KW), dict(c.clamp), stride=stride, padding=padding, dilation=dilation,
                       groups=groups, bias=c.bias)
    d = _fp32_inputs(c)
    with torch.no_grad():
        conv.weight.copy_(d['w'])
        if c.bias:
            conv.bias.copy_(d['b'])
    return conv.train()


@functools.lru_cache(maxsize=None)
def weight_scales(cid: str) -> torch.Tensor:
    """The weight plane scales [kw, O] of the torch formulation on the CPU."""
    conv = make_module(BY_ID[cid])
    with torch.no_grad():
        conv.w_approximate(conv.weight)
        return conv.w_approximate.plane_scales().detach().float().contiguous().clone()


def shifted(t: torch.Tensor, device=None, fill: float = -7.25):
    """(buffer, view): ``t`` as a contiguous view that starts ONE element into a buffer filled with ``fill`` (64 elements
    behind it too): with 2-byte elements the view's address is 2-byte- but not 4-byte-aligned."""
    buf = torch.full((t.numel() + 65,), fill, dtype=t.dtype, device=device if device is not None else t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def step64(c: Case, dtype, xscales, wscales) -> dict:
    """conv_dgrad_cases.step64 on the exact fp32 values of the rounded tensors, for given scales."""
    d = inputs(c.id, dtype)
    return D.step64(c, d['x'].float(), d['w'], d['b'], d['gy'].float(), xscales, wscales)
