"""Cases, inputs and the fp64 reference of QuantLinear's 16-bit train step (lsq_linear_signw_dgrad_half,
quant/binary/hip_train_linear.py with ``hip_train_half``), shared by tests/test_linear_train_half_host.py and
tests/test_gpu_linear_train_half.py.  Plain Python on the CPU; nothing here touches a GPU.

A case is (N, T, F, O, xs, ws, clamp, bias): an input [N, F] (T = 1) or [N, T, F], M = N T rows.  The table holds the smallest
shapes that reach each piece of the kernels -- ``kernel`` names the class the tile rule of lsq_linear_signw_dgrad puts the case
in (``QuantLinear._tile_class`` with F in O's place): the split kernel with one product, ragged rows / columns / summed
dimension, odd F and O (with 2-byte elements rows then start at addresses that are 2-byte- but not 4-byte-aligned), LeNet's
fc1 and T > 1 with sample boundaries inside a 32-row tile; 64 x 64 tiles with ragged edges and with T = 4; 128 x 128 tiles.

``inputs(cid, dtype)``: x and gy from detgen rounded into the type, then the special values of x placed AGAIN (rounding moves
them): +-0, +-alpha as the type rounds it, +-1 and, with two or more activation planes, in sample 0 the two representable
neighbours of the second sign's edge (conv_train_half_cases.edge_pair), at positions that are no multiple of 3, so that the
ls-2 / ls-T search of v_1, which reads every third element of the row (act_skip = 3), does not see them.  ``step64`` is the
step in fp64 on the exact values of the rounded tensors for given scales: the quantizer chain of train_step_cases.chain64
(decisions from the fp32 chain, values in fp64) around fp64 matrix products; the weight scales of the table are
oracle.ref_port.weight_scales'.
"""

import collections
import functools

import torch

import detgen
import train_step_cases as T
from conv_train_half_cases import DTYPE_NAMES, DTYPES, TINY, UNIT, edge_of, edge_pair, neighbours, shifted  # noqa: F401
from oracle import ref_port as P

Case = collections.namedtuple('Case', 'id N T F O xs ws clamp bias kernel')

IDENT, SYM2, SYM15 = T.IDENT, T.SYM2, T.SYM15
SYM3 = {'kind': 'symmetric', 'alpha': 3}

CASES = [
    # ---- the split kernel: fewer than 256 tiles of 64 x 64 in M x F
    Case('one_product', 1, 1, 1, 1, 'fp', 'ls-1', IDENT, True, 'split'),
    Case('ragged', 7, 1, 33, 65, 'ls-T', 'ls-2', SYM3, True, 'split'),
    Case('odd_rows', 3, 1, 35, 63, 'ls-2', 'gf-3', SYM3, True, 'split'),          # odd F and O
    Case('lenet_fc1', 64, 1, 800, 10, 'gf-3', 'ls-1', SYM3, False, 'split'),
    Case('rows_per_sample', 3, 5, 64, 130, 'ls-1', 'gf-8', SYM2, True, 'split'),  # T > 1: sample boundaries inside a tile
    # ---- 64 x 64 tiles: at least 256 of them, fewer than 256 of 128 x 128
    Case('tiles64_ragged', 1000, 1, 1033, 65, 'fp', 'ls-2', SYM15, True, 'small'),
    Case('tiles64_t4', 250, 4, 1024, 64, 'ls-2', 'ls-1', SYM3, True, 'small'),
    # ---- 128 x 128 tiles
    Case('tiles128', 2100, 1, 2000, 130, 'ls-1', 'gf-3', IDENT, True, 'big'),
]
BY_ID = {c.id: c for c in CASES}
PAIRS = [(c, t) for c in CASES for t in DTYPES]

planes, alpha_of = T.planes, T.alpha_of


def pair_id(p) -> str:
    return f'{p[0].id}-{DTYPE_NAMES[p[1]]}'


def tile_class(c: Case) -> str:
    """The kernel lsq_linear_signw_dgrad(_half) runs for the case: QuantLinear._tile_class with F in O's place."""
    from quant.binary.binary_linear import QuantLinear
    return QuantLinear._tile_class(c.N * c.T, c.F)


def x_shape(c: Case):
    return (c.N, c.F) if c.T == 1 else (c.N, c.T, c.F)


def gy_shape(c: Case):
    return x_shape(c)[:-1] + (c.O,)


def alpha_in(c: Case, dtype) -> float:
    """The clamp bound as Tensor.clamp rounds it into ``dtype`` (-1: none).  Every bound of the table is exact in both types,
    which is what lets ``step64`` use the bound itself."""
    a = alpha_of(c.clamp)
    r = float(torch.tensor(a, dtype=dtype)) if a >= 0 else a
    assert r == a, (c.id, a, r)
    return r


def act_scales_cpu(c: Case, x: torch.Tensor) -> list:
    """The per-sample plane scales [kx] x [N] of the torch formulation's activation quantizer for fp32 ``x`` (CPU)."""
    return T.act_scales_cpu(c, x.reshape(c.N, c.T * c.F, 1, 1))


# positions in sample 0 of the edge's neighbours lo, hi, -lo, -hi: none is a multiple of 3 and the first of each lies inside
# the shortest row of the table that has two planes (33 elements)
EDGE_SLICES = (slice(10, None, 48), slice(22, None, 48), slice(13, None, 60), slice(25, None, 60))
assert all(sl.start % 3 and sl.step % 3 == 0 for sl in EDGE_SLICES)


def _place_edges(c: Case, x: torch.Tensor, dtype) -> list:
    """Place the edge's neighbours in sample 0 of ``x`` and return their positions; v_1 depends on the row (gf-k: on all of
    it), so placement and v_1 are iterated until the neighbours placed are those of the row's own v_1 -- with all positions
    of the slices, else the first two of each, else the first."""
    base = x.clone()
    n = x[0].numel()
    for keep in (None, 2, 1):
        x.copy_(base)
        row0 = x[0].view(-1)
        idx = [list(range(n))[sl][:keep] for sl in EDGE_SLICES]
        placed = None
        for _ in range(8):
            pair = edge_pair(c, float(act_scales_cpu(c, x.float())[0][0]), dtype)
            if pair is None:                          # (no edge inside the clamp: nothing to place)
                x.copy_(base)
                return []
            if pair == placed:
                return [i for part in idx for i in part]
            for part, val in zip(idx, (pair[0], pair[1], -pair[0], -pair[1])):
                row0[part] = val
            placed = pair
    raise AssertionError(f'{c.id}: the edge of the second sign does not settle')


@functools.lru_cache(maxsize=None)
def _fp32_inputs(cid: str) -> dict:
    c = BY_ID[cid]
    tag = f'lthalf.{cid}'
    x = detgen.normal(tag + '.x', x_shape(c), scale=1.2)
    w = detgen.normal(tag + '.w', (c.O, c.F), scale=1.5 * c.F ** -0.5)
    b = detgen.normal(tag + '.b', (c.O,), scale=0.1) if c.bias else None
    gy = detgen.normal(tag + '.gy', gy_shape(c))
    return {'x': x, 'w': w, 'b': b, 'gy': gy}


@functools.lru_cache(maxsize=None)
def inputs(cid: str, dtype) -> dict:
    """CPU tensors of a (case, type) (nothing writes into them afterwards): x, gy in ``dtype``; w, b in fp32; alpha (the bound
    in the type); edge_idx: the positions in sample 0 of the second sign's edge neighbours; xscales: the per-sample plane
    scales [kx] x [N] of the torch formulation on x.float() (fp32)."""
    c = BY_ID[cid]
    d = _fp32_inputs(cid)
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
    xscales = [v.float().contiguous() for v in act_scales_cpu(c, x.float())]
    return {'x': x, 'w': d['w'], 'b': d['b'], 'gy': d['gy'].to(dtype), 'alpha': alpha, 'xscales': xscales, 'edge_idx': edge_idx}


def make_module(c: Case):
    """The case's QuantLinear on the CPU in train mode (fp32 weight and bias)."""
    from quant.binary.binary_linear import QuantLinear
    lin = QuantLinear(c.xs, c.ws, c.F, c.O, dict(c.clamp), bias=c.bias)
    d = _fp32_inputs(c.id)
    with torch.no_grad():
        lin.weight.copy_(d['w'])
        if c.bias:
            lin.bias.copy_(d['b'])
    return lin.train()


@functools.lru_cache(maxsize=None)
def weight_scales(cid: str) -> torch.Tensor:
    """The weight plane scales [kw, O] (ls-T: two planes of one scale) of oracle.ref_port on the CPU; a row too short for the
    scale solve (F = 1) gets 0.25 * 2^-q as in tests/test_gpu_linear_train.py."""
    c = BY_ID[cid]
    w = _fp32_inputs(cid)['w']
    try:
        sc = P.weight_scales(w.view(c.O, c.F, 1, 1), c.ws)
    except RuntimeError:
        sc = [torch.full((c.O,), 0.25 * 0.5 ** q) for q in range(planes(c.ws))]
    sc = [sc[0], sc[0]] if c.ws == 'ls-T' else list(sc)
    return torch.stack([s.float().view(-1) for s in sc]).contiguous()


def step64(c: Case, dtype, xscales, wscales) -> dict:
    """One train step of QuantLinear in fp64 on the CPU, on the exact values of the rounded tensors, for given scales
    (``xscales`` [kx][N], empty or None for fp activations; ``wscales`` [kw][O]).  Returns y, gx, gxq, m_x, gw, gb: m_x is the
    estimator's multiplier, gx = m_x * gxq."""
    d = inputs(c.id, dtype)
    m = c.N * c.T
    x = d['x'].float().reshape(c.N, c.T * c.F)
    gy64 = d['gy'].double().reshape(m, c.O)
    xs = [] if xscales is None else [v.detach().cpu().float().reshape(-1) for v in xscales]
    ws = [u.detach().cpu().float().reshape(-1) for u in wscales]
    xq, gradx = T.chain64(x, xs, d['alpha'])
    wq, gradw = T.chain64(d['w'].float(), ws, -1.0)
    xq2 = xq.reshape(m, c.F)
    y = xq2 @ wq.t()
    if d['b'] is not None:
        y = y + d['b'].double()
    gxq = (gy64 @ wq).reshape(c.N, c.T * c.F)
    m_x = gradx(torch.ones_like(gxq))
    shape = x_shape(c)
    return {'y': y.reshape(gy_shape(c)), 'gx': gradx(gxq).reshape(shape), 'gxq': gxq.reshape(shape), 'm_x': m_x.reshape(shape),
            'gw': gradw(gy64.t() @ xq2), 'gb': gy64.sum(0)}
