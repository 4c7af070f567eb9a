"""The cases of lsq_train_wgrad_half (include/lsq_hip_train_half.h) as data: the geometries of
tests/test_gpu_train_wgrad_half.py, each the smallest shape at which one mechanism of csrc/train_half/lsq_wgrad_half.hip or of
csrc/train/lsq_wgrad_core.h (which it shares with lsq_train_wgrad, csrc/train/lsq_wgrad.hip) can go wrong, with the host-side
arithmetic of the two entries -- each file's count of chunks, lsq_wgrad_core.h's tile_plan() (tiles, the K split) and the
workspace -- restated independently (plan, plan_fp32), the geometries both entries refuse, a packer of activation planes and the
fp64 closed form.  tests/test_train_wgrad_half_host.py and tests/test_wgrad_core_host.py hold the table to what it says.  Plain
Python on the CPU; nothing here touches a GPU."""

import collections

import torch

Case = collections.namedtuple('Case', 'id C O N H W k stride pad scheme')


def _c(id, C, O, N, H, W, k, stride, pad, scheme):
    two = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    return Case(id, C, O, N, H, W, two(k), stride, two(pad), scheme)


#: C, O, N, H, W, (KH, KW), stride, (pad_h, pad_w), scheme
MECHANISMS = (
    _c('one_chunk', 3, 1, 1, 3, 3, 3, 1, 1, 'ls-1'),              # one chunk: S = 1, the direct store; one out-channel
    _c('sample_is_chunk', 64, 64, 3, 8, 8, 3, 1, 1, 'ls-2'),      # Ho Wo = 64: a sample is exactly one chunk
    _c('padded_7x7', 130, 96, 8, 7, 7, 3, 1, 1, 'ls-T'),          # Ho Wo = 49 (padded sample segments), three channel words with a
                                                                  # tail, O = 64 + 32; the fold
    _c('tail_9x9', 100, 65, 2, 9, 9, 3, 1, 1, 'gf-3'),            # Ho Wo = 81 (a sample's tail of 17), an O tail of 1, three planes
    _c('one_by_one', 64, 33, 5, 1, 1, 1, 1, 0, 'ls-1'),           # the 1 x 1 kernel (TT = 1), Ho Wo = 1: every k-step holds one
                                                                  # real position
    _c('taps_8x8', 72, 8, 1, 20, 12, (8, 8), 1, (7, 0), 'ls-1'),  # 64 taps (eight tap tiles), halo rows
    _c('eight_planes', 16, 33, 2, 8, 8, (4, 3), 1, (3, 2), 'gf-8'),   # eight planes, pad = k - 1 on both axes
    _c('s2_3x5', 20, 50, 2, 10, 11, (3, 5), 2, (2, 0), 'ls-2'),   # stride 2: the geometry of conv_train_half_cases' s2_3x5
    _c('resnet_s2_small', 64, 128, 16, 14, 14, 3, 2, 1, 'ls-2'),  # a ResNet stride-2 layer in small
)
#: the five 3 x 3 ResNet-18 layer shapes at batch 16 (C, O, H, stride), as tests/test_gpu_wgrad.py runs them
RESNET18 = tuple(_c(f'r18_{c}_{o}_{h}', c, o, 16, h, h, 3, s, 1, 'ls-2')
                 for c, o, h, s in ((64, 64, 56, 1), (64, 128, 56, 2), (128, 128, 28, 1), (256, 256, 14, 1), (512, 512, 7, 1)))
CASES = MECHANISMS + RESNET18
BY_ID = {c.id: c for c in CASES}
#: the cases of the exact anchors (integer operands): the first five
ANCHORS = MECHANISMS[:5]

DTYPES = (torch.bfloat16, torch.float16)
DTYPE_NAMES = {torch.bfloat16: 'bf16', torch.float16: 'fp16'}
DTYPE_CODES = {torch.bfloat16: 1, torch.float16: 2}           # LSQ_DTYPE_*
#: (scheme code, planes) of the quantizers
SCHEMES = {'ls-1': (1, 1), 'ls-2': (2, 2), 'ls-T': (3, 2), 'gf-3': (4, 3), 'gf-8': (4, 8)}
PAIRS = [(c, t) for c in CASES for t in DTYPES]

BOUND = 2e-6          # |g - g64| <= BOUND * sum |gy| |x_q| per element (tests/test_gpu_wgrad.py), |gb - gb64| <= BOUND * sum |gy|

K_STEP, CHUNK_STEPS, TILE, TAP_TILE, TARGET_GROUPS = 16, 4, 64, 9, 512       # csrc/train/lsq_wgrad_core.h


def pair_id(p) -> str:
    return f'{p[0].id}-{DTYPE_NAMES[p[1]]}'


def kx_of(c: Case) -> int:
    return SCHEMES[c.scheme][1]


def out_hw(c: Case):
    return (c.H + 2 * c.pad[0] - c.k[0]) // c.stride + 1, (c.W + 2 * c.pad[1] - c.k[1]) // c.stride + 1


Plan = collections.namedtuple('Plan', 'howo sps ksteps chunks TT ntc tiles S chunks_per_split slab_floats bias_floats')


def plan(c: Case) -> Plan:
    """plan() of csrc/train_half/lsq_wgrad_half.hip: a sample's positions padded to ``sps`` k-steps of 16, chunks of four
    k-steps; then tile_plan() of csrc/train/lsq_wgrad_core.h: tiles of 64 out-channels x one channel word x TT taps, S slices of
    whole chunks (about TARGET_GROUPS workgroups)."""
    ho, wo = out_hw(c)
    howo = ho * wo
    sps = -(-howo // K_STEP)
    ksteps = c.N * sps
    chunks = -(-ksteps // CHUNK_STEPS)
    kk = c.k[0] * c.k[1]
    tt = 1 if kk == 1 else TAP_TILE
    ntc = -(-kk // tt)
    n_ot = -(-c.O // TILE)
    tiles = n_ot * (-(-c.C // 64)) * ntc
    s = max(1, min(-(-TARGET_GROUPS // tiles), chunks))
    cps = -(-chunks // s)
    s = -(-chunks // cps)
    return Plan(howo, sps, ksteps, chunks, tt, ntc, tiles, s, cps, tiles * 4 * tt * 16 * 64, n_ot * TILE)


def workspace_bytes(c: Case, with_bias: bool) -> int:
    """The stated rule: nothing for one slice; S slabs, and with the bias S rows of bias partials behind them."""
    p = plan(c)
    return 0 if p.S == 1 else 4 * p.S * (p.slab_floats + (p.bias_floats if with_bias else 0))


PlanFp32 = collections.namedtuple('PlanFp32', 'howo chunks TT ntc tiles S chunks_per_split slab_floats workspace_bytes')


def plan_fp32(c: Case) -> PlanFp32:
    """lsq_train_wgrad (csrc/train/lsq_wgrad.hip): chunks are runs of 64 of the N Ho Wo positions, across samples; tiles and
    slices by the same rule as ``plan``; S slabs of workspace where there is more than one slice."""
    ho, wo = out_hw(c)
    chunks = -(-(c.N * ho * wo) // (K_STEP * CHUNK_STEPS))
    kk = c.k[0] * c.k[1]
    tt = 1 if kk == 1 else TAP_TILE
    ntc = -(-kk // tt)
    tiles = (-(-c.O // TILE)) * (-(-c.C // 64)) * ntc
    s = max(1, min(-(-TARGET_GROUPS // tiles), chunks))
    cps = -(-chunks // s)
    s = -(-chunks // cps)
    slab = tiles * 4 * tt * 16 * 64
    return PlanFp32(ho * wo, chunks, tt, ntc, tiles, s, cps, slab, 0 if s == 1 else 4 * s * slab)


E_NULL, E_SHAPE, E_SCHEME, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -3, -5, -6          # LSQ_E_* of include/lsq_hip.h
#: Geometries that lsq_train_wgrad and lsq_train_wgrad_half refuse, and the code of both: make_geom's arguments that differ from
#: REFUSAL_BASE.  The union of the lists of tests/test_wgrad_cabi.py and tests/test_train_wgrad_half_host.py.
REFUSAL_BASE = dict(n=4, c=64, h=8, w=8, o=32, kh=3, kw=3, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1)
REFUSED = (
    (dict(n=0), E_SHAPE),
    (dict(o=0), E_SHAPE),
    (dict(c=0), E_SHAPE),
    (dict(h=1, w=1, padding=(0, 0)), E_SHAPE),                    # kernel larger than the input
    (dict(h=1, kh=5), E_SHAPE),
    (dict(padding=(-1, 1)), E_SHAPE),
    (dict(stride=(0, 0)), E_SHAPE),
    (dict(o=30, groups=4), E_SHAPE),                              # O not divisible by groups
    (dict(groups=2), E_UNSUPPORTED),
    (dict(dilation=(2, 2)), E_UNSUPPORTED),
    (dict(dilation=(2, 1)), E_UNSUPPORTED),
    (dict(stride=(3, 3)), E_UNSUPPORTED),
    (dict(stride=(1, 2)), E_UNSUPPORTED),                         # unequal strides
    (dict(padding=(3, 1)), E_UNSUPPORTED),                        # pad > k - 1
    (dict(padding=(1, 3)), E_UNSUPPORTED),
    (dict(kh=9, kw=9, h=12, w=12), E_UNSUPPORTED),                # kernel > 8
    (dict(kh=9, h=16), E_UNSUPPORTED),
    (dict(o=65536), E_UNSUPPORTED),
    (dict(c=65536), E_UNSUPPORTED),
    (dict(n=1 << 20, h=64, w=64), E_UNSUPPORTED),                 # N Ho Wo >= 2^31
)


def pack_planes(bits: torch.Tensor, pad) -> torch.Tensor:
    """Activation planes in the layout of include/lsq_hip.h from ``bits`` [k, N, C, H, W] in {0, 1}: int64 words
    [k][N][ceil(C / 64)][H + 2 pad_h][W + 2 pad_w], bit c % 64 of word c // 64; the halo words and the bits of channels >= C are 0."""
    k, n, c, h, w = bits.shape
    gt = (c + 63) // 64
    full = torch.zeros((k, n, gt * 64, h, w), dtype=torch.int64)
    full[:, :, :c] = bits.to(torch.int64)
    words = torch.zeros((k, n, gt, h, w), dtype=torch.int64)
    for b in range(64):
        words |= full[:, :, b::64] << b          # (bit 63: the shift wraps into the sign, which is the bit pattern wanted)
    out = torch.zeros((k, n, gt, h + 2 * pad[0], w + 2 * pad[1]), dtype=torch.int64)
    out[:, :, :, pad[0]:pad[0] + h, pad[1]:pad[1] + w] = words
    return out.reshape(-1)


def unpack_planes(planes: torch.Tensor, k: int, c: Case) -> torch.Tensor:
    """bits [k, N, C, H, W] of planes in that layout (the interior: the halo is not part of x)."""
    gt, hp, wp = (c.C + 63) // 64, c.H + 2 * c.pad[0], c.W + 2 * c.pad[1]
    words = planes.cpu().view(k, c.N, gt, hp, wp)[:, :, :, c.pad[0]:c.pad[0] + c.H, c.pad[1]:c.pad[1] + c.W]
    bits = (words.unsqueeze(3) >> torch.arange(64).view(1, 1, 1, 64, 1, 1)) & 1
    return bits.reshape(k, c.N, gt * 64, c.H, c.W)[:, :, :c.C]


def xq64(bits: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """x_q = sum_p v_p[n] (2 bit_p - 1) in fp64; ``scales`` [k, N]."""
    k, n = scales.shape
    return ((2 * bits.to(torch.float64) - 1) * scales.cpu().to(torch.float64).view(k, n, 1, 1, 1)).sum(0)


def closed_form(c: Case, xq: torch.Tensor, gy: torch.Tensor) -> dict:
    """fp64: grad_wq, grad_b and the magnitudes of their bounds, sum |gy| |x_q| per weight and sum |gy| per out-channel."""
    gy64 = gy.cpu().to(torch.float64)
    wshape = (c.O, c.C) + c.k
    st = (c.stride, c.stride)
    return {'g': torch.nn.grad.conv2d_weight(xq, wshape, gy64, st, c.pad),
            'mag': torch.nn.grad.conv2d_weight(xq.abs(), wshape, gy64.abs(), st, c.pad),
            'gb': gy64.sum((0, 2, 3)), 'magb': gy64.abs().sum((0, 2, 3))}


def at_byte_offset(t: torch.Tensor, offset: int, device=None, fill: float = -7.25):
    """(buffer, view): ``t`` as a contiguous view that starts ``offset`` bytes (a multiple of the element size) into a buffer
    filled with ``fill``, 64 elements behind it too -- conv_train_half_cases.shifted for any offset."""
    first = offset // t.element_size()
    assert first * t.element_size() == offset
    buf = torch.full((t.numel() + first + 64,), fill, dtype=t.dtype, device=device if device is not None else t.device)
    view = buf[first:first + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view
