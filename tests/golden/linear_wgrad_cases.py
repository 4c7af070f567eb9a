"""Inputs and CPU references of the lsq_linear_signx_wgrad tests, shared by tests/test_linear_wgrad_host.py (the prescribed
arithmetic emulated on the CPU) and tests/test_gpu_linear_wgrad.py (the kernel): deterministic operands, the oracle's
activation scales, the signs of the quantizer chain in fp32 and the fp64 reference built from them."""

import torch

import detgen
from oracle import ref_port as P

BOUND = 1e-5          # |gwq - ref| <= BOUND * max |ref|: the project's figure for the bf16 hi + lo split
ALPHA = 2.0           # symmetric clamp in front of the quantizer
SCHEMES = ('ls-1', 'ls-2', 'ls-T', 'gf-2', 'gf-3', 'gf-8')
MS = (1, 63, 64, 65, 130, 1000, 4100)         # the summed dimension
OS = (1, 10, 33, 500)
FS = (10, 16, 65, 800)
# The first of 0, 1000, 2000, ... at which the prescribed arithmetic, summed exactly, is within half the bound at every
# accuracy case (tests/test_linear_wgrad_host.py asserts it; chosen on the CPU, never from the kernel).
SEED_BASE = 0


def planes(scheme: str) -> int:
    return {'ls-1': 1, 'ls-2': 2, 'ls-T': 2}.get(scheme) or int(scheme[3:])


def accuracy_cases(seed_base: int = None):
    """(scheme, M, O, F, seed): every scheme x every summed length; O and F rotate so that every value meets several schemes
    (O * F >= 10 everywhere: with fewer outputs max |ref| is a few random sums that may cancel)."""
    base = SEED_BASE if seed_base is None else seed_base
    out = []
    for si, scheme in enumerate(SCHEMES):
        for mi, m in enumerate(MS):
            out.append((scheme, m, OS[(mi + si) % 4], FS[(mi + 2 * si + 1) % 4], base + 100 * si + mi))
    return out


def oracle_scales(x: torch.Tensor, n: int, scheme: str, alpha: float = ALPHA) -> torch.Tensor:
    """[kx, N] scales of the per-sample quantizer (oracle.ref_port.quantize_activation on the clamped rows); ls-T: two planes
    of one scale."""
    xc = x if alpha < 0 else x.clamp(-alpha, alpha)
    sc = P.quantize_activation(xc.reshape(n, -1, 1, 1), scheme)[0]
    sc = [sc[0], sc[0]] if scheme == 'ls-T' else list(sc)
    return torch.stack([s.reshape(n).float() for s in sc]).contiguous()


def chain_signs(x: torch.Tensor, xs: torch.Tensor, t: int, alpha: float = ALPHA):
    """The +-1 planes [M, F] of the chain in fp32 as lsq_ste.hip forms them: xc = clamp(x), r_0 = 0, d_i = xc - r_i,
    b_i = (d_i >= 0 ? +1 : -1), r_{i+1} = r_i + v_i b_i with v_i = xs[i][m // t]."""
    xc = x if alpha < 0 else x.clamp(-alpha, alpha)
    r = torch.zeros_like(xc)
    out = []
    for p in range(xs.shape[0]):
        v = xs[p].repeat_interleave(t).view(-1, 1)
        d = xc - r
        b = torch.where(d >= 0, torch.ones_like(d), -torch.ones_like(d))
        out.append(b)
        r = r + v * b
    return out


def make(n, t, f, o, scheme, seed, xs=None, x=None):
    m = n * t
    gy = detgen.normal(f'linwgrad.gy.{seed}', (m, o), seed=seed)
    if x is None:
        x = detgen.normal(f'linwgrad.x.{seed}', (m, f), seed=seed, scale=1.2)
    if xs is None:
        xs = oracle_scales(x, n, scheme)
    return dict(gy=gy, x=x, xs=xs, n=n, t=t, m=m, f=f, o=o, signs=chain_signs(x, xs, t))


def scaled(c, p):
    """a_p = fl32(gy * xs[p][m // t]), [M, O] fp32."""
    return c['gy'] * c['xs'][p].repeat_interleave(c['t']).view(-1, 1)


def reference64(c, device='cpu'):
    """gy^T . (sum_p xs_p b_p) in fp64."""
    xq = 0
    for p, b in enumerate(c['signs']):
        xq = xq + c['xs'][p].double().repeat_interleave(c['t']).view(-1, 1) * b.double()
    return (c['gy'].double().to(device).t() @ xq.to(device)).cpu()


def emulated64(c, lo_pass=True, device='cpu'):
    """The kernel's operands -- a, hi = bf16(a) and lo = bf16(a - hi) in fp32 / bf16 -- summed exactly (fp64); without
    ``lo_pass`` one bf16 operand per product."""
    out = 0
    for p, b in enumerate(c['signs']):
        a = scaled(c, p)
        hi = a.bfloat16().float()
        v = hi.double()
        if lo_pass:
            v = v + (a - hi).bfloat16().double()
        out = out + (v.to(device).t() @ b.double().to(device)).cpu()
    return out
