"""Cases, inputs and CPU references of the lsq_xnor_conv2d_chain tests, shared by tests/test_chain_cases_host.py (the numpy
model against an independent slow implementation, the conditions the inputs must meet) and tests/test_gpu_chain.py (the kernel).

The model restates the arithmetic of the chain epilogue (csrc/lsq_xnor_mfma.hip, CHAIN) on a given fp32 ``y [N,O,Ho,Wo]``:
  * value ``v = clamp(y)``, or ``clamp(fma(y, s[o], t[o]))`` with a folded batch norm; sign bit ``v >= 0`` (-0.0 gives 1).  With
    an affine the bit is decided in fp64 from ``y*s + t``: the product of two fp32 numbers is exact in fp64 and the rounded sum
    keeps its sign; the clamp cannot flip a sign;
  * units (no affine: exact): per pixel and octet of channels 8g .. 8g+7 the sequential fp32 sum of ``|v|``, rounded to a
    multiple of 2^e (ties to even), summed per sample as integers; e = e2 - 31 with alpha = m 2^e2, 0.5 <= m < 1;
  * scale ``float32(units * 2^e / M)``, the division in fp64;
  * plane words in the layout of include/lsq_hip.h (``pack_ref`` of tests/test_gpu_parity.py).
Non-finite values are out of scope (the two kernels clamp a NaN differently; no caller produces one)."""

import functools
import math

import numpy as np
import torch

import detgen

ALPHAS = (0.37, 1.0, 1.3, 2.0, 6.0, 300.0)
ALPHA_IN = 2.0                      # the clamp of the producer's own input quantizer
XS_NOMINAL = 0.78                   # mean |clamp(N(0, 1), 2)|: what the producer's activation scale will be, for sizing wscales

# 3 x 3 producer geometries: id -> (N, H, W, stride, pad, dil)
GEOMS = {
    'a': (5, 3, 3, (2, 2), (1, 1), (1, 1)),      # 4 px per sample: a tile spans 8 samples, the last tile holds 20 px
    'b': (7, 4, 4, (1, 1), (1, 1), (1, 1)),      # 16 px: two samples per tile, half-empty last tile
    'c': (3, 5, 7, (1, 1), (1, 1), (1, 1)),      # 35 px: sample boundaries inside tiles at odd offsets
    'd': (2, 9, 13, (2, 1), (2, 1), (1, 1)),     # per-axis stride and padding
    'e': (2, 8, 6, (1, 1), (2, 2), (2, 1)),      # dil_h = 2 (eligible: only dil_w is checked)
    'f': (1, 14, 14, (1, 1), (1, 1), (1, 1)),    # a real layer shape
    'g': (8, 56, 56, (1, 1), (1, 1), (1, 1)),    # 784 tiles > 64 x 12 waves: a wave walks more than one tile
}
CHANNELS = (64, 128, 256, 512)
OUTS = (64, 128, 192)
NEXT_PADS = ((0, 0), (1, 1), (2, 1))
WPLANES = (1, 2, 3, 1)
# epilogue -> (act, res_pre, res_post); act in none | relu | prelu | prelu_c
EPILOGUES = {'none': ('none', False, False), 'relu': ('relu', False, False), 'prelu': ('prelu', False, False),
             'prelu_c': ('prelu_c', False, False), 'res_pre': ('relu', True, False), 'res_post': ('prelu', False, True),
             'res_both': ('none', True, True)}


class Case:
    def __init__(self, cid, geom, C, O, next_pad, wplanes, epilogue, alpha, affine, bias):
        self.id, self.geom, self.C, self.O, self.next_pad, self.wplanes = cid, geom, C, O, next_pad, wplanes
        self.epilogue, self.alpha, self.affine, self.bias = epilogue, alpha, affine, bias
        self.N, self.H, self.W, self.stride, self.pad, self.dil = GEOMS[geom]
        self.act, self.res_pre, self.res_post = EPILOGUES[epilogue]
        self.Ho = (self.H + 2 * self.pad[0] - self.dil[0] * 2 - 1) // self.stride[0] + 1
        self.Wo = (self.W + 2 * self.pad[1] - self.dil[1] * 2 - 1) // self.stride[1] + 1
        self.M = O * self.Ho * self.Wo                   # the consumer's row

    def __repr__(self):
        return self.id


def _cases():
    out = []
    for gi, geom in enumerate('abcdef'):
        for ci, C in enumerate(CHANNELS):
            i = 4 * gi + ci
            out.append(Case(f'{geom}{C}', geom, C, OUTS[(gi + ci) % 3], NEXT_PADS[(gi + 2 * ci) % 3], WPLANES[(gi + ci) % 4],
                            list(EPILOGUES)[i % 7], ALPHAS[i % 6], (i // 2) % 2 == 1, i % 3 != 0))
    out.append(Case('g64', 'g', 64, 128, (1, 1), 1, 'res_pre', 1.3, False, True))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def unit_exponent(alpha: float) -> int:
    """e of the unit 2^e: e2 - 31 with float32(alpha) = m 2^e2, 0.5 <= m < 1 (frexpf)."""
    return math.frexp(float(np.float32(alpha)))[1] - 31


# ------------------------------------------------------------------------------------------------------------- inputs
def _mean_taps(c: Case) -> float:
    """Kernel taps inside the image, averaged over the output pixels (border pixels of small images have few)."""
    def inside(size, out, stride, pad, dil):
        return [sum(0 <= o * stride - pad + k * dil < size for k in range(3)) for o in range(out)]
    th, tw = inside(c.H, c.Ho, c.stride[0], c.pad[0], c.dil[0]), inside(c.W, c.Wo, c.stride[1], c.pad[1], c.dil[1])
    return sum(a * b for a in th for b in tw) / (len(th) * len(tw))


@functools.lru_cache(maxsize=None)
def inputs(cid: str) -> dict:
    """CPU tensors of a case (nothing writes into them): x, w, wscales [k, O], bias, slope, res_pre, res_post, s, t.
    The value in front of the next clamp gets a standard deviation of about 0.8 alpha: through wscales without an affine,
    through the affine's magnitude (on a y of standard deviation 1) with one."""
    c = BY_ID[cid]
    tag = f'chain.{cid}'
    sigma = 1.0 if c.affine else 0.8 * c.alpha
    nres = int(c.res_pre) + int(c.res_post)
    conv_std = sigma * math.sqrt(1.0 - 0.16 * nres)
    x = detgen.normal(tag + '.x', (c.N, c.C, c.H, c.W), scale=1.0)
    planes_gain = math.sqrt(sum(4.0 ** -q for q in range(c.wplanes)))
    ws0 = detgen.uniform(tag + '.ws', (c.O,), 0.8, 1.2) * (conv_std / (XS_NOMINAL * math.sqrt(c.C * _mean_taps(c)) * planes_gain))
    wscales = torch.stack([ws0 * 0.5 ** q for q in range(c.wplanes)]).contiguous()
    w = detgen.normal(tag + '.w', (c.O, c.C, 3, 3), scale=1.2) * ws0.view(-1, 1, 1, 1)
    d = {'x': x, 'w': w.contiguous(), 'wscales': wscales, 'bias': None, 'slope': None, 'res_pre': None, 'res_post': None,
         's': None, 't': None}
    if c.bias:
        d['bias'] = detgen.normal(tag + '.bias', (c.O,), scale=0.1 * sigma)
    if c.act == 'prelu':
        d['slope'] = torch.tensor([0.25])
    if c.act == 'prelu_c':
        slope = detgen.uniform(tag + '.slope', (c.O,), 0.1, 0.4)
        slope[5::16] = -0.2                                # (a negative slope folds the negative side over)
        d['slope'] = slope
    shape = (c.N, c.O, c.Ho, c.Wo)
    if c.res_pre:
        d['res_pre'] = detgen.normal(tag + '.res_pre', shape, scale=0.4 * sigma)
    if c.res_post:
        d['res_post'] = detgen.normal(tag + '.res_post', shape, scale=0.4 * sigma)
    if c.affine:
        s = detgen.uniform(tag + '.s', (c.O,), 0.8, 1.2) * (0.8 * c.alpha)
        s[1::3] *= -1.0                                    # both signs
        t = detgen.normal(tag + '.t', (c.O,), scale=0.1 * c.alpha)
        for ch, zero in ((3, 0.0), (7, -0.0), (40, 0.0), (c.O - 1, -0.0)):     # the value is exactly +-0 whatever y is: bit 1
            s[ch] = 0.0
            t[ch] = zero
        d['s'], d['t'] = s.contiguous(), t.contiguous()
    return d


def sign_pm1(t: torch.Tensor) -> torch.Tensor:
    return torch.where(t >= 0, 1.0, -1.0).to(torch.float64)


def weight_signs(w: torch.Tensor, wscales: torch.Tensor):
    """lsq_pack_weight's planes: bit_q = (w - result) >= 0, result += +-u_q, in fp32."""
    out, result = [], torch.zeros_like(w)
    for u in wscales:
        bit = (w - result) >= 0
        out.append(torch.where(bit, 1.0, -1.0).to(torch.float64))
        uu = u.view(-1, 1, 1, 1).expand_as(w)
        result = result + torch.where(bit, uu, -uu)
    return out


def epilogue64(c: Case, d: dict, acc: torch.Tensor) -> torch.Tensor:
    """y = act(conv + bias + res_pre) + res_post in fp64."""
    y = acc
    if d['bias'] is not None:
        y = y + d['bias'].double().view(1, -1, 1, 1)
    if d['res_pre'] is not None:
        y = y + d['res_pre'].double()
    if c.act == 'relu':
        y = y.clamp_min(0.0)
    elif c.act in ('prelu', 'prelu_c'):
        sl = d['slope'].double()
        sl = sl.view(1, -1, 1, 1) if sl.numel() > 1 else sl
        y = torch.where(y > 0, y, sl * y)
    if d['res_post'] is not None:
        y = y + d['res_post'].double()
    return y


def conv64(c: Case, xb: torch.Tensor, xs: torch.Tensor, d: dict) -> torch.Tensor:
    """The fp64 convolution of the sign tensors with their scales, epilogue included: xb [N,C,H,W] of +-1 (fp64), xs [N]."""
    acc = torch.zeros((c.N, c.O, c.Ho, c.Wo), dtype=torch.float64)
    for u, sq in zip(d['wscales'], weight_signs(d['w'], d['wscales'])):
        ints = torch.nn.functional.conv2d(xb, sq, None, c.stride, c.pad, c.dil)
        acc = acc + ints * u.double().view(1, -1, 1, 1)
    return epilogue64(c, d, acc * xs.double().view(-1, 1, 1, 1))


@functools.lru_cache(maxsize=None)
def reference(cid: str) -> torch.Tensor:
    """y of the case in fp64 on the CPU (computed once, shared, left unchanged): the producer's input quantized ls-1 under
    ALPHA_IN with the fp64 mean as its scale."""
    c, d = BY_ID[cid], inputs(cid)
    xs = d['x'].double().clamp(-ALPHA_IN, ALPHA_IN).abs().mean(dim=(1, 2, 3))
    return conv64(c, sign_pm1(d['x']), xs, d)


def pre_clamp64(y, s, t) -> np.ndarray:
    """The value in front of the next layer's clamp, in fp64."""
    z = np.asarray(y, dtype=np.float64)
    if s is not None:
        z = z * np.asarray(s, dtype=np.float64).reshape(1, -1, 1, 1) + np.asarray(t, dtype=np.float64).reshape(1, -1, 1, 1)
    return z


def mean64(y, s, t, alpha: float) -> np.ndarray:
    """Per-sample fp64 mean of |clamp(.)|: what the scale approximates."""
    a = float(np.float32(alpha))
    return np.abs(np.clip(pre_clamp64(y, s, t), -a, a)).mean(axis=(1, 2, 3))


# -------------------------------------------------------------------------------------------- the epilogue's arithmetic
def model_bits(y: np.ndarray, s, t, alpha: float) -> np.ndarray:
    """bool [N,O,Ho,Wo]: the sign bits the epilogue writes for fp32 y."""
    y = np.asarray(y, dtype=np.float32)
    if s is None:
        a = np.float32(alpha)
        return np.clip(y, -a, a) >= 0                     # (-0.0 >= 0: bit 1)
    return pre_clamp64(y, s, t) >= 0


def octet_sums(av: np.ndarray) -> np.ndarray:
    """fp32 [N,O,P] -> fp32 [N,O/8,P]: ((((((a0+a1)+a2)+a3)+a4)+a5)+a6)+a7 over each octet of channels, fp32 adds."""
    n, o, p = av.shape
    a = np.asarray(av, dtype=np.float32).reshape(n, o // 8, 8, p)
    acc = a[:, :, 0].copy()
    for k in range(1, 8):
        acc = (acc + a[:, :, k]).astype(np.float32)
    return acc


def round_to_units(octs: np.ndarray, e: int) -> np.ndarray:
    """fp32 sums -> int64 multiples of 2^e, ties to even (the division by a power of two is exact in fp64)."""
    return np.rint(np.asarray(octs, dtype=np.float64) / 2.0 ** e).astype(np.int64)


def model_units(y: np.ndarray, alpha: float) -> np.ndarray:
    """int64 [N]: the row sums of |clamp(y)| in units of 2^e, exactly as the epilogue adds them (no affine)."""
    y = np.asarray(y, dtype=np.float32)
    a = np.float32(alpha)
    av = np.abs(np.clip(y, -a, a)).reshape(y.shape[0], y.shape[1], -1)
    return round_to_units(octet_sums(av), unit_exponent(alpha)).sum(axis=(1, 2))


def model_scale(units, alpha: float, M: int) -> np.ndarray:
    """fp32 [N]: float32(units * 2^e / M), the arithmetic in fp64 as the consumer side does it."""
    u = np.asarray(units, dtype=np.int64).astype(np.float64)
    return (u * 2.0 ** unit_exponent(alpha) / float(M)).astype(np.float32)


def model_words(bits: np.ndarray, next_pad) -> np.ndarray:
    """uint64 [N, O/64, Ho + 2 ph, Wo + 2 pw]: the next layer's plane, halo zero."""
    from test_gpu_parity import pack_ref
    return pack_ref(bits, 1, next_pad)
