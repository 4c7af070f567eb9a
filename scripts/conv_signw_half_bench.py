#!/usr/bin/env python3
"""Measurement of the 16-bit-activation sign-weight convolution (lsq_signw_conv2d_half) against the cast route and against
the dense 16-bit convolution, one JSON document written to --out and printed.

  python scripts/conv_signw_half_bench.py [--rounds R] [--only names] [--out profiles/conv_signw_half.json]

The graph-replay timing and the alternating rounds are those of scripts/conv_act_half_bench.py.  Per shape (batch x channels
x height x width -> out-channels, 3x3 pad 1 at stride 1 or 2), weight scheme (ls-1, ls-2) and input type (bf16, fp16),
microseconds of
  * `kernel.half`: lsq_signw_conv2d_half on the 16-bit batch, 16-bit output,
  * `kernel.cast_route`: x.float() -> lsq_signw_conv2d (given its prepared weights, `cast_route_prepared_weights`: the
    persistent 3x3 fast path where the call takes it) -> .to(dtype),
  * `forward.half` / `forward.cast_route`: the whole eval forward of QuantConv2d('fp', w, C, O, 3, padding=1) with
    fp_half = True and fp_half_kernel True / False,
  * `forward.autocast_torch`: _forward_torch under an autocast of the type (w_q rounded into the type, dense MIOpen),
the median of the rounds, with the spread (max - min) / median of each, and `error`: max |y - y64| / max |y64| of the three
forwards against F.conv2d in fp64 on the clamped 16-bit batch (computed on the GPU, once).
`landing` collects, per scheme and type, the speedups over the cast route next to the spreads of both: QuantConv2d.fp_half
becomes True only in a change that has these numbers in hand, and only for the shapes where the kernel wins beyond the
spreads."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from linear_fp_bench import DEV, graph_time  # noqa: E402

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
CLAMP = {'kind': 'symmetric', 'alpha': 2}
# (name, N, C, H, W, O, stride): the four ResNet-18 layer shapes and the three stride-2 ones at batch 256, the CIFAR shape,
# one small batch
SHAPES = [('resnet_56', 256, 64, 56, 56, 64, 1), ('resnet_28', 256, 128, 28, 28, 128, 1), ('resnet_14', 256, 256, 14, 14, 256, 1),
          ('resnet_7', 256, 512, 7, 7, 512, 1), ('resnet_56_s2', 256, 64, 56, 56, 128, 2), ('resnet_28_s2', 256, 128, 28, 28, 256, 2),
          ('resnet_14_s2', 256, 256, 14, 14, 512, 2), ('cifar_32', 100, 64, 32, 32, 64, 1), ('batch8_28', 8, 128, 28, 28, 128, 1)]
SCHEMES = ('ls-1', 'ls-2')


def module(ws, c, o, stride, seed):
    from quant.binary.binary_conv import QuantConv2d
    from oracle import ref_port as P
    g = torch.Generator().manual_seed(seed)
    conv = QuantConv2d('fp', ws, c, o, 3, CLAMP, padding=1, stride=stride)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.05)
        conv.bias.copy_(torch.randn((o,), generator=g) * 0.1)
        for buf, v in zip(conv.w_approximate.cached_scales(), P.weight_scales(conv.weight, ws)):
            buf.copy_(v)
    conv.fp_half = True
    return conv.eval().to(DEV)


def one_case(n, c, h, w, o, stride, ws, rounds):
    from quant import _hip
    x32 = (torch.randn((n, c, h, w), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV)
    conv = module(ws, c, o, stride, seed=2)
    geom = _hip.make_geom(n, c, h, w, o, 3, 3, (stride, stride), (1, 1), (1, 1), 1)
    wbits, _, wscales, wprep = conv._packed_weights(geom, _hip)
    bias = conv.bias.detach()
    ho, wo = _hip.out_hw(geom)
    out = {'N': n, 'C': c, 'H': h, 'W': w, 'O': o, 'stride': stride, 'w_quant': ws, 'planes': int(wscales.shape[0]),
           'plan': int(_hip.conv_half_lib().lsq_signw_conv2d_half_plan(ctypes.byref(geom))),
           'cast_route_prepared_weights': wprep is not None, 'bytes_x': 2 * n * c * h * w}
    variants, errors = {}, {}
    with torch.no_grad():
        wq64 = conv.w_approximate(conv.weight).double()
    for dt, dtype in DTYPES.items():
        x = x32.to(dtype)
        alpha = conv._alpha_in(dtype)
        y32 = torch.empty((n, o, ho, wo), device=DEV)

        def forward(half, x=x):
            conv.fp_half_kernel = half
            with torch.no_grad():
                return conv(x)

        def autocast(x=x, dtype=dtype):
            with torch.no_grad(), torch.autocast('cuda', dtype=dtype):
                return conv._forward_torch(x)

        def cast_kernel(x=x, alpha=alpha, y32=y32, dtype=dtype):
            _hip.signw_conv2d(x.float(), alpha, wbits, wscales, bias, geom, y32, wprep=wprep)
            return y32.to(dtype)

        v = {f'{dt}.kernel.half': lambda x=x, alpha=alpha: _hip.signw_conv2d_half(x, alpha, wbits, wscales, bias, geom),
             f'{dt}.kernel.cast_route': cast_kernel,
             f'{dt}.forward.half': lambda forward=forward: forward(True),
             f'{dt}.forward.cast_route': lambda forward=forward: forward(False),
             f'{dt}.forward.autocast_torch': autocast}
        y64 = F.conv2d(x.clamp(-2, 2).double(), wq64, bias.double(), stride, 1)
        scale = y64.abs().max().item()
        for name in ('forward.half', 'forward.cast_route', 'forward.autocast_torch'):
            errors[f'{dt}.{name}'] = (v[f'{dt}.{name}']().double() - y64).abs().max().item() / scale
        del y64
        torch.cuda.synchronize()
        variants.update(v)
    out['error'] = errors

    chain = 10
    reps = 5
    for fn in variants.values():                      # warm-up of every variant, then rounds with the variants alternating
        graph_time(fn, 1, chain)
    samples = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            samples[name].append(graph_time(fn, reps, chain))
    out['us'] = {name: statistics.median(s) for name, s in samples.items()}
    out['spread'] = {name: (max(s) - min(s)) / statistics.median(s) for name, s in samples.items()}
    out['graph_chain'] = chain
    us = out['us']
    out['kernel_speedup_vs_cast_route'] = {dt: us[f'{dt}.kernel.cast_route'] / us[f'{dt}.kernel.half'] for dt in DTYPES}
    out['forward_speedup_vs_cast_route'] = {dt: us[f'{dt}.forward.cast_route'] / us[f'{dt}.forward.half'] for dt in DTYPES}
    out['forward_speedup_vs_autocast_torch'] = {dt: us[f'{dt}.forward.autocast_torch'] / us[f'{dt}.forward.half'] for dt in DTYPES}
    conv.fp_half_kernel = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_signw_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_signw_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'clamp_alpha': CLAMP['alpha'], 'shapes': {}, 'landing': {}}
    for name, n, c, h, w, o, stride in SHAPES:
        if only and name not in only:
            continue
        for ws in SCHEMES:
            r = res['shapes'].setdefault(name, {})[ws] = one_case(n, c, h, w, o, stride, ws, args.rounds)
            for dt in DTYPES:
                res['landing'].setdefault(ws, {}).setdefault(dt, {})[name] = {
                    'forward_speedup_vs_cast_route': r['forward_speedup_vs_cast_route'][dt],
                    'kernel_speedup_vs_cast_route': r['kernel_speedup_vs_cast_route'][dt],
                    'forward_speedup_vs_autocast_torch': r['forward_speedup_vs_autocast_torch'][dt],
                    'spread_half': r['spread'][f'{dt}.forward.half'],
                    'spread_cast_route': r['spread'][f'{dt}.forward.cast_route']}
            print(name, ws, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res['landing']))


if __name__ == '__main__':
    main()
