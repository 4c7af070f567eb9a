#!/usr/bin/env python3
"""Measurement of the 16-bit activation quantizer of QuantConv2d (lsq_act_quant_half) and of the module's eval forward on
both routes, one JSON document written to --out and printed.

  python scripts/conv_act_half_bench.py [--rounds R] [--out profiles/conv_act_half.json]

The graph-replay timing and the alternating rounds are those of scripts/linear_act_solve_half_bench.py.  Per shape (batch x
channels x height x width), activation scheme (ls-1, ls-2 free-running with skip 3, ls-2 with given scales) and input type
(bf16, fp16), microseconds of
  * `quant.half_kernel`: lsq_act_quant_half on the 16-bit batch,
  * `quant.cast_route`: x.float() -> lsq_act_quant, and `quant.cast_route_without_conversion`: lsq_act_quant on a batch that
    already is fp32,
  * `forward.half_kernel` / `forward.cast_route`: the whole eval forward of QuantConv2d(x_quant, 'ls-1', C, C, 3, padding=1)
    with act_half = True and act_half_kernel True / False (quantizer, lsq_xnor_conv2d, the cast of the result),
the median of the rounds, with the spread (max - min) / median of each.  `planes_equal` / `outputs_equal`: the two routes'
planes and outputs compared bit for bit on the timed inputs (computed scales other than v1 are sums in a different order).
The replays of one graph re-read the same batch, so from 103 MB down it may come from the 256 MiB Infinity Cache rather than
from HBM -- for both routes alike.  `landing` collects, per scheme and type, the speedups over the cast route next to the
spreads of both: QuantConv2d.act_half becomes True only in a change that has these numbers in hand."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402

from linear_fp_bench import DEV, graph_time  # noqa: E402

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
CLAMP = {'kind': 'symmetric', 'alpha': 2}
ALPHA = 2.0
SKIP = 3
SHAPES = [('resnet_56', 256, 64, 56, 56), ('resnet_28', 256, 128, 28, 28), ('resnet_14', 256, 256, 14, 14),
          ('resnet_7', 256, 512, 7, 7), ('cifar_32', 100, 64, 32, 32)]
# (name, x_quant, scales given)
SCHEMES = [('ls-1', 'ls-1', False), ('ls-2', 'ls-2', False), ('ls-2_given', 'ls-2', True)]


def module(xq, c, given, seed):
    from quant.binary.binary_conv import QuantConv2d
    from oracle import ref_port as P
    g = torch.Generator().manual_seed(seed)
    conv = QuantConv2d(xq, 'ls-1', c, c, 3, CLAMP, padding=1, **({'moving_average_mode': 'eval_only'} if given else {}))
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.05)
        conv.bias.copy_(torch.randn((c,), generator=g) * 0.1)
        for buf, v in zip(conv.w_approximate.cached_scales(), P.weight_scales(conv.weight, 'ls-1')):
            buf.copy_(v)
        if given:
            avg = conv.x_approximate.moving_avg_module.moving_average
            avg.copy_(torch.tensor([0.9 * 0.5 ** q for q in range(avg.numel())]).view_as(avg))
    conv.act_half = True
    assert conv.act_skip == SKIP
    return conv.eval().to(DEV)


def one_case(n, c, h, w, xq, given, rounds):
    from quant import _hip
    x32 = (torch.randn((n, c, h, w), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV)
    conv = module(xq, c, given, seed=2)
    scheme, k = conv.x_approximate.hip_scheme, conv.x_approximate.n_planes
    geom = _hip.make_geom(n, c, h, w, c, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    words = k * _hip.act_plane_words(geom)
    forced = conv.x_approximate.eval_scales(n)
    if forced is not None:
        forced = forced.to(device=DEV, dtype=torch.float32).contiguous()
    out = {'N': n, 'C': c, 'H': h, 'W': w, 'x_quant': xq, 'scales_given': given, 'skip': SKIP, 'bytes_x': 2 * n * c * h * w}
    variants, equal_planes, equal_out = {}, {}, {}
    for dt, dtype in DTYPES.items():
        x = x32.to(dtype)
        xf = x.float()
        ph, pc = (torch.zeros((words,), dtype=torch.int64, device=DEV) for _ in range(2))
        sh, sc = (torch.empty((k, n), device=DEV) for _ in range(2))

        def forward(half, x=x):
            conv.act_half_kernel = half
            with torch.no_grad():
                return conv(x)

        v = {f'{dt}.quant.half_kernel': lambda x=x, ph=ph, sh=sh: _hip.act_quant_half(x, geom, scheme, k, SKIP, ALPHA, ph, sh, forced),
             f'{dt}.quant.cast_route': lambda x=x, pc=pc, sc=sc: _hip.act_quant(x.float(), geom, scheme, k, SKIP, ALPHA, pc, sc, forced),
             f'{dt}.quant.cast_route_without_conversion': lambda xf=xf, pc=pc, sc=sc: _hip.act_quant(xf, geom, scheme, k, SKIP, ALPHA,
                                                                                                   pc, sc, forced),
             f'{dt}.forward.half_kernel': lambda forward=forward: forward(True),
             f'{dt}.forward.cast_route': lambda forward=forward: forward(False)}
        v[f'{dt}.quant.half_kernel']()
        v[f'{dt}.quant.cast_route']()
        yh, yc = v[f'{dt}.forward.half_kernel'](), v[f'{dt}.forward.cast_route']()
        torch.cuda.synchronize()
        equal_planes[dt] = bool(torch.equal(ph, pc))
        equal_out[dt] = bool(torch.equal(yh.view(torch.int16), yc.view(torch.int16)))
        variants.update(v)
    out['planes_equal'], out['outputs_equal'] = equal_planes, equal_out

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
    out['quant_speedup_vs_cast_route'] = {dt: us[f'{dt}.quant.cast_route'] / us[f'{dt}.quant.half_kernel'] for dt in DTYPES}
    out['quant_speedup_vs_fp32_rows'] = {dt: us[f'{dt}.quant.cast_route_without_conversion'] / us[f'{dt}.quant.half_kernel']
                                         for dt in DTYPES}
    out['forward_speedup_vs_cast_route'] = {dt: us[f'{dt}.forward.cast_route'] / us[f'{dt}.forward.half_kernel'] for dt in DTYPES}
    conv.act_half_kernel = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_act_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_act_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'clamp_alpha': ALPHA, 'skip': SKIP, 'shapes': {},
           'landing': {}}
    for name, n, c, h, w in SHAPES:
        if only and name not in only:
            continue
        for sname, xq, given in SCHEMES:
            r = res['shapes'].setdefault(name, {})[sname] = one_case(n, c, h, w, xq, given, args.rounds)
            for dt in DTYPES:
                res['landing'].setdefault(sname, {}).setdefault(dt, {})[name] = {
                    'forward_speedup_vs_cast_route': r['forward_speedup_vs_cast_route'][dt],
                    'quant_speedup_vs_cast_route': r['quant_speedup_vs_cast_route'][dt],
                    'quant_speedup_vs_fp32_rows': r['quant_speedup_vs_fp32_rows'][dt],
                    'spread_half_kernel': r['spread'][f'{dt}.forward.half_kernel'],
                    'spread_cast_route': r['spread'][f'{dt}.forward.cast_route']}
            print(name, sname, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res['landing']))


if __name__ == '__main__':
    main()
