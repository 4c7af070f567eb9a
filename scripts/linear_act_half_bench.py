#!/usr/bin/env python3
"""Measurement of the activation quantizer for bf16 / fp16 rows (lsq_linear_act_quant_half) and of QuantLinear's eval forward
on both routes, one JSON document written to --out and printed.

  python scripts/linear_act_half_bench.py [--rounds R] [--out profiles/linear_act_quant_half.json]

The graph-replay timing and the alternating rounds are those of scripts/linear_fp_bench.py / linear_half_bench.py.  Per shape
(rows x features x outputs), activation scheme (ls-1 free-running; ls-2 with given scales, i.e. a moving average in eval
mode) and input type (bf16, fp16), microseconds of
  * `quant.half_kernel`: lsq_linear_act_quant_half on the 16-bit rows,
  * `quant.cast_route`: x.float() -> lsq_act_quant, and `quant.cast_route_without_conversion`: lsq_act_quant on rows that
    already are fp32,
  * `forward.half_kernel` / `forward.cast_route`: the whole eval forward of QuantLinear(x_quant, 'ls-1') with
    act_half_kernel True / False (quantizer, lsq_linear_xnor, the cast of the result),
the median of the rounds, with the spread (max - min) / median of each.  `planes_equal` / `outputs_equal`: the two routes'
planes and outputs compared bit for bit on the timed inputs (ls-1 free-running: the planes; the scales of the two kernels
are sums in different orders).  `bytes_x` is what the new kernel must read; the replays of one graph re-read the same rows,
so from 67 MB down they may come from the 256 MiB Infinity Cache rather than from HBM -- for both routes alike.
`landing` collects, per scheme and type, the forward's speedup over the cast route next to the spreads of both:
QuantLinear.act_half_kernel stays True only if no shape is slower beyond them."""
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
SHAPES = [('lenet_fc1', 64, 800, 500), ('resnet18_head', 256, 512, 1000), ('decode_m1', 1, 4096, 4096),
          ('decode_m16', 16, 4096, 4096), ('mlp', 8192, 4096, 4096)]
SCHEMES = [('ls-1', 'free-running'), ('ls-2', 'given scales')]


def module(xq, f, o, seed):
    from quant.binary import QuantLinear
    from oracle import ref_port as P
    g = torch.Generator().manual_seed(seed)
    lin = QuantLinear(xq, 'ls-1', f, o, CLAMP, moving_average_mode='eval_only' if xq == 'ls-2' else 'off')
    with torch.no_grad():
        lin.weight.copy_(torch.randn((o, f), generator=g) * 0.05)
        lin.bias.copy_(torch.randn((o,), generator=g) * 0.1)
        for buf, v in zip(lin.w_approximate.cached_scales(), P.weight_scales(lin.weight.view(o, f, 1, 1), 'ls-1')):
            buf.copy_(v)
        if xq == 'ls-2':
            lin.x_approximate.moving_avg_module.moving_average.copy_(torch.tensor([0.9, 0.4]))
    return lin.eval().to(DEV)


def one_case(m, f, o, xq, rounds):
    from quant import _hip
    x32 = (torch.randn((m, f), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV)
    lin = module(xq, f, o, seed=2)
    xa = lin.x_approximate
    k, scheme = xa.n_planes, xa.hip_scheme
    forced = xa.eval_scales(m)
    forced = None if forced is None else forced.to(DEV).float().contiguous()
    geom = _hip.make_geom(m, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    words = k * _hip.act_plane_words(geom)
    out = {'M': m, 'F': f, 'O': o, 'x_quant': xq, 'planes': k, 'bytes_x': 2 * m * f}
    variants, equal_planes, equal_out = {}, {}, {}
    for dt, dtype in DTYPES.items():
        x = x32.to(dtype)
        xf = x.float()
        ph, pc = (torch.zeros((words,), dtype=torch.int64, device=DEV) for _ in range(2))
        sh, sc = (torch.empty((k, m), device=DEV) for _ in range(2))

        def forward(half, x=x):
            lin.act_half_kernel = half
            with torch.no_grad():
                return lin(x)

        v = {f'{dt}.quant.half_kernel': lambda x=x, ph=ph, sh=sh: _hip.linear_act_quant_half(x, scheme, k, ALPHA, ph, sh, forced),
             f'{dt}.quant.cast_route': lambda x=x, pc=pc, sc=sc: _hip.act_quant(x.float(), geom, scheme, k, 3, ALPHA, pc, sc, forced),
             f'{dt}.quant.cast_route_without_conversion': lambda xf=xf, pc=pc, sc=sc: _hip.act_quant(xf, geom, scheme, k, 3, ALPHA, pc,
                                                                                                   sc, forced),
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

    chain = 100 if m <= 256 else 10
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
    out['forward_speedup_vs_cast_route'] = {dt: us[f'{dt}.forward.cast_route'] / us[f'{dt}.forward.half_kernel'] for dt in DTYPES}
    out['quant_read_bytes_per_s'] = {dt: out['bytes_x'] / (us[f'{dt}.quant.half_kernel'] * 1e-6) for dt in DTYPES}
    lin.act_half_kernel = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linear_act_quant_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'linear_act_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'clamp_alpha': ALPHA, 'shapes': {}, 'landing': {}}
    for name, m, f, o in SHAPES:
        if only and name not in only:
            continue
        for xq, how in SCHEMES:
            r = res['shapes'].setdefault(name, {})[f'{xq} {how}'] = one_case(m, f, o, xq, args.rounds)
            for dt in DTYPES:
                res['landing'].setdefault(f'{xq} {how}', {}).setdefault(dt, {})[name] = {
                    'forward_speedup_vs_cast_route': r['forward_speedup_vs_cast_route'][dt],
                    'quant_speedup_vs_cast_route': r['quant_speedup_vs_cast_route'][dt],
                    'spread_half_kernel': r['spread'][f'{dt}.forward.half_kernel'],
                    'spread_cast_route': r['spread'][f'{dt}.forward.cast_route']}
            print(name, xq, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res['landing']))


if __name__ == '__main__':
    main()
