#!/usr/bin/env python3
"""Measurement of the free-running ls-2 / ls-T quantizer for bf16 / fp16 rows (lsq_linear_act_quant_solve_half) and of
QuantLinear's eval forward on both routes, one JSON document written to --out and printed.

  python scripts/linear_act_solve_half_bench.py [--rounds R] [--out profiles/linear_act_solve_half.json]

The graph-replay timing and the alternating rounds are those of scripts/linear_act_half_bench.py.  Per shape (rows x
features x outputs), activation scheme (ls-2, ls-T; free-running, skip 3) and input type (bf16, fp16), microseconds of
  * `quant.solve_kernel`: lsq_linear_act_quant_solve_half on the 16-bit rows,
  * `quant.cast_route`: x.float() -> lsq_act_quant free-running, and `quant.cast_route_without_conversion`: lsq_act_quant on
    rows that already are fp32,
  * `forward.solve_kernel` / `forward.cast_route`: the whole eval forward of QuantLinear(x_quant, 'ls-1') with
    act_half_solve = True and act_half_kernel True / False (quantizer, lsq_linear_xnor, the cast of the result),
the median of the rounds, with the spread (max - min) / median of each.  `v1_equal` / `planes_equal` / `outputs_equal`: the
two routes' v1, planes and outputs compared bit for bit on the timed inputs (v2 of ls-2 is a sum in a different order).  The
replays of one graph re-read the same rows, so from 67 MB down they may come from the 256 MiB Infinity Cache rather than
from HBM -- for both routes alike.  `landing` collects, per scheme and type, the speedups over the cast route next to the
spreads of both: QuantLinear.act_half_solve becomes True only in a change that has these numbers in hand."""
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
SHAPES = [('lenet_fc1', 64, 800, 500), ('resnet18_head', 256, 512, 1000), ('decode_m1', 1, 4096, 4096),
          ('decode_m16', 16, 4096, 4096), ('mlp', 8192, 4096, 4096)]
SCHEMES = ['ls-2', 'ls-T']


def module(xq, f, o, seed):
    from quant.binary import QuantLinear
    from oracle import ref_port as P
    g = torch.Generator().manual_seed(seed)
    lin = QuantLinear(xq, 'ls-1', f, o, CLAMP)
    with torch.no_grad():
        lin.weight.copy_(torch.randn((o, f), generator=g) * 0.05)
        lin.bias.copy_(torch.randn((o,), generator=g) * 0.1)
        for buf, v in zip(lin.w_approximate.cached_scales(), P.weight_scales(lin.weight.view(o, f, 1, 1), 'ls-1')):
            buf.copy_(v)
    lin.act_half_solve = True
    assert lin.act_skip == SKIP
    return lin.eval().to(DEV)


def one_case(m, f, o, xq, rounds):
    from quant import _hip
    x32 = (torch.randn((m, f), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV)
    lin = module(xq, f, o, seed=2)
    scheme = lin.x_approximate.hip_scheme
    geom = _hip.make_geom(m, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    words = 2 * _hip.act_plane_words(geom)
    out = {'M': m, 'F': f, 'O': o, 'x_quant': xq, 'skip': SKIP, 'bytes_x': 2 * m * f}
    variants, equal_v1, equal_planes, equal_out = {}, {}, {}, {}
    for dt, dtype in DTYPES.items():
        x = x32.to(dtype)
        xf = x.float()
        ph, pc = (torch.zeros((words,), dtype=torch.int64, device=DEV) for _ in range(2))
        sh, sc = (torch.empty((2, m), device=DEV) for _ in range(2))

        def forward(half, x=x):
            lin.act_half_kernel = half
            with torch.no_grad():
                return lin(x)

        v = {f'{dt}.quant.solve_kernel': lambda x=x, ph=ph, sh=sh: _hip.linear_act_quant_solve_half(x, scheme, SKIP, ALPHA, ph, sh),
             f'{dt}.quant.cast_route': lambda x=x, pc=pc, sc=sc: _hip.act_quant(x.float(), geom, scheme, 2, SKIP, ALPHA, pc, sc),
             f'{dt}.quant.cast_route_without_conversion': lambda xf=xf, pc=pc, sc=sc: _hip.act_quant(xf, geom, scheme, 2, SKIP, ALPHA,
                                                                                                   pc, sc),
             f'{dt}.forward.solve_kernel': lambda forward=forward: forward(True),
             f'{dt}.forward.cast_route': lambda forward=forward: forward(False)}
        v[f'{dt}.quant.solve_kernel']()
        v[f'{dt}.quant.cast_route']()
        yh, yc = v[f'{dt}.forward.solve_kernel'](), v[f'{dt}.forward.cast_route']()
        torch.cuda.synchronize()
        equal_v1[dt] = bool(torch.equal(sh[0].view(torch.int32), sc[0].view(torch.int32)))
        equal_planes[dt] = bool(torch.equal(ph, pc))
        equal_out[dt] = bool(torch.equal(yh.view(torch.int16), yc.view(torch.int16)))
        variants.update(v)
    out['v1_equal'], out['planes_equal'], out['outputs_equal'] = equal_v1, equal_planes, equal_out

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
    out['quant_speedup_vs_cast_route'] = {dt: us[f'{dt}.quant.cast_route'] / us[f'{dt}.quant.solve_kernel'] for dt in DTYPES}
    out['forward_speedup_vs_cast_route'] = {dt: us[f'{dt}.forward.cast_route'] / us[f'{dt}.forward.solve_kernel'] for dt in DTYPES}
    lin.act_half_kernel = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linear_act_solve_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'linear_act_solve_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'clamp_alpha': ALPHA, 'skip': SKIP, 'shapes': {},
           'landing': {}}
    for name, m, f, o in SHAPES:
        if only and name not in only:
            continue
        for xq in SCHEMES:
            r = res['shapes'].setdefault(name, {})[xq] = one_case(m, f, o, xq, args.rounds)
            for dt in DTYPES:
                res['landing'].setdefault(xq, {}).setdefault(dt, {})[name] = {
                    'forward_speedup_vs_cast_route': r['forward_speedup_vs_cast_route'][dt],
                    'quant_speedup_vs_cast_route': r['quant_speedup_vs_cast_route'][dt],
                    'spread_solve_kernel': r['spread'][f'{dt}.forward.solve_kernel'],
                    'spread_cast_route': r['spread'][f'{dt}.forward.cast_route']}
            print(name, xq, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res['landing']))


if __name__ == '__main__':
    main()
