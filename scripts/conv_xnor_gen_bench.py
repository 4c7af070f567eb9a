#!/usr/bin/env python3
"""Measurement of the general fp4 matrix-core XNOR convolution (lsq_xnor_conv2d_gen, QuantConv2d.xnor_general), one JSON
document written to --out and printed.

  python scripts/conv_xnor_gen_bench.py [--rounds R] [--only NAMES] [--out profiles/conv_xnor_gen.json]

The graph-replay timing is that of scripts/linear_fp_bench.py.  Per shape at batch 256 (ls-1 weights) and activation scheme
(ls-1: one plane, ls-2: two planes, one launch per call either way): microseconds of `xnor_conv2d_gen` against `xnor_conv2d`
on the same operands -- the popcount kernel for every shape but the yardstick `c128_28_3x3`, which lsq_xnor_conv2d serves on
its tuned fp4 matrix-core kernel.  Every round times (baseline, new, baseline again), so the baseline is sampled twice as
often and in both positions: `baseline_spread` is (max - min) / median over all of its samples.  `verdict` is 'tie' where the
medians differ by less than that spread, else 'faster' / 'slower'.  `fp4_fraction`: binary MACs per second of the new kernel
over half the 9.1 PFLOP/s the fp4 MFMA measured on this part.  `equal`: the two outputs compared bit for bit.
The replays of one graph re-read the same tensors, so up to the 256 MiB Infinity Cache they may come from there rather than
from HBM -- for both routes alike.  QuantConv2d.xnor_general stays False whatever this prints."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402

from linear_fp_bench import DEV, graph_time  # noqa: E402

BATCH = 256
ALPHA = 2.0
FP4_MACS_PER_S = 9.1e15 / 2
# (name, C, O, H = W, kernel, stride, pad, dilation)
SHAPES = [('b256_64_56_1x1', 256, 64, 56, 1, 1, 0, 1), ('b64_256_56_1x1', 64, 256, 56, 1, 1, 0, 1),
          ('b512_128_28_1x1', 512, 128, 28, 1, 1, 0, 1), ('b1024_256_14_1x1', 1024, 256, 14, 1, 1, 0, 1),
          ('b2048_512_7_1x1', 2048, 512, 7, 1, 1, 0, 1), ('b512_2048_7_1x1', 512, 2048, 7, 1, 1, 0, 1),
          ('w320_16_3x3', 320, 320, 16, 3, 1, 1, 1), ('w640_8_3x3', 640, 640, 8, 3, 1, 1, 1),
          ('d256_14_3x3_dil2', 256, 256, 14, 3, 1, 2, 2), ('c128_28_5x5', 128, 128, 28, 5, 1, 2, 1),
          ('c128_28_3x3', 128, 128, 28, 3, 1, 1, 1)]
SCHEMES = {'ls1': 1, 'ls2': 2}


def compare(pairs, rounds, chain=40, reps=7):
    """pairs = {name: (baseline, new)} -> per name the medians, the spreads and the verdict."""
    for base, new in pairs.values():
        graph_time(base, 1, chain)
        graph_time(new, 1, chain)
    res = {}
    for name, (base, new) in pairs.items():
        b, n = [], []
        for _ in range(rounds):
            b.append(graph_time(base, reps, chain))
            n.append(graph_time(new, reps, chain))
            b.append(graph_time(base, reps, chain))
        mb, mn = statistics.median(b), statistics.median(n)
        spread = (max(b) - min(b)) / mb
        verdict = 'tie' if abs(mn - mb) <= spread * mb else ('faster' if mn < mb else 'slower')
        res[name] = {'baseline_us': mb, 'new_us': mn, 'speedup': mb / mn, 'baseline_spread': spread,
                     'new_spread': (max(n) - min(n)) / mn, 'verdict': verdict}
    return res


def one_shape(c, o, hw, kernel, stride, pad, dil, rounds):
    from quant import _hip
    n = BATCH
    geom = _hip.make_geom(n, c, hw, hw, o, kernel, kernel, (stride, stride), (pad, pad), (dil, dil), 1)
    ho, wo = _hip.out_hw(geom)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn((n, c, hw, hw), generator=g) * 1.2).to(DEV)
    w = (torch.randn((o, c, kernel, kernel), generator=g) * 0.05).to(DEV)
    bias = (torch.randn((o,), generator=g) * 0.1).to(DEV)
    wscales = w.reshape(o, -1).abs().mean(dim=1)[None].contiguous()
    wbits, wsum = _hip.pack_weight(w, geom, wscales)
    out = {'N': n, 'C': c, 'O': o, 'H': hw, 'W': hw, 'kernel': kernel, 'stride': stride, 'pad': pad, 'dilation': dil,
           'outputs': n * o * ho * wo, 'equal': {}, 'baseline_kernel': {}}
    pairs, ys = {}, {}
    for name, k in SCHEMES.items():
        planes = torch.zeros((k * _hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
        xs = torch.empty((k, n), device=DEV)
        forced = torch.tensor([0.9 * 0.5 ** q for q in range(k)], device=DEV)[:, None].repeat(1, n).contiguous()
        _hip.act_quant(x, geom, _hip.SCHEME_LS1 if k == 1 else _hip.SCHEME_LS2, k, 3, ALPHA, planes, xs, forced)
        assert _hip.xnor_conv2d_gen_supported(geom, k, 1)
        ys[name] = [torch.empty((n, o, ho, wo), dtype=torch.float32, device=DEV) for _ in range(2)]

        def base(planes=planes, k=k, xs=xs, y=ys[name][0]):
            _hip.xnor_conv2d(planes, k, xs, wbits, wsum, wscales, bias, geom, y)
            return y

        def new(planes=planes, k=k, xs=xs, y=ys[name][1]):
            assert _hip.xnor_conv2d_gen(planes, k, xs, wbits, wsum, wscales, bias, geom, y)
            return y

        pairs[name] = (base, new)
        out['equal'][name] = bool(torch.equal(base(), new()))
        out['baseline_kernel'][name] = 'fp4 (tuned 3x3)' if _hip.xnor_mfma_eligible(geom, k, n * o * ho * wo) else 'popcount'
    out['us'] = compare(pairs, rounds)
    for name, k in SCHEMES.items():
        macs = n * o * ho * wo * c * kernel * kernel * k
        out['us'][name]['fp4_fraction'] = macs / (out['us'][name]['new_us'] * 1e-6) / FP4_MACS_PER_S
        out['us'][name]['new_tmacs_per_s'] = macs / (out['us'][name]['new_us'] * 1e-6) / 1e12
        out['us'][name]['baseline_tmacs_per_s'] = macs / (out['us'][name]['baseline_us'] * 1e-6) / 1e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_xnor_gen.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_xnor_gen_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'batch': BATCH, 'w_quant': 'ls-1',
           'x_quant': 'ls-1 / ls-2 (given scales)', 'shapes': {}, 'summary': {}, 'loses_to_baseline': []}
    for name, c, o, hw, kernel, stride, pad, dil in SHAPES:
        if only and name not in only:
            continue
        r = res['shapes'][name] = one_shape(c, o, hw, kernel, stride, pad, dil, args.rounds)
        for key, t in r['us'].items():
            res['summary'].setdefault(key, {})[name] = {
                'speedup': round(t['speedup'], 3), 'verdict': t['verdict'], 'baseline_spread': round(t['baseline_spread'], 3),
                'fp4_fraction': round(t['fp4_fraction'], 4), 'baseline_kernel': r['baseline_kernel'][key], 'equal': r['equal'][key]}
            if t['verdict'] == 'slower':
                res['loses_to_baseline'].append(f'{name}.{key}')
        print(name, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res['summary']))


if __name__ == '__main__':
    main()
