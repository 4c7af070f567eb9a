#!/usr/bin/env python3
"""Measurement of the general fp4 matrix-core XNOR convolution with a 16-bit epilogue and the plane passes in the kernel
(lsq_xnor_conv2d_gen_half, QuantConv2d.xnor_general_half), one JSON document written to --out and printed.

  python scripts/conv_xnor_gen_half_bench.py [--rounds R] [--only NAMES] [--dtype bf16] [--out profiles/conv_xnor_gen_half.json]

The graph-replay timing is that of scripts/linear_fp_bench.py (graphs of 40 calls).  Per shape of DESIGN 4.36's table at batch
256 and plane counts (kx, kw) = (1, 1), (2, 1) -- one pass -- and (2, 2) -- two passes: microseconds of `xnor_conv2d_gen_half`
against, on the same operands,
  (a) `xnor_conv2d_half`, today's route of a 16-bit network: the popcount kernel with a 16-bit epilogue, one launch per pass and
      an fp32 running sum in a workspace between them;
  (b) `xnor_conv2d_gen` into an fp32 y followed by `.to(dtype)`.
Every shape is warmed first; every round times (a, new, b, a), so (a) is sampled twice as often and in both positions:
`a_spread` is (max - min) / median over all of its samples, `b_spread` and `new_spread` likewise.  `verdict_vs_a` is 'tie' where
the medians differ by less than (a)'s spread, else 'faster' / 'slower'.  `equal`: the three outputs compared bit for bit at the
timed sizes.  The replays of one graph re-read the same tensors, so up to the 256 MiB Infinity Cache they may come from there
rather than from HBM -- for every route alike.  QuantConv2d.xnor_general_half stays False whatever this prints."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402

from conv_xnor_gen_bench import ALPHA, BATCH, SHAPES  # noqa: E402
from linear_fp_bench import DEV, graph_time  # noqa: E402

PLANES = {'kx1_kw1': (1, 1), 'kx2_kw1': (2, 1), 'kx2_kw2': (2, 2)}
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}


def compare(routes, rounds, chain=40, reps=7):
    """routes = {name: (a, b, new)} -> per name the medians, the spreads and the verdict against (a)."""
    for fns in routes.values():
        for fn in fns:
            graph_time(fn, 1, chain)
    res = {}
    for name, (a, b, new) in routes.items():
        ta, tb, tn = [], [], []
        for _ in range(rounds):
            ta.append(graph_time(a, reps, chain))
            tn.append(graph_time(new, reps, chain))
            tb.append(graph_time(b, reps, chain))
            ta.append(graph_time(a, reps, chain))
        ma, mb, mn = statistics.median(ta), statistics.median(tb), statistics.median(tn)
        spread = (max(ta) - min(ta)) / ma
        verdict = 'tie' if abs(mn - ma) <= spread * ma else ('faster' if mn < ma else 'slower')
        res[name] = {'a_us': ma, 'b_us': mb, 'new_us': mn, 'speedup_vs_a': ma / mn, 'speedup_vs_b': mb / mn, 'a_spread': spread,
                     'b_spread': (max(tb) - min(tb)) / mb, 'new_spread': (max(tn) - min(tn)) / mn, 'verdict_vs_a': verdict}
    return res


def one_shape(c, o, hw, kernel, stride, pad, dil, rounds, dtype):
    from quant import _hip
    n = BATCH
    geom = _hip.make_geom(n, c, hw, hw, o, kernel, kernel, (stride, stride), (pad, pad), (dil, dil), 1)
    ho, wo = _hip.out_hw(geom)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn((n, c, hw, hw), generator=g) * 1.2).to(DEV)
    w = (torch.randn((o, c, kernel, kernel), generator=g) * 0.05).to(DEV)
    bias = (torch.randn((o,), generator=g) * 0.1).to(DEV)
    out = {'N': n, 'C': c, 'O': o, 'H': hw, 'W': hw, 'kernel': kernel, 'stride': stride, 'pad': pad, 'dilation': dil,
           'outputs': n * o * ho * wo, 'equal': {}, 'a_kernel': {}}
    routes = {}
    y32 = torch.empty((n, o, ho, wo), dtype=torch.float32, device=DEV)
    for name, (k, kw) in PLANES.items():
        res, rows = w.reshape(o, -1).clone(), []
        for _ in range(kw):                          # the greedy chain of weight scales
            rows.append(res.abs().mean(dim=1))
            res = res - rows[-1][:, None] * torch.where(res >= 0, 1.0, -1.0)
        wscales = torch.stack(rows).contiguous()
        wbits, wsum = _hip.pack_weight(w, geom, wscales)
        planes = torch.zeros((k * _hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
        xs = torch.empty((k, n), device=DEV)
        forced = torch.tensor([0.9 * 0.5 ** q for q in range(k)], device=DEV)[:, None].repeat(1, n).contiguous()
        _hip.act_quant(x, geom, _hip.SCHEME_LS1 if k == 1 else _hip.SCHEME_LS2, k, 3, ALPHA, planes, xs, forced)
        assert _hip.xnor_conv2d_gen_half_supported(geom, k, kw, dtype)
        ops = (planes, k, xs, wbits, wsum, wscales, bias, geom)

        def a(ops=ops):
            return _hip.xnor_conv2d_half(*ops, dtype)

        def b(ops=ops):
            assert _hip.xnor_conv2d_gen(*ops, y32)
            return y32.to(dtype)

        def new(ops=ops):
            return _hip.xnor_conv2d_gen_half(*ops, dtype)

        routes[name] = (a, b, new)
        ya = a()
        out['equal'][name] = bool(torch.equal(ya, new())) and bool(torch.equal(ya, b()))
        out['a_kernel'][name] = 'fp4 (tuned 3x3)' if _hip.xnor_mfma_eligible(geom, k, n * o * ho * wo) else 'popcount'
        del ya
    out['us'] = compare(routes, rounds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: the ten of DESIGN 4.36 without its yardstick)')
    ap.add_argument('--dtype', default='bf16', choices=list(DTYPES))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_xnor_gen_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_xnor_gen_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'batch': BATCH, 'dtype': args.dtype,
           'x_quant': 'ls-1 / ls-2 (given scales)', 'w_quant': 'ls-1 / ls-2 (greedy scales)', 'shapes': {}, 'summary': {},
           'loses_to_a': [], 'not_measured': ['fp16 timings' if args.dtype == 'bf16' else 'bf16 timings',
                                              'batch sizes other than 256', 'a whole network under autocast']}
    for name, c, o, hw, kernel, stride, pad, dil in SHAPES:
        if (only and name not in only) or (not only and name == 'c128_28_3x3'):      # (the yardstick is the tuned kernel's shape)
            continue
        r = res['shapes'][name] = one_shape(c, o, hw, kernel, stride, pad, dil, args.rounds, DTYPES[args.dtype])
        for key, t in r['us'].items():
            res['summary'].setdefault(key, {})[name] = {
                'vs_a': round(t['speedup_vs_a'], 3), 'vs_b': round(t['speedup_vs_b'], 3), 'verdict_vs_a': t['verdict_vs_a'],
                'a_spread': round(t['a_spread'], 3), 'b_spread': round(t['b_spread'], 3), 'a_kernel': r['a_kernel'][key],
                'equal': r['equal'][key]}
            if t['verdict_vs_a'] == 'slower':
                res['loses_to_a'].append(f'{name}.{key}')
        print(name, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res['summary']))


if __name__ == '__main__':
    main()
