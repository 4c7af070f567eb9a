#!/usr/bin/env python3
"""Measurement of the fp4 matrix-core XNOR convolution for any channel count (lsq_xnor_conv2d_narrow,
QuantConv2d.xnor_narrow), one JSON document written to --out and printed.

  python scripts/conv_xnor_narrow_bench.py [--rounds R] [--only NAMES] [--out profiles/conv_xnor_narrow.json]

Timing and verdicts are those of scripts/conv_xnor_gen_bench.py (graph replays; every round times baseline, new, baseline;
'tie' inside the baseline's spread).  Per shape (ls-2 activations with given scales, ls-1 weights): microseconds of
`xnor_conv2d_narrow` against `xnor_conv2d` on the same operands -- the popcount kernel for every shape here -- and, for the
pooled rows, `xnor_conv2d_narrow(pool=2)` with ReLU against `xnor_conv2d` with ReLU followed by F.max_pool2d.  `equal`: the
two outputs compared bit for bit.  `lenet`: microseconds per graph replay of QLeNet5's eval forward at batch 64 with
QuantConv2d.xnor_narrow off and on.  The switch stays False whatever this prints."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from conv_xnor_gen_bench import compare  # noqa: E402
from linear_fp_bench import DEV  # noqa: E402

ALPHA = 2.0
# (name, N, C, O, H = W, kernel, stride, pad, pool)
SHAPES = [('lenet_conv2_b64', 64, 20, 50, 12, 5, 1, 0, 2), ('lenet_conv2_b256', 256, 20, 50, 12, 5, 1, 0, 2),
          ('c32_32_3x3_b100', 100, 32, 32, 32, 3, 1, 1, 1), ('c96_28_3x3_b256', 256, 96, 96, 28, 3, 1, 1, 1),
          ('c160_14_3x3_b256', 256, 160, 160, 14, 3, 1, 1, 1), ('c96_192_28_1x1_s2_b256', 256, 96, 192, 28, 1, 2, 0, 1)]


def one_shape(n, c, o, hw, kernel, stride, pad, pool, rounds):
    from quant import _hip
    k = 2
    geom = _hip.make_geom(n, c, hw, hw, o, kernel, kernel, (stride, stride), (pad, pad), (1, 1), 1)
    ho, wo = _hip.out_hw(geom)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn((n, c, hw, hw), generator=g) * 1.2).to(DEV)
    w = (torch.randn((o, c, kernel, kernel), generator=g) * 0.05).to(DEV)
    bias = (torch.randn((o,), generator=g) * 0.1).to(DEV)
    wscales = w.reshape(o, -1).abs().mean(dim=1)[None].contiguous()
    wbits, wsum = _hip.pack_weight(w, geom, wscales)
    planes = torch.zeros((k * _hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xs = torch.empty((k, n), device=DEV)
    forced = torch.tensor([0.9 * 0.5 ** q for q in range(k)], device=DEV)[:, None].repeat(1, n).contiguous()
    _hip.act_quant(x, geom, _hip.SCHEME_LS2, k, 3, ALPHA, planes, xs, forced)
    assert _hip.xnor_conv2d_narrow_supported(geom, k, 1, pool)
    relu = pool == 2
    y_full = torch.empty((n, o, ho, wo), dtype=torch.float32, device=DEV)
    y_new = torch.empty((n, o, ho // pool, wo // pool), dtype=torch.float32, device=DEV)

    def base():
        _hip.xnor_conv2d(planes, k, xs, wbits, wsum, wscales, bias, geom, y_full, relu=relu)
        return F.max_pool2d(y_full, 2, 2) if pool == 2 else y_full

    def new():
        assert _hip.xnor_conv2d_narrow(planes, k, xs, wbits, wsum, wscales, bias, geom, y_new, relu=relu, pool=pool)
        return y_new

    out = {'N': n, 'C': c, 'O': o, 'H': hw, 'W': hw, 'kernel': kernel, 'stride': stride, 'pad': pad, 'pool': pool,
           'outputs': n * o * ho * wo, 'equal': bool(torch.equal(base(), new()))}
    out['us'] = compare({'ls2': (base, new)}, rounds)['ls2']
    macs = n * o * ho * wo * c * kernel * kernel * k
    out['us']['new_tmacs_per_s'] = macs / (out['us']['new_us'] * 1e-6) / 1e12
    out['us']['baseline_tmacs_per_s'] = macs / (out['us']['baseline_us'] * 1e-6) / 1e12
    return out


def lenet(rounds):
    """QLeNet5 eval forward at batch 64 per graph replay, QuantConv2d.xnor_narrow off (baseline) and on."""
    from quant.binary.binary_conv import QuantConv2d
    from quant.models.lenet import QLeNet5
    torch.manual_seed(2)
    net = QLeNet5(loss_fn=None, x_quant='ls-2', w_quant='ls-1', clamp={'kind': 'symmetric', 'alpha': ALPHA})
    with torch.no_grad():
        net.conv2.w_approximate.v1.copy_(net.conv2.weight.abs().mean(dim=(1, 2, 3)))
    net.eval().to(DEV)
    x = torch.randn((64, 1, 28, 28), generator=torch.Generator().manual_seed(3)).to(DEV)

    def run(on):
        def fn():
            QuantConv2d.xnor_narrow = on
            try:
                with torch.no_grad():
                    return net(x)
            finally:
                QuantConv2d.xnor_narrow = False
        return fn

    off, on = run(False), run(True)
    res = compare({'lenet_b64': (off, on)}, rounds, chain=10)['lenet_b64']
    res['equal'] = bool(torch.equal(off(), on()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names, "lenet" for the network (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_xnor_narrow.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_xnor_narrow_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'w_quant': 'ls-1', 'x_quant': 'ls-2 (given scales)',
           'shapes': {}, 'summary': {}, 'loses_to_baseline': []}
    for name, n, c, o, hw, kernel, stride, pad, pool in SHAPES:
        if only and name not in only:
            continue
        r = res['shapes'][name] = one_shape(n, c, o, hw, kernel, stride, pad, pool, args.rounds)
        t = r['us']
        res['summary'][name] = {'speedup': round(t['speedup'], 3), 'verdict': t['verdict'], 'equal': r['equal'],
                                'baseline_spread': round(t['baseline_spread'], 3)}
        if t['verdict'] == 'slower':
            res['loses_to_baseline'].append(name)
        print(name, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    def dump():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write('\n')

    dump()                               # (the per-call rows are kept whatever becomes of the network's graph)
    if not only or 'lenet' in only:
        res['lenet'] = lenet(args.rounds)
        print('lenet', json.dumps(res['lenet']), flush=True)
        if res['lenet']['verdict'] == 'slower':
            res['loses_to_baseline'].append('lenet')
        dump()
    print(json.dumps(res['summary']))


if __name__ == '__main__':
    main()
