#!/usr/bin/env python3
"""Measurement of the given-scale next quantizer in the XNOR convolution's epilogue (lsq_xnor_conv2d_chain_fixed,
quant.binary.chain.FIXED_SCALES), one JSON document written to --out and printed.

  python scripts/chain_fixed_bench.py [--rounds R] [--only layers,net] [--batches 1,8,32,256] [--out profiles/chain_fixed.json]

  * `layers`: per 3 x 3 layer shape of ResNet-18 at batch 256 (ls-1 weights, ls-2 activations with given scales on both sides,
    PReLU and a residual in the epilogue as inside the network), microseconds of ONE `xnor_conv2d_chain_fixed` against
    `xnor_conv2d` followed by `act_quant(forced)` on its output -- what the layer pair costs with the switch off.  Calls are
    captured 40 to a graph (scripts/linear_fp_bench.py) and walk over `sets` copies of every buffer they touch, sized so that a
    copy is read again only after more than twice the 256 MiB Infinity Cache has gone by.
  * `net`: the headline network with moving-average activation scales (bench.py's `imagenet_ls1w_ls2a_moving_average` leg) at
    each batch size, eager (host included) and as one graph replay (quant/common/graph_replay.py), switch on against off.
Every round times (baseline, new, baseline again): `baseline_spread` is (max - min) / median over the baseline's samples, and
`verdict` is 'tie' where the medians differ by less than it.  `equal`: the outputs of the two routes compared bit for bit on the
timed inputs.  chain.FIXED_SCALES stays False whatever this prints."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402

from conv_xnor_half_bench import SHAPES, module  # noqa: E402
from linear_fp_bench import DEV, graph_time  # noqa: E402

BATCH = 256
CACHE = 256 << 20


def sample(base, new, rounds, timer):
    b, n = [], []
    for _ in range(rounds):
        b.append(timer(base))
        n.append(timer(new))
        b.append(timer(base))
    mb, mn = statistics.median(b), statistics.median(n)
    spread = (max(b) - min(b)) / mb
    verdict = 'tie' if abs(mn - mb) <= spread * mb else ('faster' if mn < mb else 'slower')
    return {'baseline_us': mb, 'new_us': mn, 'speedup': mb / mn, 'baseline_spread': spread, 'new_spread': (max(n) - min(n)) / mn,
            'verdict': verdict}


def one_layer(c, hw, o, stride, rounds, chain=40, reps=7):
    from quant import _hip
    n = BATCH
    conv = module(c, o, stride, seed=2)
    geom = _hip.make_geom(n, c, hw, hw, o, 3, 3, (stride, stride), (1, 1), (1, 1), 1)
    ho, wo = _hip.out_hw(geom)
    g2 = _hip.make_geom(n, o, ho, wo, o, 3, 3, (1, 1), (1, 1), (1, 1), 1)                 # the consumer: 3 x 3, pad 1
    k = 2
    forced = conv.x_approximate.eval_scales(n).to(device=DEV, dtype=torch.float32).contiguous()
    wbits, wsum, wscales, _ = conv._packed_weights(geom, _hip)
    bias, slope = conv.bias.detach(), torch.full((1,), 0.25, device=DEV)
    pre = (torch.rand((o,), device=DEV) + 0.5, torch.randn((o,), device=DEV) * 0.1)        # the consumer's folded batch norm
    words_in, words_out = _hip.act_plane_words(geom), _hip.act_plane_words(g2)
    per_set = 8 * k * (words_in + words_out) + 4 * 2 * n * o * ho * wo                      # planes in and out, y, residual
    nsets = max(2, min(64, -(-2 * CACHE // per_set) + 1))
    sets = []
    for i in range(nsets):
        x = (torch.randn((n, c, hw, hw), generator=torch.Generator().manual_seed(i)) * 1.2).to(DEV)
        planes = torch.zeros((k * words_in,), dtype=torch.int64, device=DEV)
        xs = torch.empty((k, n), device=DEV)
        _hip.act_quant(x, geom, _hip.SCHEME_LS2, k, 3, 2.0, planes, xs, forced)
        del x
        sets.append({'planes': planes, 'xs': xs, 'res': torch.randn((n, o, ho, wo), device=DEV),
                     'y': torch.empty((n, o, ho, wo), device=DEV),
                     'next': torch.zeros((k * words_out,), dtype=torch.int64, device=DEV), 'scales': torch.empty((k, n), device=DEV)})
    turn = [0]

    def pick():
        turn[0] += 1
        return sets[turn[0] % nsets]

    def base():
        s = pick()
        _hip.xnor_conv2d(s['planes'], k, s['xs'], wbits, wsum, wscales, bias, geom, s['y'], False, s['res'], None, slope)
        _hip.act_quant(s['y'], g2, _hip.SCHEME_LS2, k, 3, 2.0, s['next'], s['scales'], forced, pre)
        return s

    def new():
        s = pick()
        nxt = _hip.NextFixed(s['next'].data_ptr(), k, forced.data_ptr(), pre[0].data_ptr(), pre[1].data_ptr(), 2.0, 1, 1)
        assert _hip.xnor_conv2d_chain_fixed(s['planes'], k, s['xs'], wbits, wsum, wscales, bias, geom, s['y'], nxt, False, s['res'],
                                            None, slope)
        return s

    turn[0] = 0
    a = base()
    ya, pa = a['y'].clone(), a['next'].clone()
    turn[0] = 0
    b = new()
    out = {'N': n, 'C': c, 'H': hw, 'O': o, 'stride': stride, 'sets': nsets, 'bytes_per_set': per_set, 'graph_chain': chain,
           'equal': bool(torch.equal(ya, b['y']) and torch.equal(pa, b['next']))}
    del ya, pa
    out['us'] = sample(base, new, rounds, lambda fn: graph_time(fn, reps, chain))
    return out


def network(batch, rounds):
    import bench
    from quant.binary import chain
    from quant.common.graph_replay import GraphedForward
    arch = bench.imagenet_arch('ls-2', 3)
    arch.update(moving_average_mode='eval_only', moving_average_momentum=0.0)
    model = bench.build_model(arch, DEV)
    x = torch.randn((max(batch, 4), 3, 224, 224), generator=torch.Generator().manual_seed(0)).to(DEV)
    model.train()
    with torch.no_grad():
        model(x[:4])                                  # one calibration step: the scale buffers take the batch's values
    model.eval()
    x = x[:batch].contiguous()

    def forward(on):
        chain.FIXED_SCALES = on
        with torch.no_grad():
            return model(x)

    steps = 20 if batch >= 32 else 50

    def eager(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / steps)
        return statistics.median(ts)

    out = {'batch': batch, 'equal': bool(torch.equal(forward(False), forward(True)))}
    out['eager_us'] = sample(lambda: forward(False), lambda: forward(True), rounds, eager)
    graphs = {}
    for on in (False, True):
        chain.FIXED_SCALES = on
        graphs[on] = GraphedForward(model, x)
    chain.FIXED_SCALES = False
    out['graph_equal'] = bool(torch.equal(graphs[False].replay(), graphs[True].replay()))
    out['graph_us'] = sample(graphs[False].replay, graphs[True].replay, rounds, eager)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='layers,net')
    ap.add_argument('--batches', default='1,8,32,256')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'chain_fixed.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'chain_fixed_bench.py measures on the GPU'
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'layers': {}, 'net': {}}
    if 'layers' in args.only:
        for name, c, hw, o, stride in SHAPES:
            res['layers'][name] = one_layer(c, hw, o, stride, args.rounds)
            print(name, json.dumps(res['layers'][name]), flush=True)
            torch.cuda.empty_cache()
    if 'net' in args.only:
        for batch in map(int, args.batches.split(',')):
            res['net'][f'b{batch}'] = network(batch, args.rounds)
            print(f'b{batch}', json.dumps(res['net'][f'b{batch}']), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
