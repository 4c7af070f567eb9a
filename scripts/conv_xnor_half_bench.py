#!/usr/bin/env python3
"""Measurement of the XNOR convolution with a 16-bit epilogue (lsq_xnor_conv2d_half, QuantConv2d.xnor_half), one JSON document
written to --out and printed.

  python scripts/conv_xnor_half_bench.py [--rounds R] [--only NAMES] [--out profiles/conv_xnor_half.json]

The graph-replay timing is that of scripts/linear_fp_bench.py.  Per 3 x 3 layer shape of ResNet-18 at batch 256 (ls-1 weights,
ls-2 activations with given scales: one launch per call) and output type (bf16, fp16):
  * `conv`: microseconds of `xnor_conv2d_half` against `xnor_conv2d` into an fp32 y followed by `.to(dtype)`, what
    QuantConv2d does with the switch off, on the same planes;
  * `block`: microseconds of `fused_forward(x16, relu=True, res_pre=r16)` with xnor_half on (quantizer + one launch) against the
    switch off (quantizer, lsq_xnor_conv2d, `.to()`, `+`, `relu`: the composition in torch), same module, same input;
  * `peak_bytes`: torch.cuda.max_memory_allocated over one call of each, above what was allocated before it.
Every round times (baseline, new, baseline again), so the baseline is sampled twice as often and in both positions:
`baseline_spread` is (max - min) / median over all of its samples -- its own run-to-run spread.  `verdict` is 'tie' where the
medians differ by less than that spread, else 'faster' / 'slower'.  `equal`: the outputs of the two routes compared bit for bit
on the timed inputs.  The replays of one graph re-read the same tensors, so up to the 256 MiB Infinity Cache they may come from
there rather than from HBM -- for both routes alike.  QuantConv2d.xnor_half stays False whatever this prints."""
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
BATCH = 256
# (name, C, H = W, O, stride): every distinct 3 x 3 quantized layer of ResNet-18 (quant/models/resnet.py)
SHAPES = [('c64_56', 64, 56, 64, 1), ('c64_56_s2', 64, 56, 128, 2), ('c128_28', 128, 28, 128, 1), ('c128_28_s2', 128, 28, 256, 2),
          ('c256_14', 256, 14, 256, 1), ('c256_14_s2', 256, 14, 512, 2), ('c512_7', 512, 7, 512, 1)]


def module(c, o, stride, seed):
    from quant.binary.binary_conv import QuantConv2d
    from oracle import ref_port as P
    g = torch.Generator().manual_seed(seed)
    conv = QuantConv2d('ls-2', 'ls-1', c, o, 3, CLAMP, padding=1, stride=stride, moving_average_mode='eval_only')
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.05)
        conv.bias.copy_(torch.randn((o,), generator=g) * 0.1)
        for buf, v in zip(conv.w_approximate.cached_scales(), P.weight_scales(conv.weight, 'ls-1')):
            buf.copy_(v)
        avg = conv.x_approximate.moving_avg_module.moving_average
        avg.copy_(torch.tensor([0.9 * 0.5 ** q for q in range(avg.numel())]).view_as(avg))
    conv.act_half = True
    return conv.eval().to(DEV)


def peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    top = torch.cuda.max_memory_allocated() - base
    del out
    return top


def compare(pairs, rounds, chain=40, reps=7):
    """pairs = {name: (baseline, new)} -> per name the medians, the baseline's spread and the verdict."""
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
    return res, chain


def one_shape(c, hw, o, stride, rounds):
    from quant import _hip
    n = BATCH
    conv = module(c, o, stride, seed=2)
    geom = _hip.make_geom(n, c, hw, hw, o, 3, 3, (stride, stride), (1, 1), (1, 1), 1)
    ho, wo = _hip.out_hw(geom)
    x32 = (torch.randn((n, c, hw, hw), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV)
    r32 = torch.randn((n, o, ho, wo), generator=torch.Generator().manual_seed(3)).to(DEV)
    k = conv.x_approximate.n_planes
    forced = conv.x_approximate.eval_scales(n).to(device=DEV, dtype=torch.float32).contiguous()
    planes = torch.zeros((k * _hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xs = torch.empty((k, n), device=DEV)
    _hip.act_quant(x32, geom, conv.x_approximate.hip_scheme, k, 3, 2.0, planes, xs, forced)
    wbits, wsum, wscales, _ = conv._packed_weights(geom, _hip)
    bias = conv.bias.detach()
    shape = (n, o, ho, wo)
    out = {'N': n, 'C': c, 'H': hw, 'W': hw, 'O': o, 'stride': stride, 'outputs': n * o * ho * wo, 'equal': {}, 'peak_bytes': {}}
    pairs = {}
    for dt, dtype in DTYPES.items():
        x, res = x32.to(dtype), r32.to(dtype)

        def conv_base(dtype=dtype):      # (the fp32 y allocated per call, as QuantConv2d does)
            y32 = torch.empty(shape, dtype=torch.float32, device=DEV)
            _hip.xnor_conv2d(planes, k, xs, wbits, wsum, wscales, bias, geom, y32)
            return y32.to(dtype)

        def conv_new(dtype=dtype):
            return _hip.xnor_conv2d_half(planes, k, xs, wbits, wsum, wscales, bias, geom, dtype)

        def block(on, x=x, res=res):
            conv.xnor_half = on
            with torch.no_grad():
                return conv.fused_forward(x, relu=True, res_pre=res)

        block_base, block_new = (lambda block=block: block(False)), (lambda block=block: block(True))
        pairs[f'{dt}.conv'] = (conv_base, conv_new)
        pairs[f'{dt}.block'] = (block_base, block_new)
        out['equal'][f'{dt}.conv'] = bool(torch.equal(conv_base().view(torch.int16), conv_new().view(torch.int16)))
        # (the block's composition rounds after the convolution, after the add and after the ReLU; the fused launch rounds once)
        a, b = block_base(), block_new()
        out['equal'][f'{dt}.block'] = bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))
        out[f'{dt}.block_outputs_that_differ'] = int((a.view(torch.int16) != b.view(torch.int16)).sum())
        del a, b
        for name, (base, new) in ((f'{dt}.conv', pairs[f'{dt}.conv']), (f'{dt}.block', pairs[f'{dt}.block'])):
            out['peak_bytes'][name] = {'baseline': peak(base), 'new': peak(new)}
    out['us'], out['graph_chain'] = compare(pairs, rounds)
    conv.xnor_half = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_xnor_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_xnor_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'batch': BATCH, 'x_quant': 'ls-2 (given scales)',
           'w_quant': 'ls-1', 'shapes': {}, 'summary': {}}
    for name, c, hw, o, stride in SHAPES:
        if only and name not in only:
            continue
        r = res['shapes'][name] = one_shape(c, hw, o, stride, args.rounds)
        for key, t in r['us'].items():
            res['summary'].setdefault(key, {})[name] = {
                'speedup': round(t['speedup'], 3), 'verdict': t['verdict'], 'baseline_spread': round(t['baseline_spread'], 3),
                'peak_ratio': round(r['peak_bytes'][key]['new'] / max(1, r['peak_bytes'][key]['baseline']), 3)}
        print(name, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res['summary']))


if __name__ == '__main__':
    main()
