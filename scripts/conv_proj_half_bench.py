#!/usr/bin/env python3
"""Measurement of the projection shortcut on 16-bit tensors (lsq_pointwise_conv_half, lsq_xnor_conv2d_proj_half;
quant.models.resnet.PROJ_HALF), one JSON document written to --out and printed.

  python scripts/conv_proj_half_bench.py [--rounds R] [--only NAMES] [--out profiles/conv_proj_half.json]

The graph-replay timing is that of scripts/linear_fp_bench.py, the comparison loop that of scripts/conv_xnor_half_bench.py: every
round times (baseline, new, baseline again), `baseline_spread` is (max - min) / median over all baseline samples, `verdict` is
'tie' where the medians differ by less than that spread.  Per projection shape of ResNet-18 at batch 256 (the three down-sampling
blocks, double shortcut: the consumer is the block's stride-2 3 x 3 convolution, ls-2 activations with given scales against ls-1
weights, ReLU, the projection as res_post) and type (bf16, fp16), each new call against the route the parent offers:
  * `pointwise`: `pointwise_conv_half(x16)` against `pointwise_conv(x16.float()).to(dtype)`;
  * `fused`: `xnor_conv2d_proj_half` against `xnor_conv2d_proj` on the widened operands into an fp32 y, `.to(dtype)`;
  * `fused_vs_pair`: `xnor_conv2d_proj_half` against the unfused 16-bit pair `pointwise_conv_half` + `xnor_conv2d_half` (baseline
    = the pair), the comparison `proj_fused_wins` was measured for in fp32 (profiles/proj_fused.json); `gate_agrees` records
    whether the 16-bit verdict is the gate's answer for the shape.
`equal`: the two routes' outputs compared bit for bit (for `fused_vs_pair` they are NOT expected to be equal: the pair rounds the
shortcut first; the count of differing outputs is recorded).  The replays of one graph re-read the same tensors, so up to the
256 MiB Infinity Cache they may come from there rather than from HBM -- for both routes alike.  resnet.PROJ_HALF stays False
whatever this prints."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402

from conv_xnor_half_bench import compare, module, peak  # noqa: E402
from linear_fp_bench import DEV  # noqa: E402

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
BATCH = 256
# (name, Cp = consumer C, H = W of the block's input, O): the three projection shortcuts of ResNet-18, stride 2
SHAPES = [('p64_56', 64, 56, 128), ('p128_28', 128, 28, 256), ('p256_14', 256, 14, 512)]


def one_shape(c, hw, o, rounds):
    from quant import _hip
    n = BATCH
    conv = module(c, o, 2, seed=2)
    geom = _hip.make_geom(n, c, hw, hw, o, 3, 3, (2, 2), (1, 1), (1, 1), 1)
    ho, wo = _hip.out_hw(geom)
    x32 = (torch.randn((n, c, hw, hw), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV)
    g = torch.Generator().manual_seed(5)
    pw = (torch.randn((o, c), generator=g) * c ** -0.5).to(DEV)
    pb = (torch.randn((o,), generator=g) * 0.3).to(DEV)
    k = conv.x_approximate.n_planes
    forced = conv.x_approximate.eval_scales(n).to(device=DEV, dtype=torch.float32).contiguous()
    planes = torch.zeros((k * _hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xs = torch.empty((k, n), device=DEV)
    _hip.act_quant(x32, geom, conv.x_approximate.hip_scheme, k, 3, 2.0, planes, xs, forced)
    wbits, wsum, wscales, _ = conv._packed_weights(geom, _hip)
    bias = conv.bias.detach()
    shape = (n, o, ho, wo)
    out = {'N': n, 'Cp': c, 'H': hw, 'W': hw, 'O': o, 'stride': 2, 'outputs': n * o * ho * wo, 'equal': {}, 'peak_bytes': {},
           'gate': bool(_hip.proj_fused_wins(c, o))}
    pairs = {}
    for dt, dtype in DTYPES.items():
        x16 = x32.to(dtype)

        def pw_base(x16=x16, dtype=dtype):
            return _hip.pointwise_conv(x16.float(), pw, pb, 2).to(dtype)

        def pw_new(x16=x16):
            return _hip.pointwise_conv_half(x16, pw, pb, 2)

        def fused_base(x16=x16, dtype=dtype):
            y32 = torch.empty(shape, dtype=torch.float32, device=DEV)
            assert _hip.xnor_conv2d_proj(planes, k, xs, wbits, wsum, wscales, bias, geom, y32, (x16.float(), pw, pb, 2, True), relu=True)
            return y32.to(dtype)

        def fused_new(x16=x16, dtype=dtype):
            took, y = _hip.xnor_conv2d_proj_half(planes, k, xs, wbits, wsum, wscales, bias, geom, (x16, pw, pb, 2, True), dtype,
                                                 relu=True)
            assert took
            return y

        def pair(x16=x16, dtype=dtype):
            sc = _hip.pointwise_conv_half(x16, pw, pb, 2)
            return _hip.xnor_conv2d_half(planes, k, xs, wbits, wsum, wscales, bias, geom, dtype, relu=True, res_post=sc)

        pairs[f'{dt}.pointwise'] = (pw_base, pw_new)
        pairs[f'{dt}.fused'] = (fused_base, fused_new)
        pairs[f'{dt}.fused_vs_pair'] = (pair, fused_new)
        for name, (base, new) in list(pairs.items())[-3:]:
            a, b = base().view(torch.int16), new().view(torch.int16)
            out['equal'][name] = bool(torch.equal(a, b))
            out.setdefault('outputs_that_differ', {})[name] = int((a != b).sum())
            del a, b
            out['peak_bytes'][name] = {'baseline': peak(base), 'new': peak(new)}
    out['us'], out['graph_chain'] = compare(pairs, rounds)
    out['gate_agrees'] = {}
    for dt in DTYPES:
        t = out['us'][f'{dt}.fused_vs_pair']
        # the gate says "fused wins"; the 16-bit measurement agrees when it is faster (or within the spread: no reason to differ)
        out['gate_agrees'][dt] = (t['verdict'] != 'slower') == out['gate']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_proj_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_proj_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'batch': BATCH, 'x_quant': 'ls-2 (given scales)',
           'w_quant': 'ls-1', 'epilogue': 'relu, projection as res_post', 'shapes': {}, 'summary': {}}
    for name, c, hw, o in SHAPES:
        if only and name not in only:
            continue
        r = res['shapes'][name] = one_shape(c, hw, o, args.rounds)
        for key, t in r['us'].items():
            res['summary'].setdefault(key, {})[name] = {
                'baseline_us': round(t['baseline_us'], 1), 'new_us': round(t['new_us'], 1), 'speedup': round(t['speedup'], 3),
                'verdict': t['verdict'], 'baseline_spread': round(t['baseline_spread'], 3), 'new_spread': round(t['new_spread'], 3),
                'peak_ratio': round(r['peak_bytes'][key]['new'] / max(1, r['peak_bytes'][key]['baseline']), 3)}
        res['summary'].setdefault('gate_agrees', {})[name] = r['gate_agrees']
        print(name, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res['summary']))


if __name__ == '__main__':
    main()
