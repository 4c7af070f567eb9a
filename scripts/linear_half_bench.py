#!/usr/bin/env python3
"""Measurement of the 16-bit-activation x sign-weight linear layer (lsq_linear_signw_half), one JSON document written to
--out and printed.

  python scripts/linear_half_bench.py [--rounds R] [--out profiles/linear_signw_half.json]

The shapes, the graph-replay timing and the alternating rounds are those of scripts/linear_fp_bench.py.  Per shape and
input type (bf16, fp16), microseconds of
  * lsq_linear_signw_half with a 16-bit and with an fp32 output,
  * the route a 16-bit input had before: x.float() -> lsq_linear_signw -> .to(dtype) (`cast_route`), and the same kernel on
    rows that already are fp32 with the fp32 result kept (`cast_route_without_conversions`),
  * F.linear in the 16-bit type on the dense dequantized operands clamp(x), w_q,
and the max error of each against fp64 (the oracle clamps the 16-bit rows as Tensor.clamp does).  `class` is the kernel
the tile rule picks (split / small = 64 x 64 tiles / big = 128 x 128 tiles); `landing` collects, per class and type, the
speedup of the new kernel over the cast route next to the spreads of both: QuantLinear.half_kernel_classes names the
classes where the former exceeds the latter on every shape.  `fp16_subnormals` / `bf16_subnormals` is the known-answer run
of tests/test_gpu_linear_half.py: 64 subnormal activations against an all +1 plane ('kept': their exact sum came out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from linear_fp_bench import DEV, HBM, PEAK_BF16, SHAPES, graph_time, layer  # noqa: E402

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
ALPHA = 2.0


def one_shape(name, m, f, o, ws, rounds):
    from quant import _hip
    from quant.binary import QuantLinear
    x32 = (torch.randn((m, f), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV)
    lin, wsc, wbits, wq, _ = layer(m, f, o, ws, seed=2)
    bias = lin.bias.detach()
    kw = wsc.shape[0]
    out = {'M': m, 'F': f, 'O': o, 'w_quant': ws, 'weight_planes': kw, 'class': QuantLinear._tile_class(m, o)}
    variants, errs = {}, {}
    for dt, dtype in DTYPES.items():
        x = x32.to(dtype)
        xf = x.float()
        xc, wq16, b16 = x.clamp(-ALPHA, ALPHA), wq.to(dtype), bias.to(dtype)
        v = {f'{dt}.half_kernel_out16': lambda x=x: _hip.linear_signw_half(x, ALPHA, wbits, wsc, bias, m, f, o),
             f'{dt}.half_kernel_out32': lambda x=x: _hip.linear_signw_half(x, ALPHA, wbits, wsc, bias, m, f, o,
                                                                            out_dtype=torch.float32),
             f'{dt}.cast_route': lambda x=x, dtype=dtype: _hip.linear_signw(x.float(), ALPHA, wbits, wsc, bias, m, f, o).to(dtype),
             f'{dt}.cast_route_without_conversions': lambda xf=xf: _hip.linear_signw(xf, ALPHA, wbits, wsc, bias, m, f, o),
             f'{dt}.f_linear_16': lambda xc=xc, wq16=wq16, b16=b16: F.linear(xc, wq16, b16)}
        with torch.no_grad():
            y64 = F.linear(xc.double(), wq.double(), bias.double())
            scale = y64.abs().max().item()
            for k, fn in v.items():
                errs[k] = (fn().double() - y64).abs().max().item() / scale
        variants.update(v)
    torch.cuda.synchronize()
    out['max_rel_err_vs_fp64'] = errs

    chain = 10 * 10 if m <= 16 else 200 if m * f * o < 1 << 30 else 10
    reps = 5
    for fn in variants.values():                      # warm-up of every variant, then rounds with the variants alternating
        graph_time(fn, 1, chain)
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(graph_time(fn, reps, chain))
    out['us'] = {k: statistics.median(v) for k, v in samples.items()}
    out['spread'] = {k: (max(v) - min(v)) / statistics.median(v) for k, v in samples.items()}
    out['graph_chain'] = chain
    us = out['us']
    out['speedup_vs_cast_route'] = {dt: us[f'{dt}.cast_route'] / us[f'{dt}.half_kernel_out16'] for dt in DTYPES}
    flops = 2.0 * m * f * o * kw                              # one 16-bit pass per plane
    nbytes = 2.0 * m * f + kw * ((f + 63) // 64) * ((o + 15) // 16 * 16) * 8 + 2.0 * m * o
    t_mfma, t_hbm = flops / PEAK_BF16, nbytes / HBM
    out['flops_16bit'], out['bytes'] = flops, nbytes
    out['bound'] = '16-bit peak' if t_mfma >= t_hbm else 'HBM'
    out['peak_share'] = {dt: max(t_mfma, t_hbm) / (us[f'{dt}.half_kernel_out16'] * 1e-6) for dt in DTYPES}
    return out


def subnormals(dtype):
    """64 subnormals k * (smallest subnormal) against an all +1 ls-1 plane of scale 1: 'kept' (the exact sum), 'flushed' (0)."""
    from quant import _hip
    tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133
    x = (torch.arange(1, 65, dtype=torch.float64) * tiny).to(dtype).view(1, 64).to(DEV)
    g = _hip.make_geom(1, 64, 1, 1, 1, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    ones = torch.ones((1, 1), device=DEV)
    wbits, _ = _hip.pack_weight(torch.full((1, 64, 1, 1), 0.5, device=DEV), g, ones)
    got = _hip.linear_signw_half(x, -1.0, wbits, ones, None, 1, 64, 1, out_dtype=torch.float32).item()
    return {'exact_sum': 2080 * tiny, 'result': got,
            'finding': 'kept' if got == 2080 * tiny else 'flushed' if got == 0 else 'neither'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linear_signw_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'linear_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'peak_16bit_flops': PEAK_BF16, 'hbm_bytes_per_s': HBM,
           'rounds': args.rounds, 'clamp_alpha': ALPHA, 'shapes': {}, 'landing': {},
           'fp16_subnormals': subnormals(torch.float16), 'bf16_subnormals': subnormals(torch.bfloat16)}
    for name, m, f, o, ws in SHAPES:
        if only and name not in only:
            continue
        r = res['shapes'][name] = one_shape(name, m, f, o, ws, args.rounds)
        for dt in DTYPES:
            res['landing'].setdefault(r['class'], {}).setdefault(dt, {})[name] = {
                'speedup_vs_cast_route': r['speedup_vs_cast_route'][dt],
                'spread_half_kernel': r['spread'][f'{dt}.half_kernel_out16'], 'spread_cast_route': r['spread'][f'{dt}.cast_route']}
        print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res['landing']))


if __name__ == '__main__':
    main()
