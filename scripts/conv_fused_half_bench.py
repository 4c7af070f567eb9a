#!/usr/bin/env python3
"""Measurement of the fused 16-bit block half for fp activations (lsq_signw_conv2d_fused_half, QuantConv2d.fp_half_fused /
fp_half_bn_fold), one JSON document merged into --out and printed.

  python scripts/conv_fused_half_bench.py [--rounds R] [--only NAMES] [--out profiles/conv_fused_half.json]

The graph-replay timing and the comparison are those of scripts/conv_xnor_half_bench.py (HIP-graph replays of 10 calls, the
median of R alternating rounds, the baseline sampled twice a round; `verdict` is 'tie' inside the baseline's own spread).  Per
3 x 3 layer shape of ResNet-18 at batch 256 and 100 x 64 x 32 x 32, weights ls-1 / ls-2, type bf16 / fp16 and block-half
variant (`post`: pre_bn + PReLU + res_post; `pre`: pre_bn + PReLU + res_pre), `fused_forward` on three routes of one module:
  (a) fp_half alone: torch's batch norm, lsq_signw_conv2d_half, the epilogue composed in torch -- the baseline;
  (b) fp_half_fused: torch's batch norm, one lsq_signw_conv2d_fused_half;
  (c) fp_half_fused + fp_half_bn_fold: one lsq_signw_conv2d_fused_half.
`us` holds the pairs (a, b) as `.fused` and (a, c) as `.fold`; `peak_bytes` is torch.cuda.max_memory_allocated over one call
above what was allocated before it; `error` is max|y - y64| / max|y64| of each route on the first ERR_SAMPLES samples against
the fp64 composition (batch norm, clamp, convolution, epilogue) on the 16-bit input, computed on the CPU.  A shape runs in one
process (--only), so that a caller can put every one under its own time limit; --out is read, updated and rewritten.  Both
switches stay False whatever this prints."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from conv_xnor_half_bench import compare, peak  # noqa: E402
from linear_fp_bench import DEV  # noqa: E402

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
CLAMP = {'kind': 'symmetric', 'alpha': 2}
ERR_SAMPLES = 4
# (name, N, C, H = W, O, stride): every distinct 3 x 3 quantized layer of ResNet-18 at batch 256, and the CIFAR shape
SHAPES = [('c64_56', 256, 64, 56, 64, 1), ('c64_56_s2', 256, 64, 56, 128, 2), ('c128_28', 256, 128, 28, 128, 1),
          ('c128_28_s2', 256, 128, 28, 256, 2), ('c256_14', 256, 256, 14, 256, 1), ('c256_14_s2', 256, 256, 14, 512, 2),
          ('c512_7', 256, 512, 7, 512, 1), ('c64_32_n100', 100, 64, 32, 64, 1)]
ROUTES = {'a': (False, False), 'b': (True, False), 'c': (True, True)}


def module(ws, c, o, stride, seed):
    from quant.binary.binary_conv import QuantConv2d
    from oracle import ref_port as P
    g = torch.Generator().manual_seed(seed)
    conv = QuantConv2d('fp', ws, c, o, 3, CLAMP, padding=1, stride=stride)
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.05)
        conv.bias.copy_(torch.randn((o,), generator=g) * 0.1)
        for buf, v in zip(conv.w_approximate.cached_scales(), P.weight_scales(conv.weight, ws)):
            buf.copy_(v)
        bn.running_mean.copy_(torch.randn((c,), generator=g) * 0.2)
        bn.running_var.copy_(torch.rand((c,), generator=g) + 0.5)
        bn.weight.copy_(torch.rand((c,), generator=g) + 0.5)
        bn.bias.copy_(torch.randn((c,), generator=g) * 0.3)
    conv.fp_half = True
    return conv.eval().to(DEV), bn.eval().to(DEV)


def fp64_block(conv, bn, ws, x, res, slopes, post):
    """The block half in fp64 on the CPU, on the 16-bit input as it is."""
    from oracle import ref_port as P
    w = conv.weight.detach().cpu()
    wq = P.quantize_weight(w, ws, [b.cpu() for b in conv.w_approximate.cached_scales()]).double()
    t = F.batch_norm(x.cpu().double(), bn.running_mean.cpu().double(), bn.running_var.cpu().double(), bn.weight.detach().cpu().double(),
                     bn.bias.detach().cpu().double(), False, 0.0, bn.eps).clamp(-2.0, 2.0)
    y = F.conv2d(t, wq, conv.bias.detach().cpu().double(), conv.stride, conv.padding)
    r = res.cpu().double()
    y = y if post else y + r
    y = torch.where(y > 0, y, slopes.cpu().double().view(1, -1, 1, 1) * y)
    return y + r if post else y


def one_shape(n, c, hw, o, stride, rounds):
    from quant import _hip
    geom = _hip.make_geom(n, c, hw, hw, o, 3, 3, (stride, stride), (1, 1), (1, 1), 1)
    ho, wo = _hip.out_hw(geom)
    x32 = (torch.randn((n, c, hw, hw), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV)
    r32 = torch.randn((n, o, ho, wo), generator=torch.Generator().manual_seed(3)).to(DEV)
    slopes = (torch.rand((o,), generator=torch.Generator().manual_seed(4)) * 0.5).to(DEV)
    out = {'N': n, 'C': c, 'H': hw, 'W': hw, 'O': o, 'stride': stride, 'outputs': n * o * ho * wo, 'peak_bytes': {}, 'error': {},
           'outputs_that_differ_from_a': {}}
    pairs = {}
    for ws in ('ls-1', 'ls-2'):
        conv, bn = module(ws, c, o, stride, seed=2)
        for dt, dtype in DTYPES.items():
            x, res = x32.to(dtype), r32.to(dtype)
            for variant, post in (('post', True), ('pre', False)):
                key = f'{ws}.{dt}.{variant}'

                def run(route, x=x, res=res, conv=conv, bn=bn, post=post):
                    conv.fp_half_fused, conv.fp_half_bn_fold = ROUTES[route]
                    with torch.no_grad():
                        return conv.fused_forward(x, pre_bn=bn, prelu=slopes, **({'res_post': res} if post else {'res_pre': res}))

                fb, fc = (lambda run=run: run('b')), (lambda run=run: run('c'))

                # (route a's torch PReLU takes fp32 slopes on a 16-bit tensor only under an autocast of the type)
                def fa(run=run, dtype=dtype):
                    with torch.autocast('cuda', dtype=dtype):
                        return run('a')

                pairs[key + '.fused'] = (fa, fb)
                pairs[key + '.fold'] = (fa, fc)
                out['peak_bytes'][key] = {'a': peak(fa), 'b': peak(fb), 'c': peak(fc)}
                ya = fa()
                out['outputs_that_differ_from_a'][key] = {r: int((f().view(torch.int16) != ya.view(torch.int16)).sum())
                                                          for r, f in (('b', fb), ('c', fc))}
                del ya
                xs, rs = x[:ERR_SAMPLES].contiguous(), res[:ERR_SAMPLES].contiguous()
                y64 = fp64_block(conv, bn, ws, xs, rs, slopes, post)
                err = {}
                for route in ROUTES:
                    with torch.autocast('cuda', dtype=dtype, enabled=route == 'a'):
                        y = run(route, x=xs, res=rs)
                    err[route] = ((y.cpu().double() - y64).abs().max() / y64.abs().max()).item()
                out['error'][key] = err
    out['us'], out['graph_chain'] = compare(pairs, rounds, chain=10)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_fused_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_fused_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'shapes': {}, 'summary': {}}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            res = json.load(fh)
    res.update(device=torch.cuda.get_device_name(0), rounds=args.rounds, x_quant='fp', err_samples=ERR_SAMPLES)
    for name, n, c, hw, o, stride in SHAPES:
        if only and name not in only:
            continue
        r = res['shapes'][name] = one_shape(n, c, hw, o, stride, args.rounds)
        for key, t in r['us'].items():
            res['summary'].setdefault(key, {})[name] = {
                'baseline_us': round(t['baseline_us'], 1), 'new_us': round(t['new_us'], 1), 'speedup': round(t['speedup'], 3),
                'verdict': t['verdict'], 'baseline_spread': round(t['baseline_spread'], 3)}
        print(name, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res['summary']))


if __name__ == '__main__':
    main()
