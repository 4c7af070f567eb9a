#!/usr/bin/env python3
"""Measurement of the 16-bit quantizer with the eval batch norm folded into its read (lsq_act_quant_bn_half,
QuantConv2d.act_half_bn_fold), one JSON document written to --out and printed.

  python scripts/conv_act_bn_half_bench.py [--rounds R] [--only NAMES] [--out profiles/conv_act_bn_half.json]

The graph-replay timing is that of scripts/linear_fp_bench.py, the comparison that of scripts/conv_xnor_half_bench.py: every
round times (baseline, new, baseline again); `baseline_spread` is (max - min) / median over all samples of the baseline;
`verdict` is 'tie' where the medians differ by less than that spread, else 'faster' / 'slower'.  Per quantizer shape of
ResNet-18 at batch 256 and input type (bf16, fp16):
  * `quant.<scheme>`: microseconds of `bn(x)` in torch followed by `act_quant_half` (the route without the fold) against one
    `act_quant_bn_half` on x -- ls-1, ls-2 free-running (skip 3) and ls-2 with given scales;
  * `block.<scheme>`: microseconds of `fused_forward(x16, pre_bn=bn, relu=True, res_pre=r16)` with act_half and xnor_half on,
    act_half_bn_fold off against on -- ls-1 and ls-2 free-running, 3 x 3, stride 1, O = C;
  * `deviation`: between the folded tensor t = (x.float() * scale + shift).to(dtype) and torch's `bn(x)` -- the share of
    elements whose bits differ and the largest difference in ulps of the type.  Both round one fp32 evaluation of the same
    affine map, associated differently: a record, not a gate;
  * `equal`: the planes and scales of the fold against `act_quant_half` on t, bit for bit, on the timed inputs.
The replays of one graph re-read the same tensors, so up to the 256 MiB Infinity Cache they may come from there rather than
from HBM -- for both routes alike.  QuantConv2d.act_half_bn_fold stays False whatever this prints."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402

from conv_xnor_half_bench import compare  # noqa: E402
from linear_fp_bench import DEV  # noqa: E402

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
CLAMP = {'kind': 'symmetric', 'alpha': 2}
BATCH = 256
LS1, LS2 = 1, 2
# (name, C, H = W): the inputs of the quantized 3 x 3 layers of ResNet-18 (quant/models/resnet.py)
SHAPES = [('c64_56', 64, 56), ('c128_28', 128, 28), ('c256_14', 256, 14), ('c512_7', 512, 7)]
# (name, scheme, k, scales given)
QUANT = [('ls-1', LS1, 1, False), ('ls-2 free', LS2, 2, False), ('ls-2 given', LS2, 2, True)]


def module(xq, c, seed):
    from quant.binary.binary_conv import QuantConv2d
    from oracle import ref_port as P
    g = torch.Generator().manual_seed(seed)
    conv = QuantConv2d(xq, 'ls-1', c, c, 3, CLAMP, padding=1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.05)
        conv.bias.copy_(torch.randn((c,), generator=g) * 0.1)
        for buf, v in zip(conv.w_approximate.cached_scales(), P.weight_scales(conv.weight, 'ls-1')):
            buf.copy_(v)
    conv.act_half = conv.xnor_half = True
    return conv.eval().to(DEV)


def batch_norm(c, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand((c,), generator=g))
        bn.bias.copy_(torch.randn((c,), generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn((c,), generator=g) * 0.3)
        bn.running_var.copy_(0.5 + torch.rand((c,), generator=g))
    return bn.eval().to(DEV)


def ordered(t):
    """The 16 bits of a bf16 / fp16 tensor as integers in the order of the values (one step = one ulp)."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def one_shape(c, hw, rounds):
    from quant import _hip
    n = BATCH
    geom = _hip.make_geom(n, c, hw, hw, c, 3, 3, (1, 1), (1, 1), (1, 1), 1)
    x32 = (torch.randn((n, c, hw, hw), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV)
    r32 = torch.randn((n, c, hw, hw), generator=torch.Generator().manual_seed(3)).to(DEV)
    bn = batch_norm(c, seed=4)
    convs = {'ls-1': module('ls-1', c, seed=2), 'ls-2 free': module('ls-2', c, seed=2)}
    pre = convs['ls-1']._folded_bn(bn)
    words = _hip.act_plane_words(geom)
    forced = torch.tensor([[0.9], [0.45]]).expand(2, n).contiguous().to(DEV)
    out = {'N': n, 'C': c, 'H': hw, 'W': hw, 'elements': n * c * hw * hw, 'equal': {}, 'deviation': {}}
    pairs = {}
    for dt, dtype in DTYPES.items():
        x, res = x32.to(dtype), r32.to(dtype)
        with torch.no_grad():
            t = (x.float() * pre[0].view(1, -1, 1, 1) + pre[1].view(1, -1, 1, 1)).to(dtype)
            d = (ordered(t) - ordered(bn(x))).abs()
        out['deviation'][dt] = {'share_of_elements_that_differ': float((d != 0).float().mean()), 'max_ulps': int(d.max())}
        del d
        for name, scheme, k, given in QUANT:
            planes = [torch.zeros((k * words,), dtype=torch.int64, device=DEV) for _ in range(2)]
            scales = [torch.empty((k, n), device=DEV) for _ in range(2)]
            f = forced if given else None

            def base(x=x, scheme=scheme, k=k, f=f, planes=planes[0], scales=scales[0]):
                with torch.no_grad():
                    _hip.act_quant_half(bn(x), geom, scheme, k, 3, 2.0, planes, scales, f)

            def new(x=x, scheme=scheme, k=k, f=f, planes=planes[1], scales=scales[1]):
                _hip.act_quant_bn_half(x, geom, scheme, k, 3, 2.0, planes, scales, f, pre)

            _hip.act_quant_half(t, geom, scheme, k, 3, 2.0, planes[0], scales[0], f)
            new()
            out['equal'][f'{dt}.quant.{name}'] = bool(torch.equal(planes[0], planes[1])
                                                      and torch.equal(scales[0].view(torch.int32), scales[1].view(torch.int32)))
            pairs[f'{dt}.quant.{name}'] = (base, new)
        del t
        for name, conv in convs.items():
            def block(on, conv=conv, x=x, res=res):
                conv.act_half_bn_fold = on
                with torch.no_grad():
                    return conv.fused_forward(x, pre_bn=bn, relu=True, res_pre=res)

            pairs[f'{dt}.block.{name}'] = ((lambda block=block: block(False)), (lambda block=block: block(True)))
            a, b = block(False), block(True)
            out[f'{dt}.block.{name}.outputs_that_differ_from_torch_bn'] = float((a.view(torch.int16) != b.view(torch.int16)).float().mean())
            del a, b
    out['us'], out['graph_chain'] = compare(pairs, rounds)
    for conv in convs.values():
        conv.act_half_bn_fold = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_act_bn_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_act_bn_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'batch': BATCH, 'w_quant': 'ls-1', 'clamp': 2.0,
           'skip': 3, 'shapes': {}, 'summary': {}}
    for name, c, hw in SHAPES:
        if only and name not in only:
            continue
        r = res['shapes'][name] = one_shape(c, hw, args.rounds)
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
