#!/usr/bin/env python3
"""Measurement of QuantConv2d's input gradient on its own kernel (lsq_signw_conv2d_dgrad, quant.binary.hip_train with
DGRAD_KERNEL), one JSON document written to --out and printed.

  python scripts/conv_dgrad_bench.py [--rounds R] [--batch B] [--only NAMES] [--skip-steps] [--out profiles/conv_dgrad.json]

layers  the 16 quantized 3 x 3 layers and the three 1 x 1 stride-2 projections of ResNet-18 at batch B (ten distinct shapes,
        each with the number of layers that have it), ls-1 and ls-2 weights: microseconds of
          kernel     one lsq_signw_conv2d_dgrad call, the transpose of the planes into the workspace included, against
          old_route  what hip_train's backward does with the switch off: per weight plane the residual tensor, its permute /
                     flip / copy, lsq_pack_weight and one lsq_signw_conv2d, later planes through res_post; stride 2 over a
                     zero-filled, scattered-into gradient of the stride-1 size.
        HIP-graph replays of `chain` back-to-back calls divided by `chain`, both routes alternating, every variant warmed up;
        the median over the rounds with its spread (max - min over median).  The max difference of the two routes' results
        relative to max |gx| is recorded too (both are held to fp64 by the tests).
steps   scripts/train_step.py's whole train step of ResNet-18 (ls-1 weights / ls-2 activations) at batch B with the switch
        off and on, alternating: ms per step and torch.cuda.max_memory_allocated."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402

DEV = 'cuda:0'
PEAK_BF16 = 2.5e15       # dense bf16 MFMA FLOP/s of the MI355X
# (name, C, O, H, kernel, stride, pad, layers of ResNet-18 with this shape)
SHAPES = [('c64_56', 64, 64, 56, 3, 1, 1, 4), ('c64_128_56_s2', 64, 128, 56, 3, 2, 1, 1), ('c128_28', 128, 128, 28, 3, 1, 1, 3),
          ('c128_256_28_s2', 128, 256, 28, 3, 2, 1, 1), ('c256_14', 256, 256, 14, 3, 1, 1, 3),
          ('c256_512_14_s2', 256, 512, 14, 3, 2, 1, 1), ('c512_7', 512, 512, 7, 3, 1, 1, 3),
          ('proj64_128_56', 64, 128, 56, 1, 2, 0, 1), ('proj128_256_28', 128, 256, 28, 1, 2, 0, 1),
          ('proj256_512_14', 256, 512, 14, 1, 2, 0, 1)]
W_SCHEMES = ('ls-1', 'ls-2')


def graph_time(fn, reps, chain):
    """median us per call of `chain` calls captured in one graph and replayed `reps` times."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(chain):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / chain)
    del g
    return statistics.median(ts)


def old_route(_hip, gy, weight, wscales, n, c, h, w, o, k, s, p):
    """grad_xq as hip_train's backward computes it with DGRAD_KERNEL off (the same calls in the same order)."""
    from quant.binary.hip_train import _constants, _weight_residual_planes
    if s == 1:
        gin = gy
    else:
        hu, wu = h + 2 * p - k + 1, w + 2 * p - k + 1
        gin = gy.new_zeros((n, o, hu, wu))
        gin[:, :, ::s, ::s][:, :, :gy.shape[2], :gy.shape[3]] = gy
    tgeom = _hip.make_geom(n, o, gin.shape[2], gin.shape[3], c, k, k, (1, 1), (k - 1 - p, k - 1 - p), (1, 1), 1)
    ones, zeros = _constants(c, o, gy.device)
    gxq = None
    for r, u in zip(_weight_residual_planes(weight, wscales), wscales):
        wt = r.permute(1, 0, 2, 3).flip(2, 3).contiguous()
        tbits, _ = _hip.pack_weight(wt, tgeom, ones)
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=gy.device)
        _hip.signw_conv2d(gin, -1.0, tbits, ones, None, tgeom, out, pre=(u.contiguous(), zeros), res_post=gxq)
        gxq = out
    return gxq


def layer_part(batch, shape, ws, rounds):
    from quant import _hip
    from quant.binary.binary_conv import QuantConv2d
    name, c, o, h, k, s, p, count = shape
    conv = QuantConv2d('ls-2', ws, c, o, k, {'kind': 'symmetric', 'alpha': 2}, stride=s, padding=p, bias=False)
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (c * k * k) ** -0.5)
    conv = conv.to(DEV).train()
    weight = conv.weight.detach()
    with torch.no_grad():
        conv.w_approximate(weight)
        wsc = conv.w_approximate.plane_scales().to(torch.float32).contiguous()
    geom = _hip.make_geom(batch, c, h, h, o, k, k, (s, s), (p, p), (1, 1), 1)
    ho, wo = _hip.out_hw(geom)
    wbits, _ = _hip.pack_weight(weight, geom, wsc)
    gy = (torch.randn((batch, o, ho, wo), generator=gen) * 1e-3).to(DEV)

    variants = {'kernel': lambda: _hip.signw_conv2d_dgrad(gy, wbits, wsc, geom),
                'old_route': lambda: old_route(_hip, gy, weight, wsc, batch, c, h, h, o, k, s, p)}
    a, b = variants['kernel'](), variants['old_route']()
    torch.cuda.synchronize()
    out = {'C': c, 'O': o, 'H': h, 'kernel_size': k, 'stride': s, 'layers': count, 'weight_planes': int(wsc.shape[0]),
           'max_diff_of_routes_over_max': float((a - b).abs().max() / b.abs().max())}
    del a, b
    chain = 3
    samples = {v: [] for v in variants}
    for _ in range(rounds):
        for v, fn in variants.items():
            samples[v].append(graph_time(fn, 5, chain))
    out['us'] = {v: statistics.median(t) for v, t in samples.items()}
    out['spread'] = {v: (max(t) - min(t)) / statistics.median(t) for v, t in samples.items()}
    out['old_over_kernel'] = out['us']['old_route'] / out['us']['kernel']
    flops = 2.0 * 2.0 * batch * ho * wo * o * c * k * k * int(wsc.shape[0])      # hi and lo pass of every plane, no zero taps
    out['bf16_peak_share_of_kernel'] = flops / PEAK_BF16 / (out['us']['kernel'] * 1e-6)
    out['graph_chain'] = chain
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--skip-steps', action='store_true', help='per-layer times only')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_dgrad.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_dgrad_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'what': 'conv_dgrad', 'device': torch.cuda.get_device_name(0), 'batch': args.batch, 'rounds': args.rounds,
           'peak_bf16_flops': PEAK_BF16, 'layers': {}}
    for ws in W_SCHEMES:
        rows = {}
        for shape in SHAPES:
            if only and shape[0] not in only:
                continue
            rows[shape[0]] = layer_part(args.batch, shape, ws, args.rounds)
            print(ws, shape[0], json.dumps(rows[shape[0]]), flush=True)
            torch.cuda.empty_cache()
        res['layers'][ws] = {'shapes': rows,
                             'network_total_us': {v: sum(r['us'][v] * r['layers'] for r in rows.values())
                                                  for v in ('kernel', 'old_route')}}
    if not args.skip_steps:
        import train_step
        from quant.binary import hip_train
        dev = torch.device(DEV)
        runs = {'off': [], 'on': []}
        for _ in range(2):                                # off, on, off, on
            for key, flag in (('off', False), ('on', True)):
                hip_train.DGRAD_KERNEL = flag
                runs[key].append(train_step.train_steps(args.batch, args.steps, args.warmup, False, dev))
                print('step', key, json.dumps(runs[key][-1]), flush=True)
        hip_train.DGRAD_KERNEL = False
        res['train_step'] = {'net': 'resnet18_imagenet_ls1w_ls2a', 'wgrad_kernel': False, 'runs': runs,
                             'ms_per_step_median': {k: statistics.median(r['ms_per_step_median'] for r in v) for k, v in runs.items()},
                             'max_memory_allocated_gib': {k: max(r['max_memory_allocated_gib'] for r in v) for k, v in runs.items()}}
        m = res['train_step']['ms_per_step_median']
        res['train_step']['off_over_on'] = m['off'] / m['on']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
