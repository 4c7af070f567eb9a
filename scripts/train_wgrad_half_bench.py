#!/usr/bin/env python3
"""Measurement of lsq_train_wgrad_half (liblsq_hip_train_half.so, ``hip_train.WGRAD_HALF_KERNEL``), one JSON document written to
--out and printed.

  python scripts/train_wgrad_half_bench.py [--rounds R] [--batch B] [--only NAMES] [--skip-steps] [--out profiles/train_wgrad_half.json]

layers  the five 3 x 3 layer shapes of ResNet-18 at batch B, bf16 and fp16, ls-2 activations, with the bias gradient:
        microseconds of
          kernel        one lsq_train_wgrad_half call: the 16-bit grad_y and the step's sign planes in, grad_wq and grad_b out
          torch_route   (a) what it replaces in the 16-bit step: gy.float(), gy32.sum over (n, ho, wo), lsq_quant_values of
                        x.float(), and conv2d_weight (MIOpen, fp32)
          fp32_kernel   (b) gy.float(), gy32.sum and lsq_train_wgrad
        The method is conv_train_half_bench.py's: HIP-graph replays of `chain` back-to-back calls divided by `chain`, the routes
        alternating in one process, every variant warmed up; the median over the rounds with its spread (max - min over
        median).  That the kernel agrees with route (b) to 1e-5 of max |grad_wq| is checked on every shape before it is timed.
steps   the whole train step of ResNet-18 (ls-1 weights / ls-2 activations) at batch B under torch.autocast('cuda',
        torch.bfloat16) with ``hip_train_half`` and WGRAD_HALF_KERNEL off, on, off again, on again: ms per step, their spread
        and torch.cuda.max_memory_allocated of each."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402

from conv_dgrad_bench import graph_time  # noqa: E402

DEV = 'cuda:0'
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
# (name, C, O, H, stride, layers of ResNet-18 with this shape)
SHAPES = [('c64_56', 64, 64, 56, 1, 4), ('c64_128_56_s2', 64, 128, 56, 2, 1), ('c128_28', 128, 128, 28, 1, 3),
          ('c256_14', 256, 256, 14, 1, 3), ('c512_7', 512, 512, 7, 1, 3)]


def layer_part(batch, shape, dtype, rounds):
    from quant import _hip
    name, c, o, h, s, count = shape
    geom = _hip.make_geom(batch, c, h, h, o, 3, 3, (s, s), (1, 1), (1, 1), 1)
    ho, wo = _hip.out_hw(geom)
    gen = torch.Generator().manual_seed(7)
    gy = (torch.randn((batch, o, ho, wo), generator=gen) * 1e-3).to(dtype).to(DEV)
    x = (torch.randn((batch, c, h, h), generator=gen) * 1.2).to(dtype).to(DEV)
    alpha = float(torch.tensor(2.0, dtype=dtype))
    planes = torch.zeros((2 * _hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xsc = torch.empty((2, batch), dtype=torch.float32, device=DEV)
    _hip.act_quant_half(x, geom, _hip.SCHEME_LS2, 2, 3, alpha, planes, xsc)
    wshape = (o, c, 3, 3)

    def torch_route():
        gy32 = gy.float()
        gb = gy32.sum(dim=(0, 2, 3))
        xq = _hip.quant_values(x.float(), xsc, alpha)
        return torch.nn.grad.conv2d_weight(xq, wshape, gy32, (s, s), (1, 1), (1, 1), 1), gb

    def fp32_kernel():
        gy32 = gy.float()
        return _hip.wgrad(planes, 2, xsc, gy32, geom), gy32.sum(dim=(0, 2, 3))

    variants = {'kernel': lambda: _hip.wgrad_half(planes, 2, xsc, gy, geom, bias=True), 'torch_route': torch_route,
                'fp32_kernel': fp32_kernel}
    (a, ab), (b, bb) = variants['kernel'](), variants['fp32_kernel']()
    torch.cuda.synchronize()
    out = {'C': c, 'O': o, 'H': h, 'stride': s, 'layers': count,
           'kernel_vs_fp32_kernel': float((a - b).abs().max() / b.abs().max()),
           'bias_vs_sum': float((ab - bb).abs().max() / bb.abs().max())}
    assert out['kernel_vs_fp32_kernel'] <= 1e-5 and out['bias_vs_sum'] <= 1e-5, (name, out)
    del a, b, ab, bb
    chain = 3
    samples = {v: [] for v in variants}
    for _ in range(rounds):
        for v, fn in variants.items():
            samples[v].append(graph_time(fn, 5, chain))
    out['us'] = {v: statistics.median(t) for v, t in samples.items()}
    out['spread'] = {v: (max(t) - min(t)) / statistics.median(t) for v, t in samples.items()}
    out['torch_route_over_kernel'] = out['us']['torch_route'] / out['us']['kernel']
    out['fp32_kernel_over_kernel'] = out['us']['fp32_kernel'] / out['us']['kernel']
    out['kernel_tflops'] = 2.0 * gy.numel() * c * 9 * 2 / (out['us']['kernel'] * 1e-6) / 1e12       # (two planes)
    out['graph_chain'] = chain
    return out


def autocast_steps(batch, steps, warmup, switch, dev):
    """conv_train_half_bench.autocast_steps (hip_train_half on) with WGRAD_HALF_KERNEL = ``switch``, plus the spread of the steps."""
    import conv_train_half_bench
    from quant.binary import hip_train
    hip_train.WGRAD_HALF_KERNEL = switch
    try:
        return conv_train_half_bench.autocast_steps(batch, steps, warmup, True, dev)
    finally:
        hip_train.WGRAD_HALF_KERNEL = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--skip-steps', action='store_true', help='per-layer times only')
    ap.add_argument('--skip-layers', action='store_true', help='train steps only')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_wgrad_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'train_wgrad_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'what': 'train_wgrad_half', 'device': torch.cuda.get_device_name(0), 'batch': args.batch, 'rounds': args.rounds,
           'activations': 'ls-2', 'layers': {}}
    if not args.skip_layers:
        for tname, dtype in DTYPES.items():
            rows = {}
            for shape in SHAPES:
                if only and shape[0] not in only:
                    continue
                rows[shape[0]] = layer_part(args.batch, shape, dtype, args.rounds)
                print(tname, shape[0], json.dumps(rows[shape[0]]), flush=True)
                torch.cuda.empty_cache()
            res['layers'][tname] = {'shapes': rows,
                                    'network_total_us': {v: sum(r['us'][v] * r['layers'] for r in rows.values())
                                                         for v in ('kernel', 'torch_route', 'fp32_kernel')}}
    if not args.skip_steps:
        dev = torch.device(DEV)
        steps = {}
        for key, switch in (('switch_off', False), ('switch_on', True), ('switch_off_again', False), ('switch_on_again', True)):
            steps[key] = autocast_steps(args.batch, args.steps, args.warmup, switch, dev)
            print('step', key, json.dumps(steps[key]), flush=True)
        off = statistics.median([steps['switch_off']['ms_per_step_median'], steps['switch_off_again']['ms_per_step_median']])
        on = statistics.median([steps['switch_on']['ms_per_step_median'], steps['switch_on_again']['ms_per_step_median']])
        steps['off_over_on'] = off / on
        steps['spread_between_rounds'] = {
            'off': abs(steps['switch_off']['ms_per_step_median'] - steps['switch_off_again']['ms_per_step_median']) / off,
            'on': abs(steps['switch_on']['ms_per_step_median'] - steps['switch_on_again']['ms_per_step_median']) / on}
        res['train_step'] = dict(net='resnet18_imagenet_ls1w_ls2a', autocast='bfloat16', hip_train_half=True, **steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
