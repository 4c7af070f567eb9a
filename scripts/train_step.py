#!/usr/bin/env python3
"""Train-step measurement of the weight-gradient kernel (lsq_train_wgrad), one JSON line on stdout.

  python scripts/train_step.py [--steps K] [--warmup W] [--batch B] [--reps R]

1. ms per train step (forward, backward, SGD step) of the headline network -- ResNet-18 ImageNet, ls-1 weights / ls-2
   activations, bench.py's arch_config -- at batch B on cuda:0, with quant.binary.hip_train.WGRAD_KERNEL on and off, and
   torch.cuda.max_memory_allocated of each run;
2. per layer, for the 16 binary 3x3 layer shapes at batch B: the kernel against lsq_quant_values + conv2d_weight (HIP events,
   median of R), each against the fp16 matrix-core floor (two-term fp16 split: 2 kx MFMA passes of the layer's MACs at
   2.5 PF dense) and the kernel against its own floor (three bf16 terms: 3 kx passes)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402

PEAK_16BIT = 2.5e15      # dense fp16 / bf16 MFMA FLOP/s of the MI355X
RESNET18_LAYERS = ([(64, 64, 56, 1)] * 4 + [(64, 128, 56, 2)] + [(128, 128, 28, 1)] * 3 + [(128, 256, 28, 2)]
                   + [(256, 256, 14, 1)] * 3 + [(256, 512, 14, 2)] + [(512, 512, 7, 1)] * 3)


def train_steps(batch, steps, warmup, wgrad_kernel, dev):
    from quant.binary import hip_train
    hip_train.WGRAD_KERNEL = wgrad_kernel
    model = bench.build_model(bench.imagenet_arch('ls-2'), dev).train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((batch, 3, 224, 224), generator=g, device=dev)
    y = torch.randint(0, 1000, (batch,), generator=g, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    times = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        loss = step()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    out = {'ms_per_step_median': statistics.median(times), 'ms_per_step_min': min(times),
           'max_memory_allocated_gib': torch.cuda.max_memory_allocated(dev) / 2 ** 30, 'last_loss': float(loss)}
    del model, opt, x, y
    torch.cuda.empty_cache()
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def layer_times(batch, reps, dev):
    from quant import _hip
    rows, memo = [], {}
    for idx, (c, o, h, s) in enumerate(RESNET18_LAYERS):
        if (c, o, h, s) not in memo:
            geom = _hip.make_geom(batch, c, h, h, o, 3, 3, (s, s), (1, 1), (1, 1), 1)
            ho, wo = _hip.out_hw(geom)
            gen = torch.Generator(device=dev).manual_seed(idx)
            x = torch.randn((batch, c, h, h), generator=gen, device=dev)
            gy = torch.randn((batch, o, ho, wo), generator=gen, device=dev) * 1e-4
            k = 2
            planes = torch.zeros((k * _hip.act_plane_words(geom),), dtype=torch.int64, device=dev)
            scales = torch.empty((k, batch), dtype=torch.float32, device=dev)
            _hip.act_quant(x, geom, _hip.SCHEME_LS2, k, 3, 3.0, planes, scales)
            kern = lambda: _hip.wgrad(planes, k, scales, gy, geom)                         # noqa: E731
            torch_ = lambda: torch.nn.grad.conv2d_weight(_hip.quant_values(x, scales, 3.0), (o, c, 3, 3), gy,   # noqa: E731
                                                         (s, s), (1, 1))
            for _ in range(3):
                kern()
                torch_()
            tk, tt = timed(kern, reps), timed(torch_, reps)
            macs = batch * ho * wo * o * c * 9
            floor16 = 2 * macs * 2 * k / PEAK_16BIT * 1e3          # ms: fp16 hi + lo, 2 kx passes
            floor_own = 2 * macs * 3 * k / PEAK_16BIT * 1e3        # ms: bf16 hi + mid + lo, 3 kx passes
            memo[(c, o, h, s)] = {'kernel_ms': tk, 'quant_values_conv2d_weight_ms': tt, 'fp16_floor_ms': floor16,
                                  'kernel_floor_ms': floor_own, 'kernel_vs_fp16_floor': tk / floor16,
                                  'torch_vs_fp16_floor': tt / floor16, 'kernel_vs_own_floor': tk / floor_own,
                                  'speedup': tt / tk}
            del x, gy, planes, scales
        rows.append(dict(layer=idx, C=c, O=o, H=h, stride=s, **memo[(c, o, h, s)]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--skip-steps', action='store_true', help='per-layer times only')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    t0 = time.time()
    res = {'what': 'train_step', 'net': 'resnet18_imagenet_ls1w_ls2a', 'batch': a.batch, 'device': torch.cuda.get_device_name(dev)}
    if not a.skip_steps:
        res['step_wgrad_kernel'] = train_steps(a.batch, a.steps, a.warmup, True, dev)
        res['step_conv2d_weight'] = train_steps(a.batch, a.steps, a.warmup, False, dev)
        res['step_speedup'] = res['step_conv2d_weight']['ms_per_step_median'] / res['step_wgrad_kernel']['ms_per_step_median']
    layers = layer_times(a.batch, a.reps, dev)
    res['layers'] = layers
    res['layers_total_kernel_ms'] = sum(r['kernel_ms'] for r in layers)
    res['layers_total_quant_values_conv2d_weight_ms'] = sum(r['quant_values_conv2d_weight_ms'] for r in layers)
    res['layers_total_fp16_floor_ms'] = sum(r['fp16_floor_ms'] for r in layers)
    res['seconds'] = round(time.time() - t0, 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
