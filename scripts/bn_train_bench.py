#!/usr/bin/env python3
"""Measurement of the train-mode batch norm folded into QuantConv2d's train step (QuantConv2d.train_bn_fold), one
JSON document written to --out and printed.

  python scripts/bn_train_bench.py [--rounds R] [--reps K] [--steps S] [--only NAMES] [--skip-steps] [--out profiles/bn_train.json]

The comparator is the route without the fold in the same process: every round times (off, on, off) and a sample is the median
of K event-timed repetitions; `off_spread` is (max - min) / median over all samples of the off route and `verdict` is 'tie'
where the medians differ by less than that spread, else 'faster' / 'slower'.
  * `half_block`: per quantizer shape of ResNet-18 at batch 256 (ls-2 activations, ls-1 weights, 3 x 3, stride 1, O = C),
    milliseconds of forward plus backward of one bn -> conv pair, and of torch's batch norm alone on that shape (forward plus
    backward): 16 of those, weighted as the network has them, are `torch_bn_ms_per_step`;
  * `step`: milliseconds per train step (forward, backward, SGD) of the ResNet-18 of bench.py at batch 256 and
    torch.cuda.max_memory_allocated, both ways; `torch_bn_share_of_step` is torch_bn_ms_per_step over the off route's step.
QuantConv2d.train_bn_fold stays False whatever this prints."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402

DEV = torch.device('cuda:0')
BATCH = 256
# (name, C, H = W, bn -> conv pairs of that input shape in the network): the inputs of ResNet-18's quantized 3 x 3 layers
SHAPES = [('c64_56', 64, 56, 5), ('c128_28', 128, 28, 4), ('c256_14', 256, 14, 4), ('c512_7', 512, 7, 3)]


def set_fold(on):
    from quant.binary.binary_conv import QuantConv2d
    QuantConv2d.train_bn_fold = bool(on)


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


def compare(off, on, rounds, reps):
    """off / on: callables.  Alternating samples (off, on, off) per round."""
    for _ in range(3):
        off()
        on()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(off, reps))
        b.append(timed(on, reps))
        a.append(timed(off, reps))
    base, new = statistics.median(a), statistics.median(b)
    spread = (max(a) - min(a)) / base
    verdict = 'tie' if abs(new - base) < spread * base else ('faster' if new < base else 'slower')
    return {'off_ms': base, 'on_ms': new, 'off_samples': a, 'on_samples': b, 'off_spread': spread, 'speedup': base / new,
            'verdict': verdict}


def half_block(c, hw, rounds, reps):
    from quant.binary.binary_conv import QuantConv2d
    from quant.models.resnet import _bn_conv
    g = torch.Generator().manual_seed(c)
    conv = QuantConv2d('ls-2', 'ls-1', c, c, 3, {'kind': 'symmetric', 'alpha': 3}, padding=1).to(DEV).train()
    bn = torch.nn.BatchNorm2d(c).to(DEV).train()
    x = (torch.randn((BATCH, c, hw, hw), generator=g) * 1.2 + 0.3).to(DEV).requires_grad_()
    gy = (torch.randn((BATCH, c, hw, hw), generator=g) * 1e-3).to(DEV)

    def pair(on):
        set_fold(on)
        x.grad = None
        _bn_conv(bn, conv, x).backward(gy)

    def bn_alone():
        x.grad = None
        bn(x).backward(gy)

    out = compare(lambda: pair(False), lambda: pair(True), rounds, reps)
    set_fold(False)
    for _ in range(3):
        bn_alone()
    out['torch_bn_alone_ms'] = statistics.median([timed(bn_alone, reps) for _ in range(rounds)])
    out.update(N=BATCH, C=c, H=hw, W=hw, elements=BATCH * c * hw * hw)
    return out


def train_steps(on, steps, warmup):
    set_fold(on)
    model = bench.build_model(bench.imagenet_arch('ls-2'), DEV).train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn((BATCH, 3, 224, 224), generator=g, device=DEV)
    y = torch.randint(0, 1000, (BATCH,), generator=g, device=DEV)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = F.cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    times = []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        loss = step()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e))
    out = {'ms_per_step_median': statistics.median(times), 'ms_per_step_min': min(times), 'ms_per_step_max': max(times),
           'max_memory_allocated_gib': torch.cuda.max_memory_allocated(DEV) / 2 ** 30, 'last_loss': float(loss.detach())}
    del model, opt, x, y
    set_fold(False)
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--skip-steps', action='store_true', help='half-blocks only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bn_train.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bn_train_bench.py measures on the GPU'
    only = set(filter(None, a.only.split(',')))
    res = {'what': 'bn_train', 'device': torch.cuda.get_device_name(0), 'batch': BATCH, 'rounds': a.rounds, 'reps': a.reps,
           'x_quant': 'ls-2', 'w_quant': 'ls-1', 'half_block': {}}
    bn_ms = 0.0
    for name, c, hw, count in SHAPES:
        if only and name not in only:
            continue
        r = res['half_block'][name] = half_block(c, hw, a.rounds, a.reps)
        r['pairs_in_network'] = count
        bn_ms += count * r['torch_bn_alone_ms']
        print(name, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    res['torch_bn_ms_per_step'] = bn_ms
    if not a.skip_steps:
        runs = [('off', False), ('on', True), ('off_again', False)]
        res['step'] = {tag: train_steps(on, a.steps, a.warmup) for tag, on in runs}
        off = statistics.median([res['step']['off']['ms_per_step_median'], res['step']['off_again']['ms_per_step_median']])
        res['step']['off_ms'] = off
        res['step']['off_spread'] = abs(res['step']['off']['ms_per_step_median']
                                        - res['step']['off_again']['ms_per_step_median']) / off
        res['step']['speedup'] = off / res['step']['on']['ms_per_step_median']
        res['torch_bn_share_of_step'] = bn_ms / off
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps({k: v for k, v in res.items() if k != 'half_block'}))


if __name__ == '__main__':
    main()
