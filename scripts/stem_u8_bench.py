"""lsq_stem_conv_u8 on uint8 input against the route the same bytes take without it, on the GPU.

Per call, for the ImageNet stem (batch 256 and 64), the CIFAR stem (batch 100) and LeNet's front (batch 64):
  norm+kernel[_cl]  torch normalisation of the uint8 batch (NCHW / channels-last bytes) followed by the existing stem kernel
                    (lsq_stem_conv_pool, STEM_SPLIT = 22, for ImageNet; lsq_stem_conv_gen for the other two): the baseline;
  kernel_fp32       the existing stem kernel alone on a ready fp32 batch (the kernel-to-kernel ratio);
  u8_nchw, u8_cl    lsq_stem_conv_u8 on the NCHW / channels-last bytes.

Every figure is the time of one replay of a captured HIP graph of ``calls`` calls divided by ``calls``; the variants are
interleaved over ``rounds`` rounds and reported as median and (min, max).  Writes profiles/stem_u8.json.

    python scripts/stem_u8_bench.py [--rounds 15] [--out profiles/stem_u8.json]
"""

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ml-quant_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from quant import _hip                          # noqa: E402

DEV = 'cuda:0'


def capture(fn, calls):
    """A HIP graph of ``calls`` runs of ``fn`` (warmed up on a side stream first) and the last output."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            out = fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        for _ in range(calls):
            out = fn()
    return graph, out


def replay_us(graph, calls, replays=5):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(replays):
        graph.replay()
    e.record()
    torch.cuda.synchronize()
    return 1e3 * s.elapsed_time(e) / (replays * calls)


def compare(variants, calls, rounds):
    """variants = {name: fn}.  Per-call medians and spreads in microseconds, and the largest difference between the output of
    the first variant and each other one."""
    graphs, outs = {}, {}
    for name, fn in variants.items():
        graphs[name], outs[name] = capture(fn, calls)
    times = {name: [] for name in variants}
    for name in variants:
        replay_us(graphs[name], calls)                                          # (warm)
    for _ in range(rounds):
        for name in variants:
            times[name].append(replay_us(graphs[name], calls))
    first = next(iter(variants))
    row = {name: {'median_us': statistics.median(t), 'min_us': min(t), 'max_us': max(t)} for name, t in times.items()}
    for name in variants:
        if name != first:
            row[name]['max_abs_diff_to_' + first] = float((outs[name] - outs[first]).abs().max())
    return row


def shape_row(n, c, hw, o, k, stride, pad, pool, mean, std, calls, rounds):
    torch.manual_seed(0)
    x = torch.randint(0, 256, (n, c, hw, hw), dtype=torch.uint8, device=DEV)
    xcl = x.contiguous(memory_format=torch.channels_last)
    w = torch.randn(o, c, k, k, device=DEV) * (c * k * k) ** -0.5
    b = torch.randn(o, device=DEV) * 0.1
    mean, std = torch.tensor(mean, device=DEV).view(1, -1, 1, 1), torch.tensor(std, device=DEV).view(1, -1, 1, 1)
    in_scale, in_shift = (1 / (255 * std)).flatten().contiguous(), (-mean / std).flatten().contiguous()
    post = None if pool != 2 else (torch.rand(o, device=DEV) + 0.5, torch.randn(o, device=DEV) * 0.1)
    norm = lambda t: t.float().div(255).sub(mean).div(std).contiguous()         # noqa: E731
    if pool == 3:
        old = lambda t: _hip.stem_conv_pool(t, w, b, 22)                         # noqa: E731
    else:
        old = lambda t: _hip.stem_conv_gen(t, w, b, stride, pad, True, post, pool)      # noqa: E731
    ready = norm(x)
    new = lambda t: _hip.stem_conv_u8(t, w, b, in_scale, in_shift, stride, pad, True, post, pool)     # noqa: E731
    return compare({'norm+kernel': lambda: old(norm(x)), 'norm+kernel_cl': lambda: old(norm(xcl)), 'kernel_fp32': lambda: old(ready),
                    'u8_nchw': lambda: new(x), 'u8_cl': lambda: new(xcl)}, calls, rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stem_u8.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    result = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'per_call': {}}
    imagenet = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    result['per_call']['imagenet_stem_n256'] = shape_row(256, 3, 224, 64, 7, 2, 3, 3, *imagenet, 5, args.rounds)
    result['per_call']['imagenet_stem_n64'] = shape_row(64, 3, 224, 64, 7, 2, 3, 3, *imagenet, 5, args.rounds)
    result['per_call']['cifar_stem_n100'] = shape_row(100, 3, 32, 64, 3, 1, 1, 1, *imagenet, 20, args.rounds)
    result['per_call']['lenet_front_n64'] = shape_row(64, 1, 28, 20, 5, 1, 0, 2, [0.1307], [0.3081], 20, args.rounds)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
