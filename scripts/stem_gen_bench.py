"""lsq_stem_conv_gen against the route the same operands take with ``resnet.STEM_GENERAL`` off, on the GPU.

Per call: the CIFAR stem (batch 100, 256), LeNet's front (batch 64, 256) and, to place the kernel against
lsq_stem_conv_pool's ground, 3 -> 64 channels 7x7 / 2 at 224 x 224 without a pool (the model gate never sends that shape
to the new kernel).  Per graph replay: the cifar100_ls1_kd network at batch 100 and LeNet at batch 64, switch off and on.

Every figure is the time of one replay of a captured HIP graph of ``calls`` forwards divided by ``calls``; the variants are
interleaved (off, on, off, on, ...) over ``rounds`` rounds and reported as median and (min, max).  Writes
profiles/stem_gen.json.

    python scripts/stem_gen_bench.py [--rounds 15] [--out profiles/stem_gen.json]
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

import bench                                    # noqa: E402
from quant import _hip                          # noqa: E402
from quant.models import resnet                 # noqa: E402

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
    """variants = {name: fn}; fn is captured with the switch the name's suffix asks for.  Returns the per-call medians and
    spreads in microseconds and the largest difference between the outputs of the first variant and each other one."""
    graphs, outs = {}, {}
    before = resnet.STEM_GENERAL
    try:
        for name, (switch, fn) in variants.items():
            resnet.STEM_GENERAL = switch
            graphs[name], outs[name] = capture(fn, calls)
    finally:
        resnet.STEM_GENERAL = before
    times = {name: [] for name in variants}
    for name in variants:
        replay_us(graphs[name], calls)                                          # (warm)
    for _ in range(rounds):
        for name in variants:
            times[name].append(replay_us(graphs[name], calls))
    first = next(iter(variants))
    row = {name: {'median_us': statistics.median(t), 'min_us': min(t), 'max_us': max(t)} for name, t in times.items()}
    for name in variants:
        if name != first and outs[name].shape == outs[first].shape:
            row[name]['max_abs_diff_to_' + first] = float((outs[name] - outs[first]).abs().max())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stem_gen.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    result = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'per_call': {}, 'per_replay': {}}

    cifar = bench.build_model(bench.cifar_arch(), DEV)
    lenet = bench.build_lenet(DEV)
    stem = cifar.blocks[0]
    for n in (100, 256):
        x = torch.randn(n, 3, 32, 32, device=DEV)
        result['per_call'][f'cifar_stem_n{n}'] = compare({'off': (False, lambda: stem(x)), 'on': (True, lambda: stem(x))}, 20, args.rounds)
    for n in (64, 256):
        x = torch.randn(n, 1, 28, 28, device=DEV)
        result['per_call'][f'lenet_front_n{n}'] = compare({'off': (False, lambda: lenet._front(x)), 'on': (True, lambda: lenet._front(x))},
                                                          20, args.rounds)
    # 7x7 / 2 at 224 x 224 without a pool, called directly; lsq_stem_conv_pool (which also pools) is the ground beside it
    torch.manual_seed(0)
    big = resnet._Stem(torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False), torch.nn.BatchNorm2d(64), torch.nn.ReLU(),
                       torch.nn.Identity()).eval().to(DEV)
    x = torch.randn(64, 3, 224, 224, device=DEV)
    w, b = resnet._folded_conv_bn(big, big[0], big[1])
    result['per_call']['7x7_s2_224_n64_no_pool'] = compare({
        'off': (False, lambda: big(x)),
        'on': (False, lambda: _hip.stem_conv_gen(x, w, b, 2, 3, True)),
        'lsq_stem_conv_pool_split3_with_pool': (False, lambda: _hip.stem_conv_pool(x, w, b, 3))}, 5, args.rounds)

    x = torch.randn(100, 3, 32, 32, device=DEV)
    result['per_replay']['cifar100_ls1_kd_n100'] = compare({'off': (False, lambda: cifar(x)), 'on': (True, lambda: cifar(x))}, 1, args.rounds)
    x = torch.randn(64, 1, 28, 28, device=DEV)
    result['per_replay']['lenet_n64'] = compare({'off': (False, lambda: lenet(x)), 'on': (True, lambda: lenet(x))}, 1, args.rounds)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
