#!/usr/bin/env python3
"""Measurement of QuantLinear's 16-bit train step (lsq_linear_signw_dgrad_half, quant.binary.hip_train_linear with
``QuantLinear.hip_train_half``), one JSON document written to --out and printed.

  python scripts/linear_train_half_bench.py [--rounds R] [--only NAMES] [--skip-steps] [--out profiles/linear_train_half.json]

shapes  LeNet's fc1 (batch 64, 800 -> 500), the ResNet-18 head (batch 256, 512 -> 1000) and the MLP shapes 512 x 4096 -> 4096
        and 8192 x 4096 -> 4096, bf16 and fp16, ls-1 and ls-2 weights, ls-2 activations.
kernel  microseconds of one lsq_linear_signw_dgrad_half call with the straight-through epilogue (16-bit grad_y and x in, 16-bit
        grad_x out, the transpose of the planes into the workspace included) against the five launches over fp32 copies that
        give the same bits: gy.float(), lsq_linear_signw_dgrad, x.float(), lsq_ste_backward, .to(dtype).  The method is
        conv_dgrad_bench.py's: HIP-graph replays of `chain` back-to-back calls divided by `chain`, both routes alternating in one
        process, every variant warmed up; the median over the rounds with its spread (max - min over median).  That the two
        routes give the same bits is checked on every shape before it is timed.
step    milliseconds of the layer's whole train step (forward, backward of a sum-of-squares loss, no optimizer): the 16-bit
        input under torch.autocast with ``hip_train_half`` on, the same with the switch off (the torch formulation), and the
        fp32 step (``hip_train``, no autocast) on the same values; device events around `--steps` steps after a warm-up, the
        routes alternating over the rounds, and torch.cuda.max_memory_allocated of each."""
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
# (name, rows M, F, O)
SHAPES = [('lenet_fc1', 64, 800, 500), ('resnet_head', 256, 512, 1000), ('mlp_512', 512, 4096, 4096),
          ('mlp_8192', 8192, 4096, 4096)]
WEIGHTS = ('ls-1', 'ls-2')
SYM = {'kind': 'symmetric', 'alpha': 2}


def make_layer(ws, f, o):
    from quant.binary.binary_linear import QuantLinear
    lin = QuantLinear('ls-2', ws, f, o, dict(SYM), bias=True)
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(lin.weight.shape, generator=gen) * f ** -0.5)
    return lin.to(DEV).train()


def kernel_part(shape, ws, dtype, rounds):
    from quant import _hip
    name, m, f, o = shape
    lin = make_layer(ws, f, o)
    weight = lin.weight.detach()
    with torch.no_grad():
        lin.w_approximate(weight.view(o, f, 1, 1))
        wsc = lin.w_approximate.plane_scales().to(torch.float32).contiguous()
    wgeom = _hip.make_geom(1, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    wbits, _ = _hip.pack_weight(weight.view(o, f, 1, 1), wgeom, wsc)
    gen = torch.Generator().manual_seed(11)
    gy = (torch.randn((m, o), generator=gen) * 1e-3).to(dtype).to(DEV)
    x = (torch.randn((m, f), generator=gen) * 1.2).to(dtype).to(DEV)
    alpha = lin._alpha_in(dtype)
    geom = _hip.make_geom(m, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    planes = torch.zeros((2 * _hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xsc = torch.empty((2, m), dtype=torch.float32, device=DEV)
    _hip.act_quant_half(x.view(m, f, 1, 1), geom, _hip.SCHEME_LS2, 2, 3, alpha, planes, xsc)
    del planes

    variants = {'kernel': lambda: _hip.linear_signw_dgrad_half(gy, wbits, wsc, m, f, o, x, xsc, alpha),
                'composition': lambda: _hip.ste_backward(x.float(), _hip.linear_signw_dgrad(gy.float(), wbits, wsc, m, f, o),
                                                         xsc, alpha).to(dtype)}
    a, b = variants['kernel'](), variants['composition']()
    torch.cuda.synchronize()
    out = {'M': m, 'F': f, 'O': o, 'weight_planes': int(wsc.shape[0]),
           'same_bits': bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))}
    assert out['same_bits'], name
    del a, b
    chain = 3
    samples = {v: [] for v in variants}
    for _ in range(rounds):
        for v, fn in variants.items():
            samples[v].append(graph_time(fn, 5, chain))
    out['us'] = {v: statistics.median(t) for v, t in samples.items()}
    out['spread'] = {v: (max(t) - min(t)) / statistics.median(t) for v, t in samples.items()}
    out['composition_over_kernel'] = out['us']['composition'] / out['us']['kernel']
    # bytes the one-pass kernel has to move: gy in, x in, grad_x out, 2 bytes each
    out['kernel_min_bytes'] = 2 * (gy.numel() + 2 * x.numel())
    out['kernel_gb_per_s_of_min_bytes'] = out['kernel_min_bytes'] / (out['us']['kernel'] * 1e-6) / 1e9
    out['graph_chain'] = chain
    return out


def step_part(shape, ws, dtype, rounds, steps, warmup):
    name, m, f, o = shape
    gen = torch.Generator().manual_seed(13)
    x16 = (torch.randn((m, f), generator=gen) * 1.2).to(dtype).to(DEV)
    routes = {'half_step': (True, False, x16, True), 'torch_formulation': (False, False, x16, True),
              'fp32_step': (False, True, x16.float(), False)}
    layers = {r: make_layer(ws, f, o) for r in routes}
    taken = {}

    def one(route):
        half, fp32, xin, autocast = routes[route]
        lin = layers[route]
        lin.hip_train_half, lin.hip_train = half, fp32
        x = xin.detach().requires_grad_()
        lin.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype, enabled=autocast):
            y = lin(x)
        taken[route] = type(y.grad_fn).__name__
        y.float().square().sum().backward()

    def timed(route):
        for _ in range(warmup):
            one(route)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(steps):
            one(route)
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / steps, torch.cuda.max_memory_allocated(DEV) / 2 ** 20

    samples, mem = {r: [] for r in routes}, {}
    for _ in range(rounds):
        for r in routes:
            ms, mem[r] = timed(r)
            samples[r].append(ms)
    assert taken['half_step'] == '_QuantLinearStepHalfBackward' and taken['fp32_step'] == '_QuantLinearStepBackward', taken
    assert not taken['torch_formulation'].startswith('_QuantLinearStep'), taken
    ms = {r: statistics.median(t) for r, t in samples.items()}
    return {'M': m, 'F': f, 'O': o, 'ms': ms, 'spread': {r: (max(t) - min(t)) / statistics.median(t) for r, t in samples.items()},
            'max_memory_allocated_mib': mem, 'steps': steps, 'warmup': warmup,
            'torch_formulation_over_half': ms['torch_formulation'] / ms['half_step'],
            'fp32_over_half': ms['fp32_step'] / ms['half_step']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--skip-steps', action='store_true', help='kernel times only')
    ap.add_argument('--skip-kernels', action='store_true', help='train steps only')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linear_train_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'linear_train_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'what': 'linear_train_half', 'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'activations': 'ls-2',
           'kernel': {}, 'train_step': {}}
    for tname, dtype in DTYPES.items():
        for ws in WEIGHTS:
            for shape in SHAPES:
                if only and shape[0] not in only:
                    continue
                key = f'{tname}/{ws}/{shape[0]}'
                if not args.skip_kernels:
                    res['kernel'][key] = kernel_part(shape, ws, dtype, args.rounds)
                    print('kernel', key, json.dumps(res['kernel'][key]), flush=True)
                if not args.skip_steps:
                    res['train_step'][key] = step_part(shape, ws, dtype, args.rounds, args.steps, args.warmup)
                    print('step', key, json.dumps(res['train_step'][key]), flush=True)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
