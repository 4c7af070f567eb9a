#!/usr/bin/env python3
"""Measurement of QuantLinear's weight gradient on the kernel (lsq_linear_signx_wgrad and the WGRAD_KERNEL flag of
quant.binary.hip_train_linear), one JSON document written to --out and printed.

  python scripts/linear_wgrad_bench.py [--rounds R] [--only NAMES] [--out profiles/linear_wgrad.json]

Shapes: LeNet fc1 (64 x 800 -> 500), the ResNet-18 head (256 x 512 -> 1000), 512 x 4096 -> 4096 and 8192 x 4096 -> 4096 (the
table of DESIGN 4.12), each with ls-1 and ls-2 activations, one row per sample.
  kernel  microseconds of lsq_linear_signx_wgrad (the sign image written into the workspace is part of the call) against
          what it replaces -- lsq_quant_values + torch.mm(gy^T, x_q) in fp32 --, torch.mm in bf16 on a ready x_q for
          orientation, and lsq_train_wgrad at the 1 x 1 geometry (N = M, C = F, H = W = 1; where C is a multiple of 64), the
          in-tree alternative; the max error of each route against fp64.  HIP-graph replays of `chain` back-to-back calls
          divided by `chain`.
  step    forward + backward + SGD step of the module in train mode with ``hip_train``, input gradient included,
          WGRAD_KERNEL True against False in one process, eager, host work included; peak memory of one step of each above
          what is allocated before it.
Every variant is warmed up, then timed once per round with the variants alternating; the median over the rounds is
reported with its spread (max - min over median)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden'),
                os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from linear_train_bench import CLAMP, DEV, PEAK_BF16, SHAPES, eager_time, graph_time, module, summarize  # noqa: E402

X_SCHEMES = ('ls-1', 'ls-2')
ALPHA = float(CLAMP['alpha'])


def kernel_part(m, f, o, xs_scheme, rounds):
    from quant import _hip
    import linear_wgrad_cases as C
    gy = torch.randn((m, o), generator=torch.Generator().manual_seed(1)).to(DEV)
    x_cpu = torch.randn((m, f), generator=torch.Generator().manual_seed(3)) * 1.2
    xs_cpu = C.oracle_scales(x_cpu, m, xs_scheme, ALPHA)
    x, xs = x_cpu.to(DEV), xs_cpu.to(DEV)
    kx = xs.shape[0]
    xq = _hip.quant_values(x, xs, ALPHA)
    xq16, gy16 = xq.bfloat16(), gy.bfloat16()

    def kernel():
        return _hip.linear_signx_wgrad(gy, x, xs, ALPHA, m, 1, f, o)

    def replaced():
        return torch.mm(gy.t(), _hip.quant_values(x, xs, ALPHA))

    variants = {'lsq_linear_signx_wgrad': kernel, 'quant_values_plus_torch_mm_fp32': replaced,
                'torch_mm_fp32_alone': lambda: torch.mm(gy.t(), xq), 'torch_mm_bf16_alone': lambda: torch.mm(gy16.t(), xq16)}
    outs = {'lsq_linear_signx_wgrad': kernel(), 'quant_values_plus_torch_mm_fp32': replaced(),
            'torch_mm_bf16_alone': torch.mm(gy16.t(), xq16)}
    if f % 64 == 0:                                   # lsq_train_wgrad reads the forward's planes: C a multiple of 64
        geom = _hip.make_geom(m, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
        planes = torch.zeros((kx * _hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
        scales = torch.empty((kx, m), dtype=torch.float32, device=DEV)
        _hip.act_quant(x.view(m, f, 1, 1), geom, _hip.SCHEME_LS1 if kx == 1 else _hip.SCHEME_LS2, kx, 3, ALPHA, planes, scales, xs)
        gy4 = gy.view(m, o, 1, 1)

        def conv_wgrad():
            return _hip.wgrad(planes, kx, xs, gy4, geom)

        try:
            outs['lsq_train_wgrad_1x1'] = conv_wgrad().view(o, f)
            variants['lsq_train_wgrad_1x1'] = conv_wgrad
        except Exception as e:                        # a geometry the convolution's kernel does not take: say so
            print(f'lsq_train_wgrad_1x1 not measured at {m} x {f} -> {o}: {e}', flush=True)
    ref = gy.double().t() @ xq.double()
    scale = ref.abs().max().item()
    torch.cuda.synchronize()
    out = {'activation_planes': kx,
           'max_rel_err_vs_fp64': {k: (v.double() - ref).abs().max().item() / scale for k, v in outs.items()}}
    del ref, outs
    chain = 200 if m * f * o < 1 << 30 else 10
    for fn in variants.values():
        graph_time(fn, 1, chain)
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(graph_time(fn, 5, chain))
    out['us'], out['spread'] = summarize(samples)
    out['graph_chain'] = chain
    flops = 2.0 * 2.0 * m * f * o * kx                       # hi and lo pass of every plane
    out['bf16_flops'] = flops
    us = out['us']
    out['bf16_peak_share'] = flops / PEAK_BF16 / (us['lsq_linear_signx_wgrad'] * 1e-6)
    out['ratio'] = {k + '_over_kernel': v / us['lsq_linear_signx_wgrad'] for k, v in us.items() if k != 'lsq_linear_signx_wgrad'}
    return out


def step_part(m, f, o, xs_scheme, rounds):
    import quant.binary.hip_train_linear as HTL
    x = (torch.randn((m, f), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV).requires_grad_()
    gy = torch.randn((m, o), generator=torch.Generator().manual_seed(4)).to(DEV)
    lin = module(xs_scheme, 'ls-1', f, o, True)
    opt = torch.optim.SGD(lin.parameters(), lr=1e-3)

    def step(flag):
        def run():
            HTL.WGRAD_KERNEL = flag
            opt.zero_grad(set_to_none=True)
            x.grad = None
            y = lin(x)
            y.backward(gy)
            opt.step()
        return run

    steps = {'wgrad_kernel': step(True), 'quant_values_torch_mm': step(False)}
    try:
        inner = 20 if m * f * o < 1 << 30 else 5
        for fn in steps.values():
            eager_time(fn, 1, inner)
        samples = {k: [] for k in steps}
        for _ in range(rounds):
            for k, fn in steps.items():
                samples[k].append(eager_time(fn, 5, inner))
        out = {}
        out['us'], out['spread'] = summarize(samples)
        out['torch_mm_over_wgrad_kernel'] = out['us']['quant_values_torch_mm'] / out['us']['wgrad_kernel']
        out['peak_step_bytes'] = {}
        for k, fn in steps.items():
            fn()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            out['peak_step_bytes'][k] = torch.cuda.max_memory_allocated() - base
    finally:
        HTL.WGRAD_KERNEL = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linear_wgrad.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'linear_wgrad_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'peak_bf16_flops': PEAK_BF16, 'rounds': args.rounds, 'shapes': {}}
    for name, m, f, o in SHAPES:
        if only and name not in only:
            continue
        entry = {'M': m, 'F': f, 'O': o, 'kernel': {}, 'step': {}}
        for xs in X_SCHEMES:
            entry['kernel'][xs] = kernel_part(m, f, o, xs, args.rounds)
            entry['step'][f'{xs}/ls-1'] = step_part(m, f, o, xs, args.rounds)
        res['shapes'][name] = entry
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
