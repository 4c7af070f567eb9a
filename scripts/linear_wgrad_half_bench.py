#!/usr/bin/env python3
"""Measurement of QuantLinear's 16-bit weight gradient in one call (lsq_linear_signx_wgrad_half and the WGRAD_HALF_KERNEL flag
of quant.binary.hip_train_linear), one JSON document written to --out and printed.

  python scripts/linear_wgrad_half_bench.py [--rounds R] [--only NAMES] [--out profiles/linear_wgrad_half.json]

Shapes: those of scripts/linear_wgrad_bench.py -- LeNet fc1 (64 x 800 -> 500), the ResNet-18 head (256 x 512 -> 1000),
512 x 4096 -> 4096 and 8192 x 4096 -> 4096 --, each with ls-1 and ls-2 activations in bf16 and fp16, ls-1 weights, one row per
sample.
  kernel  microseconds of the new call with the weight (contract (B): sign image + GEMM + the weight's straight-through
          estimator in the epilogue = the step's grad_w) against each route it replaces, composed of the calls the 16-bit
          step makes without the switch:
            float_quant_values_mm_ste   gy.float() + x.float() + lsq_quant_values + torch.mm + lsq_ste_backward
            float_signx_wgrad_ste       gy.float() + x.float() + lsq_linear_signx_wgrad + lsq_ste_backward   (WGRAD_KERNEL)
          and, for orientation, torch.mm in the 16-bit type on a ready x_q (no casts, no quantizer, no estimator); the max
          error of the products against fp64 (the new call without the weight, contract (A), beside torch.mm in the type).
          HIP-graph replays of `chain` back-to-back calls divided by `chain`.
  step    forward + backward + SGD step of the module in train mode under torch.autocast with ``hip_train_half``, input
          gradient included, WGRAD_HALF_KERNEL True against False in one process, eager, host work included; peak memory of
          one step of each above what is allocated before it.
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

from linear_train_bench import CLAMP, DEV, SHAPES, eager_time, graph_time, module, summarize  # noqa: E402

X_SCHEMES = ('ls-1', 'ls-2')
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
ALPHA = float(CLAMP['alpha'])         # (exact in both types)
NEW = 'lsq_linear_signx_wgrad_half'


def kernel_part(m, f, o, xs_scheme, dtype, rounds):
    from quant import _hip
    from oracle import ref_port as P
    import linear_wgrad_cases as C
    gy = torch.randn((m, o), generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
    x_cpu = (torch.randn((m, f), generator=torch.Generator().manual_seed(3)) * 1.2).to(dtype)
    xs = C.oracle_scales(x_cpu.float(), m, xs_scheme, ALPHA).to(DEV)
    x = x_cpu.to(DEV)
    w_cpu = torch.randn((o, f), generator=torch.Generator().manual_seed(2)) * 0.05
    wsc = torch.stack(list(P.weight_scales(w_cpu.view(o, f, 1, 1), 'ls-1'))).float().view(1, o).contiguous().to(DEV)
    w = w_cpu.to(DEV)
    kx = xs.shape[0]
    xq = _hip.quant_values(x.float(), xs, ALPHA)
    xq16 = xq.to(dtype)

    def new():
        return _hip.linear_signx_wgrad_half(gy, x, xs, ALPHA, m, 1, f, o, w, wsc)

    def replaced_mm():
        gy32, x32 = gy.float(), x.float()
        return _hip.ste_backward(w, torch.mm(gy32.t(), _hip.quant_values(x32, xs, ALPHA)), wsc, -1.0)

    def replaced_kernel():
        gy32, x32 = gy.float(), x.float()
        return _hip.ste_backward(w, _hip.linear_signx_wgrad(gy32, x32, xs, ALPHA, m, 1, f, o), wsc, -1.0)

    variants = {NEW: new, 'float_quant_values_mm_ste': replaced_mm, 'float_signx_wgrad_ste': replaced_kernel,
                'torch_mm_16bit_alone': lambda: torch.mm(gy.t(), xq16)}
    same = {k: bool(torch.equal(new().view(torch.int32), fn().view(torch.int32))) for k, fn in
            (('float_signx_wgrad_ste', replaced_kernel),)}
    ref = gy.double().t() @ xq.double()
    scale = ref.abs().max().item()
    products = {NEW + '_without_weight': _hip.linear_signx_wgrad_half(gy, x, xs, ALPHA, m, 1, f, o),
                'torch_mm_16bit_alone': torch.mm(gy.t(), xq16).float(), 'torch_mm_fp32': torch.mm(gy.float().t(), xq)}
    torch.cuda.synchronize()
    out = {'activation_planes': kx, 'same_bits_as': same,
           'max_rel_err_vs_fp64': {k: (v.double() - ref).abs().max().item() / scale for k, v in products.items()}}
    del ref, products
    chain = 200 if m * f * o < 1 << 30 else 10
    for fn in variants.values():
        graph_time(fn, 1, chain)
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(graph_time(fn, 5, chain))
    out['us'], out['spread'] = summarize(samples)
    out['graph_chain'] = chain
    us = out['us']
    out['ratio'] = {k + '_over_new': v / us[NEW] for k, v in us.items() if k != NEW}
    return out


def step_part(m, f, o, xs_scheme, dtype, rounds):
    import quant.binary.hip_train_linear as HTL
    x = (torch.randn((m, f), generator=torch.Generator().manual_seed(1)) * 1.2).to(dtype).to(DEV).requires_grad_()
    gy = torch.randn((m, o), generator=torch.Generator().manual_seed(4)).to(dtype).to(DEV)
    lin = module(xs_scheme, 'ls-1', f, o, False)
    lin.hip_train_half = True
    opt = torch.optim.SGD(lin.parameters(), lr=1e-3)

    def step(flag):
        def run():
            HTL.WGRAD_HALF_KERNEL = flag
            opt.zero_grad(set_to_none=True)
            x.grad = None
            with torch.autocast('cuda', dtype):
                y = lin(x)
            y.backward(gy)
            opt.step()
        return run

    steps = {'wgrad_half_kernel': step(True), 'fp32_copies_torch_mm': step(False)}
    try:
        assert HTL.supported(lin, x), 'the 16-bit step does not take this layer'
        inner = 20 if m * f * o < 1 << 30 else 5
        for fn in steps.values():
            eager_time(fn, 1, inner)
        samples = {k: [] for k in steps}
        for _ in range(rounds):
            for k, fn in steps.items():
                samples[k].append(eager_time(fn, 5, inner))
        out = {}
        out['us'], out['spread'] = summarize(samples)
        out['off_over_on'] = out['us']['fp32_copies_torch_mm'] / out['us']['wgrad_half_kernel']
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
        HTL.WGRAD_HALF_KERNEL = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linear_wgrad_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'linear_wgrad_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'shapes': {}}
    for name, m, f, o in SHAPES:
        if only and name not in only:
            continue
        entry = {'M': m, 'F': f, 'O': o, 'kernel': {}, 'step': {}}
        for xs in X_SCHEMES:
            for dname, dtype in DTYPES.items():
                entry['kernel'][f'{xs}/{dname}'] = kernel_part(m, f, o, xs, dtype, args.rounds)
                entry['step'][f'{xs}/ls-1/{dname}'] = step_part(m, f, o, xs, dtype, args.rounds)
        res['shapes'][name] = entry
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
