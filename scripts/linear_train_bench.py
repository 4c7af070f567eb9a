#!/usr/bin/env python3
"""Measurement of the QuantLinear train step on the kernels (lsq_linear_signw_dgrad and quant.binary.hip_train_linear), one
JSON document written to --out and printed.

  python scripts/linear_train_bench.py [--rounds R] [--only NAMES] [--out profiles/linear_train.json]

Shapes: LeNet fc1 (64 x 800 -> 500), the ResNet-18 head (256 x 512 -> 1000), 512 x 4096 -> 4096 and 8192 x 4096 -> 4096, each
with ls-1 and ls-2 weights.
  kernel  microseconds of lsq_linear_signw_dgrad (the transpose of the planes into the workspace is part of the call)
          against torch.mm(gy, w_q) in fp32 and in bf16 on the dequantized weights, and -- the yardstick -- lsq_linear_signw,
          the forward kernel, at the same shape (the same number of MFMAs); the max error of each route against fp64; the
          share of the bf16 peak (hi and lo pass of every plane) or of HBM, whichever bounds the shape.  (How the call
          divides between its transpose and its GEMM kernel is a kernel trace's to say: DESIGN 4.12.)  HIP-graph replays of `chain` back-to-back
          calls divided by `chain`.
  step    forward + backward + SGD step of the module in train mode, input gradient included, ``hip_train`` True against
          False (False is the torch formulation) for fp and ls-2 activations, eager, host work included; the per-phase
          split of the kernel step from ``_hip.enable_timing``, with the parts it does not bracket timed on their own as
          graphs (torch's fp32 weight-gradient GEMM, the weight quantizer's torch ops, lsq_pack_weight); peak memory of one
          step of each above what is allocated before it.
Every variant is warmed up, then timed once per round with the variants alternating; the median over the rounds is
reported with its spread (max - min over median)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden')]
import torch  # noqa: E402

PEAK_BF16 = 2.5e15       # dense bf16 MFMA FLOP/s of the MI355X
HBM = 8e12               # bytes per second
DEV = 'cuda:0'
CLAMP = {'kind': 'symmetric', 'alpha': 2}
SHAPES = [('lenet_fc1', 64, 800, 500), ('resnet18_head', 256, 512, 1000), ('mlp_m512', 512, 4096, 4096),
          ('mlp_m8192', 8192, 4096, 4096)]
W_SCHEMES = ('ls-1', 'ls-2')
X_SCHEMES = ('fp', 'ls-2')


def graph_time(fn, reps, chain):
    """median us per call of `chain` calls captured in one graph and replayed `reps` times."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
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
    return statistics.median(ts)


def eager_time(fn, reps, inner):
    """median us per call of `inner` eager calls (host work included)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(ts)


def summarize(samples):
    return ({k: statistics.median(v) for k, v in samples.items()},
            {k: (max(v) - min(v)) / statistics.median(v) for k, v in samples.items()})


def module(xs, ws, f, o, hip_train, seed=2):
    from quant.binary import QuantLinear
    g = torch.Generator().manual_seed(seed)
    lin = QuantLinear(xs, ws, f, o, CLAMP)
    with torch.no_grad():
        lin.weight.copy_(torch.randn((o, f), generator=g) * 0.05)
        lin.bias.copy_(torch.randn((o,), generator=g) * 0.1)
    lin.hip_train = hip_train
    return lin.to(DEV).train()


def kernel_part(m, f, o, ws, rounds):
    from quant import _hip
    from oracle import ref_port as P
    lin = module('fp', ws, f, o, False)
    w = lin.weight.detach()
    with torch.no_grad():
        sc = P.weight_scales(w.cpu().view(o, f, 1, 1), ws)
        wq = P.quantize_weight(w.cpu().view(o, f, 1, 1), ws, sc).view(o, f).to(DEV)
    wsc = torch.stack([sc[0], sc[0]] if ws == 'ls-T' else list(sc)).contiguous().to(DEV)
    kw = wsc.shape[0]
    geom = _hip.make_geom(1, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    wbits, _ = _hip.pack_weight(w.view(o, f, 1, 1), geom, wsc)
    gy = torch.randn((m, o), generator=torch.Generator().manual_seed(1)).to(DEV)
    x = torch.randn((m, f), generator=torch.Generator().manual_seed(3)).to(DEV)
    gy16, wq16 = gy.bfloat16(), wq.bfloat16()

    def dgrad():
        return _hip.linear_signw_dgrad(gy, wbits, wsc, m, f, o)

    variants = {'lsq_linear_signw_dgrad': dgrad,
                'torch_mm_fp32': lambda: torch.mm(gy, wq), 'torch_mm_bf16': lambda: torch.mm(gy16, wq16),
                'lsq_linear_signw_forward': lambda: _hip.linear_signw(x, -1.0, wbits, wsc, None, m, f, o)}
    ref = gy.double() @ wq.double()
    scale = ref.abs().max().item()
    outs = {'lsq_linear_signw_dgrad': dgrad(), 'torch_mm_fp32': torch.mm(gy, wq), 'torch_mm_bf16': torch.mm(gy16, wq16)}
    torch.cuda.synchronize()
    out = {'weight_planes': kw, 'max_rel_err_vs_fp64': {k: (v.double() - ref).abs().max().item() / scale for k, v in outs.items()}}
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
    flops = 2.0 * 2.0 * m * f * o * kw                       # hi and lo pass of every plane
    words = kw * ((f + 63) // 64) * ((o + 15) // 16 * 16) + 2 * kw * ((o + 63) // 64) * ((f + 15) // 16 * 16)
    nbytes = 4.0 * m * o + 8.0 * words + 4.0 * m * f         # gy once, planes read + image written and read, gx written
    t = out['us']['lsq_linear_signw_dgrad'] * 1e-6
    t_mfma, t_hbm = flops / PEAK_BF16, nbytes / HBM
    out['bf16_flops'], out['bytes'] = flops, nbytes
    out['bound'] = 'bf16 peak' if t_mfma >= t_hbm else 'HBM'
    out['peak_share'] = max(t_mfma, t_hbm) / t
    us = out['us']
    out['ratio'] = {'torch_mm_fp32_over_dgrad': us['torch_mm_fp32'] / us['lsq_linear_signw_dgrad'],
                    'torch_mm_bf16_over_dgrad': us['torch_mm_bf16'] / us['lsq_linear_signw_dgrad'],
                    'dgrad_over_forward_kernel': us['lsq_linear_signw_dgrad'] / us['lsq_linear_signw_forward']}
    return out


def step_part(m, f, o, ws, xs, rounds):
    from quant import _hip
    x = (torch.randn((m, f), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV).requires_grad_()
    gy = torch.randn((m, o), generator=torch.Generator().manual_seed(4)).to(DEV)
    mods = {'hip_train': module(xs, ws, f, o, True), 'torch': module(xs, ws, f, o, False)}
    opts = {k: torch.optim.SGD(v.parameters(), lr=1e-3) for k, v in mods.items()}

    def step(k):
        def run():
            opts[k].zero_grad(set_to_none=True)
            x.grad = None
            y = mods[k](x)
            y.backward(gy)
            opts[k].step()
        return run

    steps = {k: step(k) for k in mods}
    y = mods['hip_train'](x)
    assert type(y.grad_fn).__name__ == '_QuantLinearStepBackward'
    del y
    inner = 20 if m * f * o < 1 << 30 else 5
    for fn in steps.values():
        eager_time(fn, 1, inner)
    samples = {k: [] for k in steps}
    for _ in range(rounds):
        for k, fn in steps.items():
            samples[k].append(eager_time(fn, 5, inner))
    out = {}
    out['us'], out['spread'] = summarize(samples)
    out['torch_over_hip_train'] = out['us']['torch'] / out['us']['hip_train']
    # peak memory of one step above what is allocated before it
    out['peak_step_bytes'] = {}
    for k, fn in steps.items():
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        out['peak_step_bytes'][k] = torch.cuda.max_memory_allocated() - base
    # per-phase split of the kernel step
    n = 10
    _hip.enable_timing(True)
    for _ in range(n):
        steps['hip_train']()
    torch.cuda.synchronize()
    rec = _hip.drain_timing()
    _hip.enable_timing(False)
    out['phase_us'] = {name: v[1] * 1e3 / n for name, v in rec.items()}
    out['phase_launches_per_step'] = {name: v[0] / n for name, v in rec.items()}
    # what the event pairs above do not bracket: torch's share of the step, and the weight packing, each as a graph
    chain = 200 if m * f * o < 1 << 30 else 10
    xq = x.detach().clamp(-2, 2)
    lin = mods['hip_train']
    w4 = lin.weight.detach().view(o, f, 1, 1)
    wsc = lin.w_approximate.plane_scales().float().contiguous()
    geom = _hip.make_geom(1, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    with torch.no_grad():
        out['phase_us']['torch_mm_weight_gradient'] = graph_time(lambda: torch.mm(gy.t(), xq), 5, chain)
        out['phase_us']['torch_weight_quantizer'] = graph_time(lambda: lin.w_approximate(w4), 5, min(chain, 20))
        out['phase_us']['lsq_pack_weight'] = graph_time(lambda: _hip.pack_weight(w4, geom, wsc), 5, min(chain, 20))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linear_train.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'linear_train_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'peak_bf16_flops': PEAK_BF16, 'hbm_bytes_per_s': HBM,
           'rounds': args.rounds, 'shapes': {}}
    for name, m, f, o in SHAPES:
        if only and name not in only:
            continue
        entry = {'M': m, 'F': f, 'O': o, 'kernel': {}, 'step': {}}
        for ws in W_SCHEMES:
            entry['kernel'][ws] = kernel_part(m, f, o, ws, args.rounds)
            for xs in X_SCHEMES:
                entry['step'][f'{xs}/{ws}'] = step_part(m, f, o, ws, xs, args.rounds)
        res['shapes'][name] = entry
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
