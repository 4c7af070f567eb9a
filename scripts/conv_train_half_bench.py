#!/usr/bin/env python3
"""Measurement of QuantConv2d's 16-bit train step (lsq_signw_conv2d_dgrad_half, quant.binary.hip_train with
``QuantConv2d.hip_train_half``), one JSON document written to --out and printed.

  python scripts/conv_train_half_bench.py [--rounds R] [--batch B] [--only NAMES] [--skip-steps] [--out profiles/conv_train_half.json]

layers  the ten layer shapes of scripts/conv_dgrad_bench.py (the 16 quantized 3 x 3 layers and the three 1 x 1 stride-2
        projections of ResNet-18) at batch B, bf16 and fp16, ls-1 weights and ls-2 activations: microseconds of
          kernel       one lsq_signw_conv2d_dgrad_half call with the straight-through epilogue: 16-bit grad_y and x in, 16-bit
                       grad_x out, the transpose of the planes into the workspace included, against
          composition  the four launches over fp32 copies that give the same bits: gy.float(), lsq_signw_conv2d_dgrad,
                       lsq_ste_backward on x.float() (the cast is a fifth launch), .to(dtype).
        The method is conv_dgrad_bench.py's: HIP-graph replays of `chain` back-to-back calls divided by `chain`, both routes
        alternating in one process, every variant warmed up; the median over the rounds with its spread (max - min over
        median).  That the two routes give the same bits is checked on every shape before it is timed.
steps   the whole train step of ResNet-18 (ls-1 weights / ls-2 activations, bench.py's arch_config) at batch B under
        torch.autocast('cuda', torch.bfloat16) with ``hip_train_half`` True and False -- False is the torch formulation for
        every layer that is handed a 16-bit tensor, measured over --torch-steps steps only --, the number of the quantized
        layers that took the 16-bit step, torch.cuda.max_memory_allocated of each, and scripts/train_step.py's fp32 step
        (no autocast) in the same process."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from conv_dgrad_bench import SHAPES, graph_time  # noqa: E402

DEV = 'cuda:0'
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}


def layer_part(batch, shape, dtype, rounds, decompose=False):
    from quant import _hip
    from quant.binary.binary_conv import QuantConv2d
    name, c, o, h, k, s, p, count = shape
    conv = QuantConv2d('ls-2', 'ls-1', c, o, k, {'kind': 'symmetric', 'alpha': 2}, stride=s, padding=p, bias=False)
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
    gy = (torch.randn((batch, o, ho, wo), generator=gen) * 1e-3).to(dtype).to(DEV)
    x = (torch.randn((batch, c, h, h), generator=gen) * 1.2).to(dtype).to(DEV)
    alpha = conv._alpha_in(dtype)
    planes = torch.zeros((2 * _hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xsc = torch.empty((2, batch), dtype=torch.float32, device=DEV)
    _hip.act_quant_half(x, geom, _hip.SCHEME_LS2, 2, 3, alpha, planes, xsc)
    del planes

    variants = {'kernel': lambda: _hip.signw_conv2d_dgrad_half(gy, wbits, wsc, geom, x, xsc, alpha),
                'composition': lambda: _hip.ste_backward(x.float(), _hip.signw_conv2d_dgrad(gy.float(), wbits, wsc, geom),
                                                         xsc, alpha).to(dtype)}
    a, b = variants['kernel'](), variants['composition']()
    torch.cuda.synchronize()
    out = {'C': c, 'O': o, 'H': h, 'kernel_size': k, 'stride': s, 'layers': count,
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
    if decompose:
        # where the time goes: the fp32 kernel on a gradient cast beforehand, then the new kernel with only the 16-bit
        # gradient (fp32 out, no x), with 16-bit stores as well (no x), and whole (`kernel` above)
        gy32 = gy.float()
        parts = {'fp32_kernel_on_cast_gy': lambda: _hip.signw_conv2d_dgrad(gy32, wbits, wsc, geom),
                 'half_gy_only_fp32_out': lambda: _hip.signw_conv2d_dgrad_half(gy, wbits, wsc, geom, out_dtype=torch.float32),
                 'half_gy_and_16_bit_out': lambda: _hip.signw_conv2d_dgrad_half(gy, wbits, wsc, geom),
                 'cast_gy': lambda: gy.float(), 'cast_x': lambda: x.float()}
        x32, g32 = x.float(), torch.zeros(x.shape, dtype=torch.float32, device=DEV)
        parts['ste_backward_fp32'] = lambda: _hip.ste_backward(x32, g32, xsc, alpha)
        parts['round_to_type'] = lambda: g32.to(dtype)
        psamples = {v: [] for v in parts}
        for _ in range(rounds):
            for v, fn in parts.items():
                psamples[v].append(graph_time(fn, 5, chain))
        out['decomposition_us'] = {v: statistics.median(t) for v, t in psamples.items()}
    return out


def autocast_steps(batch, steps, warmup, half, dev):
    """ms per train step of the headline network under bf16 autocast with QuantConv2d.hip_train_half = ``half``."""
    import bench
    from quant.binary.binary_conv import QuantConv2d
    QuantConv2d.hip_train_half = half
    try:
        model = bench.build_model(bench.imagenet_arch('ls-2'), dev).train()
        opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn((batch, 3, 224, 224), generator=g, device=dev)
        y = torch.randint(0, 1000, (batch,), generator=g, device=dev)
        taken = {}
        quantized = [m for m in model.modules() if isinstance(m, QuantConv2d) and m.w_quant != 'fp']
        hooks = [m.register_forward_hook(lambda mod, i, o: taken.__setitem__(id(mod), (str(i[0].dtype), type(o.grad_fn).__name__)))
                 for m in quantized]

        def step():
            opt.zero_grad(set_to_none=True)
            with torch.autocast('cuda', torch.bfloat16):
                loss = F.cross_entropy(model(x), y)
            loss.backward()
            opt.step()
            return loss

        for _ in range(warmup):
            step()
        for hk in hooks:
            hk.remove()
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
        names = [v[1] for v in taken.values()]
        out = {'ms_per_step_median': statistics.median(times), 'ms_per_step_min': min(times), 'steps': steps, 'warmup': warmup,
               'max_memory_allocated_gib': torch.cuda.max_memory_allocated(dev) / 2 ** 30, 'last_loss': float(loss),
               'quantized_layers': len(quantized),
               'layers_handed_16_bit': sum(1 for v in taken.values() if v[0] != 'torch.float32'),
               'layers_on_the_16_bit_step': names.count('_QuantConv2dStepHalfBackward'),
               'layers_on_the_fp32_step': names.count('_QuantConv2dStepBackward')}
        del model, opt, x, y
        torch.cuda.empty_cache()
        return out
    finally:
        QuantConv2d.hip_train_half = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--skip-steps', action='store_true', help='per-layer times only')
    ap.add_argument('--skip-layers', action='store_true', help='train steps only')
    ap.add_argument('--decompose', action='store_true', help='per layer also the parts of both routes, each timed alone')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-steps', type=int, default=3, help='steps of the torch formulation (hip_train_half = False)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_train_half.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'conv_train_half_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'what': 'conv_train_half', 'device': torch.cuda.get_device_name(0), 'batch': args.batch, 'rounds': args.rounds,
           'weights': 'ls-1', 'activations': 'ls-2', 'layers': {}}
    if not args.skip_layers:
        for tname, dtype in DTYPES.items():
            rows = {}
            for shape in SHAPES:
                if only and shape[0] not in only:
                    continue
                rows[shape[0]] = layer_part(args.batch, shape, dtype, args.rounds, args.decompose)
                print(tname, shape[0], json.dumps(rows[shape[0]]), flush=True)
                torch.cuda.empty_cache()
            res['layers'][tname] = {'shapes': rows,
                                    'network_total_us': {v: sum(r['us'][v] * r['layers'] for r in rows.values())
                                                         for v in ('kernel', 'composition')}}
    if not args.skip_steps:
        import train_step
        dev = torch.device(DEV)
        steps = {}
        steps['autocast_bf16_hip_train_half'] = autocast_steps(args.batch, args.steps, args.warmup, True, dev)
        print('step half', json.dumps(steps['autocast_bf16_hip_train_half']), flush=True)
        steps['autocast_bf16_torch_formulation'] = autocast_steps(args.batch, args.torch_steps, 1, False, dev)
        print('step torch', json.dumps(steps['autocast_bf16_torch_formulation']), flush=True)
        steps['fp32_step'] = train_step.train_steps(args.batch, args.steps, args.warmup, False, dev)
        print('step fp32', json.dumps(steps['fp32_step']), flush=True)
        steps['autocast_bf16_hip_train_half_again'] = autocast_steps(args.batch, args.steps, args.warmup, True, dev)
        ms = {k: v['ms_per_step_median'] for k, v in steps.items()}
        steps['torch_formulation_over_half'] = ms['autocast_bf16_torch_formulation'] / ms['autocast_bf16_hip_train_half']
        steps['fp32_over_half'] = ms['fp32_step'] / ms['autocast_bf16_hip_train_half']
        res['train_step'] = dict(net='resnet18_imagenet_ls1w_ls2a', wgrad_kernel=False, dgrad_kernel=False, **steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
