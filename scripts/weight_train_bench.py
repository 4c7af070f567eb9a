#!/usr/bin/env python3
"""Measurement of lsq_weight_quant_pack, the train step's weight side in one launch, one JSON document written to --out and
printed.

  python scripts/weight_train_bench.py [--rounds R] [--skip-steps] [--out profiles/weight_train.json]

  call    microseconds per call, eager with host work included (HIP events around `inner` back-to-back calls), of
          _hip.weight_quant_pack against the parent route on the same weight: the torch weight quantizer's train-mode forward,
          plane_scales(), lsq_pack_weight.  (The parent route is not captured in a graph: lsq_pack_weight records a memset.)
          `kernel_graph_us` is the one launch alone, replayed from a HIP graph.  Shapes: every distinct quantized conv weight
          of ResNet-18, LeNet's layers, the ResNet head and 4096 x 4096; schemes ls-1, ls-2, ls-T, gf-2.  The two routes'
          planes are compared where their scales agree in every bit (`same_bits`).
  resnet  ms per train step of scripts/train_step.py's network (ResNet-18, ls-1 weights / ls-2 activations) at batch 256 and
          8 with hip_train_common.WEIGHT_KERNEL on and off.
  linear  microseconds per QuantLinear train step (forward, backward, SGD) at 512 and 8192 x 4096 -> 4096 and LeNet fc1 with
          the switch on and off, and of the torch formulation (hip_train False).
Every variant is warmed up, then timed once per round with the variants alternating; medians over the rounds with their
spread (max - min over median)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'scripts')]
import torch  # noqa: E402

DEV = 'cuda:0'
# (name, O, C, KH, KW)
SHAPES = [('r18_64x64_3x3', 64, 64, 3, 3), ('r18_128x64_3x3', 128, 64, 3, 3), ('r18_128x128_3x3', 128, 128, 3, 3),
          ('r18_256x128_3x3', 256, 128, 3, 3), ('r18_256x256_3x3', 256, 256, 3, 3), ('r18_512x256_3x3', 512, 256, 3, 3),
          ('r18_512x512_3x3', 512, 512, 3, 3), ('r18_proj_128x64', 128, 64, 1, 1), ('r18_proj_256x128', 256, 128, 1, 1),
          ('r18_proj_512x256', 512, 256, 1, 1), ('lenet_conv2_50x20_5x5', 50, 20, 5, 5), ('lenet_fc1_500x800', 500, 800, 1, 1),
          ('lenet_fc2_10x500', 10, 500, 1, 1), ('r18_head_1000x512', 1000, 512, 1, 1), ('mlp_4096x4096', 4096, 4096, 1, 1)]
SCHEMES = ('ls-1', 'ls-2', 'ls-T', 'gf-2')
LINEAR = [('mlp_m512', 512, 4096, 4096), ('mlp_m8192', 8192, 4096, 4096), ('lenet_fc1', 64, 800, 500)]
SKIP = 3


def eager_time(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def graph_of(fn, chain):
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
    return g


def summarize(samples):
    return {k: {'median': statistics.median(v), 'spread': (max(v) - min(v)) / statistics.median(v)} for k, v in samples.items()}


def call_part(rounds, inner=20, chain=20):
    from quant import _hip
    from quant.binary.hip_module import HipQuantModule
    out = {}
    for name, o, c, kh, kw in SHAPES:
        geom = _hip.make_geom(1, c, kh, kw, o, kh, kw, (1, 1), (0, 0), (1, 1), 1)
        w = (torch.randn((o, c, kh, kw), generator=torch.Generator().manual_seed(5)) * 0.05).to(DEV)
        for ws in SCHEMES:
            wq = HipQuantModule._get_w_quantizer(ws, o).to(DEV).train()

            def kernel():
                return _hip.weight_quant_pack(w, geom, wq.hip_scheme, wq.n_planes, SKIP)

            def parent():
                with torch.no_grad():
                    wq(w)
                    sc = wq.plane_scales().to(torch.float32).contiguous()
                return (sc,) + tuple(_hip.pack_weight(w, geom, sc))

            assert _hip.weight_quant_pack_supported(geom, wq.hip_scheme, wq.n_planes, SKIP)
            new, old = kernel(), parent()
            same_scales = torch.equal(new[0], old[0])
            rec = {'scales_same_bits': same_scales,
                   'scales_max_rel_diff': float(((new[0] - old[0]).abs() / old[0].abs().clamp_min(1e-30)).max()),
                   'planes_same_bits': (torch.equal(new[1], old[1]) and torch.equal(new[2], old[2])) if same_scales else None}
            graph = graph_of(kernel, chain)
            for fn in (kernel, parent):
                eager_time(fn, inner)
            samples = {'kernel_us': [], 'parent_us': [], 'kernel_graph_us': []}
            for _ in range(rounds):
                samples['kernel_us'].append(eager_time(kernel, inner))
                samples['parent_us'].append(eager_time(parent, inner))
                samples['kernel_graph_us'].append(eager_time(graph.replay, 5) / chain)
            rec.update(summarize(samples))
            rec['bytes'] = 4 * w.numel() + 8 * new[1].numel() + 4 * new[2].numel()
            out[f'{name}.{ws}'] = rec
            print(name, ws, {k: round(v['median'], 1) for k, v in rec.items() if isinstance(v, dict)}, flush=True)
    return out


def resnet_part(rounds):
    import train_step
    from quant.binary import hip_train_common
    out = {}
    for batch in (256, 8):
        samples = {'on_ms': [], 'off_ms': []}
        for _ in range(rounds):
            for key, flag in (('on_ms', True), ('off_ms', False)):
                hip_train_common.WEIGHT_KERNEL = flag
                samples[key].append(train_step.train_steps(batch, 10, 3, False, DEV)['ms_per_step_median'])
        hip_train_common.WEIGHT_KERNEL = False
        out[f'batch{batch}'] = summarize(samples)
        print('resnet18 batch', batch, out[f'batch{batch}'], flush=True)
    return out


def linear_part(rounds, inner=5):
    from quant.binary import QuantLinear, hip_train_common
    out = {}
    for name, m, f, o in LINEAR:
        for ws in ('ls-1', 'ls-2'):
            x = torch.randn((m, f), generator=torch.Generator().manual_seed(1)).to(DEV)
            gy = torch.randn((m, o), generator=torch.Generator().manual_seed(2)).to(DEV)
            steps = {}
            for key, hip_train, flag in (('kernel_step_on_us', True, True), ('kernel_step_off_us', True, False),
                                         ('torch_step_us', False, False)):
                lin = QuantLinear('ls-2', ws, f, o, {'kind': 'symmetric', 'alpha': 2})
                lin.hip_train = hip_train
                lin = lin.to(DEV).train()
                opt = torch.optim.SGD(lin.parameters(), lr=1e-3)

                def step(lin=lin, opt=opt, flag=flag):
                    hip_train_common.WEIGHT_KERNEL = flag
                    opt.zero_grad(set_to_none=True)
                    xin = x.detach().requires_grad_()
                    lin(xin).backward(gy)
                    opt.step()

                steps[key] = step
                eager_time(step, 3)
            samples = {k: [] for k in steps}
            for _ in range(rounds):
                for k, step in steps.items():
                    samples[k].append(eager_time(step, inner))
            hip_train_common.WEIGHT_KERNEL = False
            out[f'{name}.{ws}'] = summarize(samples)
            print(name, ws, {k: round(v['median'], 1) for k, v in out[f'{name}.{ws}'].items()}, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-steps', action='store_true', help='the calls only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'weight_train.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs cuda:0'
    doc = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'skip': SKIP, 'call': call_part(args.rounds)}
    if not args.skip_steps:
        doc['linear'] = linear_part(args.rounds)
        doc['resnet18'] = resnet_part(max(2, args.rounds // 2))
    with open(args.out, 'w') as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == '__main__':
    main()
