#!/usr/bin/env python3
"""Measurement of the fp-activation x sign-weight linear layer (lsq_linear_signw), one JSON document written to --out and
printed.

  python scripts/linear_fp_bench.py [--rounds R] [--out profiles/linear_signw.json]

Shapes: LeNet fc1, the ResNet-18 head, decode rows (M = 1 and 16, 4096 -> 4096) and an MLP-sized GEMM (8192 x 4096 -> 4096),
the last two with ls-1 and ls-2 weights, and three workloads around the library's choice between its two kernels
(M = 128, 256, 512 at 4096 -> 4096: fewer than 256 tiles of 64 x 64 take the F-split kernel, so 128 rows do and 256 / 512
rows take 64 x 64 tiles).  Per shape, microseconds of
  * lsq_linear_signw, as a graph and eagerly (events around back-to-back calls: the per-call cost with y allocated by
    the caching allocator outside any graph),
  * at 256 / 512 rows, the same rows as calls of 128 rows each: the F-split kernel on the work the tiled one does,
  * the existing route: lsq_signw_conv2d on the 1x1 view (M, F, 1, 1) over the same sign planes,
  * F.linear in fp32 and in bf16 on the dequantized operands clamp(x), w_q,
  * the QuantLinear eval forward against its torch formulation (_forward_torch),
and the max error of each route against fp64, plus the share of the bf16 peak (hi and lo pass of every plane) or of HBM
(x read, the sign planes read, y written), whichever bounds the shape.  Decode rows are also timed with the weights
rotated over enough layers that the fp32 operands (64 MB a layer) exceed the 256 MiB Infinity Cache: what a deep model sees.
Kernel times are HIP-graph replays of `chain` back-to-back calls divided by `chain`; the module forward is timed eagerly,
host work included.  Every variant of a shape is warmed up, then timed once per round with the variants alternating; the
median over the rounds is reported with its spread (max - min over median)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_BF16 = 2.5e15       # dense bf16 MFMA FLOP/s of the MI355X
HBM = 8e12               # bytes per second
DEV = 'cuda:0'
CLAMP = {'kind': 'symmetric', 'alpha': 2}
ROTATE = 10              # layers of 64 MB fp32 weights for the rotated decode rows (640 MB > 256 MiB)
SHAPES = [('lenet_fc1', 64, 800, 500, 'ls-1'), ('resnet18_head', 256, 512, 1000, 'ls-1'),
          ('decode_m1_ls1', 1, 4096, 4096, 'ls-1'), ('decode_m1_ls2', 1, 4096, 4096, 'ls-2'),
          ('decode_m16_ls1', 16, 4096, 4096, 'ls-1'), ('decode_m16_ls2', 16, 4096, 4096, 'ls-2'),
          ('mlp_ls1', 8192, 4096, 4096, 'ls-1'), ('mlp_ls2', 8192, 4096, 4096, 'ls-2'),
          ('switch_m128', 128, 4096, 4096, 'ls-1'), ('switch_m256', 256, 4096, 4096, 'ls-1'),
          ('switch_m512', 512, 4096, 4096, 'ls-1')]
SPLIT_ROWS = 128         # at 4096 outputs the largest row block that takes the F-split kernel (2 x 64 tiles of 64 x 64)


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


def eager_time(fn, reps, inner=20):
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


def rotating(fns):
    """One callable that runs fns[0], fns[1], ... in turn (captured into a graph: a different layer per call)."""
    state = [0]

    def step():
        fns[state[0] % len(fns)]()
        state[0] += 1
    return step


def layer(m, f, o, ws, seed):
    from quant import _hip
    from quant.binary import QuantLinear
    from oracle import ref_port as P
    g = torch.Generator().manual_seed(seed)
    lin = QuantLinear('fp', ws, f, o, CLAMP)
    with torch.no_grad():
        lin.weight.copy_(torch.randn((o, f), generator=g) * 0.05)
        lin.bias.copy_(torch.randn((o,), generator=g) * 0.1)
        for buf, v in zip(lin.w_approximate.cached_scales(), P.weight_scales(lin.weight.view(o, f, 1, 1), ws)):
            buf.copy_(v)
    lin.eval().to(DEV)
    wsc = lin.w_approximate.plane_scales().float().contiguous()
    geom = _hip.make_geom(m, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    wbits, _ = _hip.pack_weight(lin.weight.detach().view(o, f, 1, 1), geom, wsc)
    with torch.no_grad():
        wq = P.quantize_weight(lin.weight.detach().cpu().view(o, f, 1, 1), ws,
                               [b.cpu() for b in lin.w_approximate.cached_scales()]).view(o, f).to(DEV)
    return lin, wsc, wbits, wq, geom


def one_shape(name, m, f, o, ws, rounds):
    from quant import _hip
    torch.manual_seed(0)
    x = (torch.randn((m, f), generator=torch.Generator().manual_seed(1)) * 1.2).to(DEV)
    lin, wsc, wbits, wq, geom = layer(m, f, o, ws, seed=2)
    bias = lin.bias.detach()
    kw = wsc.shape[0]
    xc = x.clamp(-2, 2)
    xc16, wq16, b16 = xc.bfloat16(), wq.bfloat16(), bias.bfloat16()
    y_conv = torch.empty((m, o, 1, 1), dtype=torch.float32, device=DEV)
    x4 = x.view(m, f, 1, 1)

    def kernel():
        return _hip.linear_signw(x, 2.0, wbits, wsc, bias, m, f, o)

    def conv1x1():
        _hip.signw_conv2d(x4, 2.0, wbits, wsc, bias, geom, y_conv)

    variants = {'lsq_linear_signw': kernel, 'signw_conv2d_1x1': conv1x1,
                'f_linear_fp32': lambda: F.linear(xc, wq, bias), 'f_linear_bf16': lambda: F.linear(xc16, wq16, b16)}
    decode = m <= 16
    if decode:
        layers = [layer(m, f, o, ws, seed=10 + i) for i in range(ROTATE)]
        variants['lsq_linear_signw_rotated'] = rotating(
            [(lambda L=L: _hip.linear_signw(x, 2.0, L[2], L[1], L[0].bias.detach(), m, f, o)) for L in layers])
        variants['f_linear_fp32_rotated'] = rotating([(lambda L=L: F.linear(xc, L[3], L[0].bias.detach())) for L in layers])
    if name.startswith('switch') and m > SPLIT_ROWS:
        blocks = [x[r:r + SPLIT_ROWS] for r in range(0, m, SPLIT_ROWS)]

        def split_blocks():
            for xb in blocks:
                _hip.linear_signw(xb, 2.0, wbits, wsc, bias, xb.shape[0], f, o)
        variants['split_kernel_in_128_row_calls'] = split_blocks

    # errors against fp64
    with torch.no_grad():
        y64 = F.linear(xc.double(), wq.double(), bias.double())
        scale = y64.abs().max().item()
        outs = {'lsq_linear_signw': kernel()}
        conv1x1()
        outs['signw_conv2d_1x1'] = y_conv.view(m, o)
        outs['f_linear_fp32'] = F.linear(xc, wq, bias)
        outs['f_linear_bf16'] = F.linear(xc16, wq16, b16)
        outs['quant_linear_eval'] = lin(x)
        outs['quant_linear_forward_torch'] = lin._forward_torch(x)
    torch.cuda.synchronize()
    out = {'M': m, 'F': f, 'O': o, 'w_quant': ws, 'weight_planes': kw,
           'max_rel_err_vs_fp64': {k: (v.double() - y64).abs().max().item() / scale for k, v in outs.items()}}

    chain = 200 if m * f * o < 1 << 30 else 10
    if decode:
        chain = 10 * ROTATE
    reps = 5
    # warm-up of every variant, then rounds with the variants alternating
    for fn in variants.values():
        graph_time(fn, 1, chain)
    with torch.no_grad():
        eager_time(lambda: lin(x), 1)
        eager_time(lambda: lin._forward_torch(x), 1)
        eager_time(kernel, 1)
    samples = {k: [] for k in list(variants) + ['lsq_linear_signw_eager', 'quant_linear_eval', 'quant_linear_forward_torch']}
    for _ in range(rounds):
        for k, fn in variants.items():
            samples[k].append(graph_time(fn, reps, chain))
        samples['lsq_linear_signw_eager'].append(eager_time(kernel, reps))
        with torch.no_grad():
            samples['quant_linear_eval'].append(eager_time(lambda: lin(x), reps))
            samples['quant_linear_forward_torch'].append(eager_time(lambda: lin._forward_torch(x), reps))
    out['us'] = {k: statistics.median(v) for k, v in samples.items()}
    out['spread'] = {k: (max(v) - min(v)) / statistics.median(v) for k, v in samples.items()}
    out['graph_chain'] = chain

    flops = 2.0 * 2.0 * m * f * o * kw                       # hi and lo pass of every plane
    nbytes = 4.0 * m * f + kw * ((f + 63) // 64) * ((o + 15) // 16 * 16) * 8 + 4.0 * m * o
    t = out['us']['lsq_linear_signw'] * 1e-6
    t_mfma, t_hbm = flops / PEAK_BF16, nbytes / HBM
    out['bf16_flops'], out['bytes'] = flops, nbytes
    out['bound'] = 'bf16 peak' if t_mfma >= t_hbm else 'HBM'
    out['peak_share'] = max(t_mfma, t_hbm) / t
    us = out['us']
    out['speedup'] = {'vs_f_linear_fp32': us['f_linear_fp32'] / us['lsq_linear_signw'],
                      'vs_signw_conv2d_1x1': us['signw_conv2d_1x1'] / us['lsq_linear_signw'],
                      'quant_linear_eval_vs_forward_torch': us['quant_linear_forward_torch'] / us['quant_linear_eval']}
    if 'split_kernel_in_128_row_calls' in us:
        out['speedup']['tiled_vs_split_kernel'] = us['split_kernel_in_128_row_calls'] / us['lsq_linear_signw']
    if decode:
        out['speedup']['rotated_vs_f_linear_fp32_rotated'] = us['f_linear_fp32_rotated'] / us['lsq_linear_signw_rotated']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', default='', help='comma-separated shape names (default: all)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linear_signw.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'linear_fp_bench.py measures on the GPU'
    only = set(filter(None, args.only.split(',')))
    res = {'device': torch.cuda.get_device_name(0), 'peak_bf16_flops': PEAK_BF16, 'hbm_bytes_per_s': HBM,
           'rounds': args.rounds, 'shapes': {}}
    for name, m, f, o, ws in SHAPES:
        if only and name not in only:
            continue
        res['shapes'][name] = one_shape(name, m, f, o, ws, args.rounds)
        print(name, json.dumps(res['shapes'][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
