#!/usr/bin/env python3
"""Measurement of the binary linear layer (lsq_linear_xnor), one JSON document written to --out and printed.

  python scripts/linear_bench.py [--reps R] [--out profiles/linear_xnor.json]

Per shape (LeNet fc1, the ResNet-18 head, an MLP-sized GEMM with ls-1 / ls-1 and ls-2 / ls-1), median microseconds of:
  * lsq_linear_xnor (the fp4 matrix-core GEMM),
  * the 1x1 popcount route (lsq_xnor_conv2d on (M, F, 1, 1)) from the same planes -- the two outputs are compared bit for bit,
  * F.linear in fp32 and in bf16 on the dequantized operands x_q, w_q,
  * the whole QuantLinear eval forward (quantizer + GEMM) and its torch formulation for reference.
Kernel times are HIP-graph replays of `chain` back-to-back calls (no host time between launches), divided by `chain`;
the QuantLinear forward is timed eagerly, host work included.  Also: the fraction of the ~10 PF dense fp4 peak
(2 M F O kx kw binary operations) and the output bytes written per second against the ~8 TB/s of HBM."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'tests', 'golden')]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_FP4 = 10e15         # dense fp4 MFMA operations per second of the MI355X
HBM = 8e12               # bytes per second
DEV = 'cuda:0'
ACT = {'ls-1': (1, 1), 'ls-2': (2, 2)}
SHAPES = [('lenet_fc1', 64, 800, 500, 'ls-2', 'ls-1'), ('resnet18_head', 256, 512, 1000, 'ls-2', 'ls-1'),
          ('mlp_ls1_ls1', 8192, 4096, 4096, 'ls-1', 'ls-1'), ('mlp_ls2_ls1', 8192, 4096, 4096, 'ls-2', 'ls-1')]


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


def one_shape(name, m, f, o, xs, ws, reps):
    from quant import _hip
    from quant.binary import QuantLinear
    from oracle import ref_port as P
    code, k = ACT[xs]
    g = torch.Generator().manual_seed(0)
    x = torch.randn((m, f), generator=g).to(DEV)
    lin = QuantLinear(xs, ws, f, o, {'kind': 'symmetric', 'alpha': 2})
    with torch.no_grad():
        lin.weight.copy_(torch.randn((o, f), generator=g) * 0.05)
        for buf, v in zip(lin.w_approximate.cached_scales(), P.weight_scales(lin.weight.view(o, f, 1, 1), ws)):
            buf.copy_(v)
    lin.eval().to(DEV)
    gx = _hip.make_geom(m, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    planes = torch.zeros((k * _hip.act_plane_words(gx),), dtype=torch.int64, device=DEV)
    scales = torch.empty((k, m), dtype=torch.float32, device=DEV)
    _hip.act_quant(x, gx, code, k, 3, 2.0, planes, scales)
    wsc = lin.w_approximate.plane_scales().float().contiguous()
    wbits, wsum = _hip.pack_weight(lin.weight.detach().view(o, f, 1, 1), gx, wsc)
    wsum2 = wsum.view(-1, o)
    bias = lin.bias.detach()
    kw = wsc.shape[0]
    y_pop = torch.empty((m, o, 1, 1), dtype=torch.float32, device=DEV)

    def kernel():
        return _hip.linear_xnor(planes, k, scales, 1, wbits, wsum2, wsc, bias, m, f, o)

    def popcount():
        _hip.xnor_conv2d(planes, k, scales, wbits, wsum, wsc, bias, gx, y_pop)

    y = kernel()
    popcount()
    torch.cuda.synchronize()
    same = bool(torch.equal(y.view(torch.int32), y_pop.view(m, o).view(torch.int32)))
    with torch.no_grad():
        xq = P.quantize_activation(P.clamp_act(x.reshape(m, f, 1, 1), {'kind': 'symmetric', 'alpha': 2}), xs,
                                   scales=[scales[i] for i in range(k)])[1].reshape(m, f)
        wq = P.quantize_weight(lin.weight.detach().view(o, f, 1, 1), ws, lin.w_approximate.cached_scales()).view(o, f)
    xq16, wq16, b16 = xq.bfloat16(), wq.bfloat16(), bias.bfloat16()
    chain = 200 if m * f * o < 1 << 30 else 10
    out = {'M': m, 'F': f, 'O': o, 'x_quant': xs, 'w_quant': ws, 'bit_identical_to_popcount': same, 'graph_chain': chain}
    out['us_lsq_linear_xnor'] = graph_time(kernel, reps, chain)
    out['us_popcount_1x1'] = graph_time(popcount, reps, chain)
    out['us_f_linear_fp32'] = graph_time(lambda: F.linear(xq, wq, bias), reps, chain)
    out['us_f_linear_bf16'] = graph_time(lambda: F.linear(xq16, wq16, b16), reps, chain)
    with torch.no_grad():
        out['us_quant_linear_eval'] = eager_time(lambda: lin(x), reps)
        out['us_quant_linear_eval_kernels_graph'] = graph_time(lambda: lin(x), reps, chain)
    ops = 2.0 * m * f * o * k * kw
    t = out['us_lsq_linear_xnor'] * 1e-6
    out['fp4_peak_fraction'] = ops / t / PEAK_FP4
    launches = kw * ((k + 1) // 2)
    ybytes = 4.0 * m * o * (2 * launches - 1)          # y written per launch, read back by every launch after the first
    out['y_bytes'] = ybytes
    out['y_bytes_hbm_fraction'] = ybytes / t / HBM
    out['speedup_vs_popcount'] = out['us_popcount_1x1'] / out['us_lsq_linear_xnor']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'linear_xnor.json'))
    args = ap.parse_args()
    torch.manual_seed(0)
    res = {'device': torch.cuda.get_device_name(0), 'peak_fp4_ops': PEAK_FP4, 'hbm_bytes_per_s': HBM, 'shapes': {}}
    for name, m, f, o, xs, ws in SHAPES:
        res['shapes'][name] = one_shape(name, m, f, o, xs, ws, args.reps)
        print(name, json.dumps(res['shapes'][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
