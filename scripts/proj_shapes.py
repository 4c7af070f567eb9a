"""Developer tool: the three down-sampling layers of ResNet-18 at batch N, the projection shortcut as a launch of its own
(lsq_pointwise_conv + lsq_xnor_conv2d) against the fused launch (lsq_xnor_conv2d_proj), alternating, device events around
REPS back-to-back calls, median of ROUNDS; checks that both give the same bits at these sizes.  One JSON line per shape.
usage: python scripts/proj_shapes.py [N]"""

import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ml-quant_amd')):
    sys.path.insert(0, p)

import torch  # noqa: E402

from quant import _hip as hip  # noqa: E402

DEV = 'cuda:0'
REPS, ROUNDS = 20, 7
SHAPES = [(64, 128, 56), (128, 256, 28), (256, 512, 14)]       # (Cp = C, O, input height): 3x3 stride-2 consumer, double shortcut


def timed(fn):
    out = []
    for _ in range(ROUNDS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(REPS):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / REPS)
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    torch.manual_seed(0)
    for c, o, h in SHAPES:
        geom = hip.make_geom(n, c, h, h, o, 3, 3, (2, 2), (1, 1), (1, 1), 1)
        x = torch.randn((n, c, h, h), device=DEV)
        planes = torch.zeros((2 * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
        xs = torch.empty((2, n), dtype=torch.float32, device=DEV)
        hip.act_quant(x, geom, hip.SCHEME_LS2, 2, 3, 3.0, planes, xs)
        wt = torch.randn((o, c, 3, 3), device=DEV)
        wsc = wt.abs().mean(dim=(1, 2, 3))[None].contiguous()
        wbits, wsum = hip.pack_weight(wt, geom, wsc)
        bias, pb = torch.randn((o,), device=DEV), torch.randn((o,), device=DEV)
        pw = torch.randn((o, c), device=DEV) * c ** -0.5
        ho, wo = hip.out_hw(geom)
        y2, y1 = torch.empty((n, o, ho, wo), device=DEV), torch.empty((n, o, ho, wo), device=DEV)

        def pair():
            sc = hip.pointwise_conv(x, pw, pb, 2)
            hip.xnor_conv2d(planes, 2, xs, wbits, wsum, wsc, bias, geom, y2, relu=True, res_post=sc)

        def pw_only():
            hip.pointwise_conv(x, pw, pb, 2)

        def fused():
            assert hip.xnor_conv2d_proj(planes, 2, xs, wbits, wsum, wsc, bias, geom, y1, (x, pw, pb, 2, True), relu=True)

        pair(); fused(); torch.cuda.synchronize()
        same = bool(torch.equal(y1, y2))
        t_pair, t_fused = [], []
        for _ in range(3):                                         # alternate the two
            t_pair += timed(pair)
            t_fused += timed(fused)
        t_pw = timed(pw_only)
        print(json.dumps({'Cp': c, 'O': o, 'H': h, 'N': n, 'same_bits': same,
                          'pair_us': round(statistics.median(t_pair), 1), 'pair_min_max': [round(min(t_pair), 1), round(max(t_pair), 1)],
                          'fused_us': round(statistics.median(t_fused), 1), 'fused_min_max': [round(min(t_fused), 1), round(max(t_fused), 1)],
                          'pointwise_alone_us': round(statistics.median(t_pw), 1)}), flush=True)


if __name__ == '__main__':
    main()
