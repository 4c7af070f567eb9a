#!/usr/bin/env python3
"""Two builds of liblsq_hip_train.so and liblsq_hip_train_half.so side by side in one process: the tree's
ml-quant_amd/lib against --parent DIR (the same two libraries built from another commit), loaded through ctypes with the
prototypes of quant/_sublibs.py and given the same operands.

  python scripts/wgrad_core_compare.py --parent DIR [--rounds 9] [--reps 30] [--skip-bits] [--skip-times] [--out profiles/wgrad_core.json]

bits    all 14 cases of tests/golden/train_wgrad_half_cases.py x {lsq_train_wgrad on an fp32 grad_y; lsq_train_wgrad_half on bf16
        and fp16, with and without grad_b}: the number of elements of grad_wq and grad_b whose raw bytes differ.  The kernels
        are deterministic functions of their operands, so anything but 0 means an order of summation moved.
times   batch 256: the five 3 x 3 ResNet-18 shapes with ls-2 planes (the <9, fold> kernels), 64 -> 64 at 56 x 56 with an ls-1
        plane (<9, no fold>), and a 1 x 1 stride-2 64 -> 128 at 56 x 56 with ls-2 and ls-1 (<1, ...>), each on the fp32 entry
        and on the 16-bit entry in both types with grad_b.  Parent and new alternate for --rounds rounds, a round being the
        median of --reps replays of a HIP graph of 3 calls; per shape the medians over the rounds, the spreads (max - min over
        the rounds, in us) and whether the new median lies within the parent's own spread of the parent's median."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'ml-quant_amd'), os.path.join(ROOT, 'scripts'), os.path.join(ROOT, 'tests', 'golden')]
import torch  # noqa: E402

import train_wgrad_half_cases as T  # noqa: E402
from conv_dgrad_bench import graph_time  # noqa: E402

DEV = 'cuda:0'
SENTINEL = -7.25
# (name, C, O, H, kernel, stride, pad, scheme)
TIMED = [('c64_56', 64, 64, 56, 3, 1, 1, 'ls-2'), ('c64_128_56_s2', 64, 128, 56, 3, 2, 1, 'ls-2'),
         ('c128_28', 128, 128, 28, 3, 1, 1, 'ls-2'), ('c256_14', 256, 256, 14, 3, 1, 1, 'ls-2'),
         ('c512_7', 512, 512, 7, 3, 1, 1, 'ls-2'), ('c64_56_ls1', 64, 64, 56, 3, 1, 1, 'ls-1'),
         ('p64_128_56_s2', 64, 128, 56, 1, 2, 0, 'ls-2'), ('p64_128_56_s2_ls1', 64, 128, 56, 1, 2, 0, 'ls-1')]


def load(directory):
    from quant import _sublibs
    libs = {}
    for name in ('train', 'train_half'):
        s = _sublibs.BY_DIR[name]
        libs[name] = ctypes.CDLL(os.path.join(directory, _sublibs.soname(s)))
        _sublibs.apply_prototypes(libs[name], s.prototypes)
    return libs


class Operands:
    """Planes and scales of a case from lsq_act_quant, one fp32 and two 16-bit gradients, outputs and a workspace."""

    def __init__(self, c, libs):
        from quant import _hip
        self.c, self.geom = c, _hip.make_geom(c.N, c.C, c.H, c.W, c.O, c.k[0], c.k[1], (c.stride, c.stride), c.pad, (1, 1), 1)
        code, self.k = T.SCHEMES[c.scheme]
        gen = torch.Generator().manual_seed(5)
        x = (torch.randn((c.N, c.C, c.H, c.W), generator=gen) * 1.3).to(DEV)
        self.planes = torch.zeros((self.k * _hip.act_plane_words(self.geom),), dtype=torch.int64, device=DEV)
        self.scales = torch.empty((self.k, c.N), dtype=torch.float32, device=DEV)
        _hip.act_quant(x, self.geom, code, self.k, 3, 2.0, self.planes, self.scales)
        gy = torch.randn((c.N, c.O) + T.out_hw(c), generator=gen) * 0.25
        self.gy = {'fp32': gy.to(DEV), 'bf16': gy.to(torch.bfloat16).to(DEV), 'fp16': gy.to(torch.float16).to(DEV)}
        g = ctypes.byref(self.geom)
        need = max(libs['train'].lsq_train_wgrad_workspace_bytes(g, self.k),
                   libs['train_half'].lsq_train_wgrad_half_workspace_bytes(g, self.k, 1))
        self.ws = torch.empty((need // 4 + 4,), dtype=torch.float32, device=DEV)
        self.gw = torch.empty((c.O, c.C) + c.k, dtype=torch.float32, device=DEV)
        self.gb = torch.empty((c.O,), dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()

    def run(self, libs, kind, bias=True):
        """One call of the entry for gradient type ``kind`` on the current stream."""
        g, st = ctypes.byref(self.geom), torch.cuda.current_stream().cuda_stream
        args = (self.planes.data_ptr(), self.k, self.scales.data_ptr(), self.gy[kind].data_ptr())
        tail = (self.ws.data_ptr(), self.ws.numel() * 4, st)
        if kind == 'fp32':
            code = libs['train'].lsq_train_wgrad(*args, g, self.gw.data_ptr(), *tail)
        else:
            code = libs['train_half'].lsq_train_wgrad_half(*args, T.DTYPE_CODES[self.gy[kind].dtype], g, self.gw.data_ptr(),
                                                           self.gb.data_ptr() if bias else None, *tail)
        assert code == 0, (self.c.id, kind, code)

    def result(self, libs, kind, bias):
        self.gw.fill_(SENTINEL)
        self.gb.fill_(SENTINEL)
        self.ws.fill_(float('nan'))
        self.run(libs, kind, bias)
        torch.cuda.synchronize()
        return self.gw.view(torch.int32).cpu().clone(), self.gb.view(torch.int32).cpu().clone()


def bits_part(parent, new):
    rows, total = {}, 0
    for c in T.CASES:
        ops = Operands(c, new)
        for kind, bias in (('fp32', False), ('bf16', True), ('bf16', False), ('fp16', True), ('fp16', False)):
            (pw, pb), (nw, nb) = ops.result(parent, kind, bias), ops.result(new, kind, bias)
            differ = int((pw != nw).sum()) + int((pb != nb).sum())
            rows[f'{c.id}-{kind}' + ('-bias' if bias else '')] = differ
            total += differ
        del ops
        torch.cuda.empty_cache()
    return {'runs': len(rows), 'elements_that_differ': total, 'per_run': rows}


def times_part(parent, new, batch, rounds, reps):
    out = {}
    for name, ci, o, h, k, s, p, scheme in TIMED:
        ops = Operands(T.Case(name, ci, o, batch, h, h, (k, k), s, (p, p), scheme), new)
        row = {}
        for kind in ('fp32', 'bf16', 'fp16'):
            samples = {'parent': [], 'new': []}
            for _ in range(rounds):
                for which, libs in (('parent', parent), ('new', new)):
                    samples[which].append(graph_time(lambda: ops.run(libs, kind), reps, 3))
            med = {w: statistics.median(t) for w, t in samples.items()}
            spread = {w: max(t) - min(t) for w, t in samples.items()}
            row[kind] = {'us': med, 'spread_us': spread, 'new_minus_parent_us': med['new'] - med['parent'],
                         'within_parent_spread': abs(med['new'] - med['parent']) <= spread['parent'],
                         'no_slower_than_parent_spread': med['new'] - med['parent'] <= spread['parent']}
            print(name, kind, json.dumps(row[kind]), flush=True)
        out[name] = row
        del ops
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help='directory with the other build of the two libraries')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--skip-bits', action='store_true')
    ap.add_argument('--skip-times', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wgrad_core.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'wgrad_core_compare.py runs on the GPU'
    from quant import _hip
    parent, new = load(args.parent), load(os.path.dirname(_hip.train_library_path()))
    res = {'what': 'wgrad_core', 'device': torch.cuda.get_device_name(0), 'batch': args.batch, 'rounds': args.rounds,
           'reps': args.reps, 'graph_chain': 3}
    if not args.skip_bits:
        res['bits'] = bits_part(parent, new)
        print('bits', res['bits']['runs'], 'runs,', res['bits']['elements_that_differ'], 'elements differ', flush=True)
    if not args.skip_times:
        res['times'] = times_part(parent, new, args.batch, args.rounds, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
