#!/usr/bin/env python3
"""Derive the limits of the FREE-RUNNING GPU parity assertions from the oracle (no GPU, no reference import).

With the reference's scales injected every GPU bit plane is exact and conv outputs agree to 1e-4.  Free running, the
GPU solves for v1 in exact arithmetic and the reference picks among near-tied candidates with the fp32 rounding of its
own reductions (optimal.py:31-38, :151), so outputs differ by what that tie-break moves.  How much that is can be
computed WITHOUT the GPU: run the oracle with the exact argmin (``oracle.ref_port.exact_solver``) and compare with the
reference's outputs (the committed fixtures).  The GPU's v1 is bit-equal to that exact argmin (asserted separately),
so for ONE layer

    |y_gpu - y_ref| <= |y_exact_oracle - y_ref| + |y_gpu - y_exact_oracle| <= tiebreak + 1e-4 max|y|.

Through several layers a binarized network amplifies arithmetic noise (a CPU and a GPU convolution differ in the last
bits; an activation within that distance of a threshold flips a +-1).  That amplification is a property of the network,
measured here on the oracle itself: the same exact-argmin forward on the input scaled by (1 + eps), |eps| <= 2^-21
(a few ulps, the size of the CPU / GPU differences in the fp stem), three seeds -> ``sensitivity``.

    limit(one layer)      = 1.05 * tiebreak + 1e-4
    limit(several layers) = 1.05 * tiebreak + 2 * sensitivity
    limit(GPU vs GPU: fused against module-by-module blocks) = 2 * sensitivity
    cosine distances are taken in fp64 and floored at 1e-9 (what 24-bit logits resolve)

Writes tests/golden/free_limits.json; tests/test_free_limits.py re-derives entries on the CPU, tests/test_gpu_parity.py
asserts the GPU against them.  usage: python tests/golden/make_free_limits.py
"""

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'ml-quant_amd'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import detgen  # noqa: E402
from oracle import ref_models as RM  # noqa: E402
from oracle import ref_port as P  # noqa: E402

TOL = 1e-4
PAIRS = [('ls-1', 'ls-1'), ('ls-2', 'ls-1'), ('ls-T', 'ls-1'), ('gf-2', 'ls-1'),
         ('ls-2', 'ls-2'), ('ls-1', 'gf-2'), ('ls-T', 'ls-T')]
NETS = {'imagenet_ls1w_ls2a': (2, 3, 64, 64), 'imagenet_ls1w_lsTa': (2, 3, 64, 64), 'imagenet_ls1w_gf2a': (2, 3, 64, 64),
        'cifar100_ls1': (4, 3, 32, 32), 'imagenet_ls1w_fpa': (2, 3, 64, 64)}


def load(name):
    out, i, path = {}, 0, os.path.join(HERE, name + '.npz')
    while os.path.exists(path):                       # <name>.npz, then its continuation files <name>.1.npz, ...
        z = np.load(path)
        out.update((k, torch.from_numpy(np.array(z[k]))) for k in z.files)
        i += 1
        path = os.path.join(HERE, f'{name}.{i}.npz')
    return out


def rel_err(y, ref):
    return float((y - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def cos_dist(y, ref):
    return 1.0 - float(torch.nn.functional.cosine_similarity(y.flatten().double(), ref.flatten().double(), dim=0))


def perturbed(x, seed):
    """x * (1 + eps), |eps| <= 2^-21: noise of the size of CPU / GPU arithmetic differences."""
    rs = np.random.RandomState(1000 + seed)
    eps = torch.from_numpy(rs.uniform(-1.0, 1.0, tuple(x.shape)).astype(np.float32)) * 2.0 ** -21
    return x * (1.0 + eps)


def conv_layers():
    """tiebreak of the single-layer cases (tests: test_quant_conv2d_vs_reference_fixture, ..._lenet_geometry_and_edges)."""
    g = load('f5_conv')
    out = {}
    x = detgen.normal('f5.x', (2, 64, 14, 14), scale=1.2)
    w = detgen.normal('f5.w.64.64.3', (64, 64, 3, 3), scale=(64 * 9) ** -0.5)
    b = detgen.normal('f5.w.64.64.3.b', (64,), scale=0.1)
    worst = 0.0
    for xs, ws in PAIRS:
        for stride in (1, 2):
            for alpha in (2, 3):
                key = f'{xs}_{ws}_s{stride}_a{alpha}'
                if key + '_xv1' not in g:
                    continue
                wsc = [g[f'{key}_w_v{i}'] for i in range(1, 9) if f'{key}_w_v{i}' in g]
                with P.exact_solver():
                    y = P.quant_conv2d(x, w, b, xs, ws, wsc, {'kind': 'symmetric', 'alpha': alpha}, stride, 1)
                worst = max(worst, rel_err(y, g[key + '_y']))
    out['conv_fixture'] = {'tiebreak': worst}
    xl = detgen.normal('f5.xl', (2, 20, 12, 12))
    wl = detgen.normal('f5.w.20.50.5', (50, 20, 5, 5), scale=500 ** -0.5)
    bl = detgen.normal('f5.w.20.50.5.b', (50,), scale=0.1)
    worst = 0.0
    for xs in ('ls-2', 'ls-T'):
        with P.exact_solver():
            y = P.quant_conv2d(xl, wl, bl, xs, 'ls-1', [g[f'lenet_{xs}_ls-1_w_v1']])
        worst = max(worst, rel_err(y, g[f'lenet_{xs}_ls-1_y']))
    out['conv_lenet'] = {'tiebreak': worst}
    wg = detgen.normal('f5.w.64.64.(3, 2)', (64, 32, 3, 2), scale=(32 * 6) ** -0.5)
    bg = detgen.normal('f5.w.64.64.(3, 2).b', (64,), scale=0.1)
    with P.exact_solver():
        y = P.quant_conv2d(x, wg, bg, 'ls-2', 'ls-1', [g['geo_w_v1']], {'kind': 'symmetric', 'alpha': 2}, (2, 1), (2, 1), (2, 1), 2)
    out['conv_geometry'] = {'tiebreak': rel_err(y, g['geo_y'])}
    for v in out.values():
        v['limit'] = 1.05 * v['tiebreak'] + TOL
        v['formula'] = '1.05 * tiebreak + 1e-4'
    return out


def filled_state_dict(module, seed):
    """state_dict of a product module tree filled as the tests fill it (names and shapes only come from the product)."""
    from quant.binary.binary_conv import QuantConv2d
    detgen.fill_module(module, seed=seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, QuantConv2d) and hasattr(m.w_approximate, 'v1'):
                for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight, m.w_quant)):
                    buf.copy_(v)
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def block_case():
    from quant.models.resnet import XnorBasicBlock
    g = load('f6_models')
    clamp = {'kind': 'symmetric', 'alpha': 3}
    blk = XnorBasicBlock(64, 128, 'ls-2', 'ls-1', ['relu', 'relu'], stride=2, double_shortcut=True, clamp=clamp)
    sd = filled_state_dict(blk, 2)
    cfg = {'x_quant': 'ls-2', 'w_quant': 'ls-1', 'clamp': clamp, 'double_shortcut': True}
    x = detgen.normal('block.x', (2, 64, 16, 16))

    def fwd(inp):
        with P.exact_solver():
            return RM.xnor_block_forward(sd, '', inp, cfg, ['relu', 'relu'], 2, True)
    y = fwd(x)
    # the reference's own arithmetic reproduces the fixture exactly (this pins the functional block)
    assert torch.equal(RM.xnor_block_forward(sd, '', x, cfg, ['relu', 'relu'], 2, True), g['block_y'])
    sens = max(rel_err(fwd(perturbed(x, s)), y) for s in range(3))
    sens_cos = max(cos_dist(fwd(perturbed(x, s)), y) for s in range(3))
    return {'block': {'tiebreak': rel_err(y, g['block_y']), 'sensitivity': sens},
            'block_cos': {'tiebreak': cos_dist(y, g['block_y']), 'sensitivity': sens_cos}}


def net_cases():
    from quant.models.resnet import QResNet
    g = load('f6_models')
    per = {}
    for tag, shape in NETS.items():
        arch = json.loads(bytes(g[tag + '_arch'].numpy()).decode())
        model = QResNet(loss_fn=None, **arch)
        sd = filled_state_dict(model, 1)
        x = detgen.normal(tag + '.x', shape)
        ref = g[tag + '_logits']

        def fwd(inp):
            with P.exact_solver():
                return RM.resnet_forward(sd, arch, inp)
        y = fwd(x)
        ys = [fwd(perturbed(x, s)) for s in range(3)]
        per[tag] = {'tiebreak': rel_err(y, ref), 'tiebreak_cos': cos_dist(y, ref),
                    'sensitivity': max(rel_err(v, y) for v in ys), 'sensitivity_cos': max(cos_dist(v, y) for v in ys)}
    return per


def fp_cases():
    """The schemes WITHOUT a search on fp activations (BASELINE configs 0 and 3): nothing to tie-break; what the GPU's
    operand rounding (bf16 hi + lo split of the activations, oracle.ref_port.split_operands) moves, plus the network's
    own sensitivity to arithmetic noise.  limit = 1.05 * split + 2 * sensitivity (tests: test_config0_lenet_and_fp_act_resnet_on_gpu)."""
    from quant.models.lenet import QLeNet5
    from quant.models.resnet import QResNet
    g7, g6 = load('f7_lenet'), load('f6_models')
    out = {}
    arch = json.loads(bytes(g7['mnist_ls1w_fpa_arch'].numpy()).decode())
    model = QLeNet5(loss_fn=None, **arch)
    detgen.fill_module(model, seed=3)
    with torch.no_grad():
        model.conv2.w_approximate.v1.copy_(P.weight_scales(model.conv2.weight, 'ls-1')[0])
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x = detgen.normal('mnist_ls1w_fpa.x', (64, 1, 28, 28))
    y = RM.lenet_forward(sd, arch, x)
    assert rel_err(y, g7['mnist_ls1w_fpa_logp']) < 1e-6                    # (the functional LeNet is the reference's; bit-equal at its thread count)
    with P.split_operands():
        ys = RM.lenet_forward(sd, arch, x)
    out['fp_lenet_logp'] = {'split': rel_err(ys, y), 'sensitivity': max(rel_err(RM.lenet_forward(sd, arch, perturbed(x, s)), y) for s in range(3))}
    tag = 'imagenet_ls1w_fpa'
    arch = json.loads(bytes(g6[tag + '_arch'].numpy()).decode())
    model = QResNet(loss_fn=None, **arch)
    sd = filled_state_dict(model, 1)
    x = detgen.normal(tag + '.x', (2, 3, 64, 64))
    y = RM.resnet_forward(sd, arch, x)
    assert rel_err(y, g6[tag + '_logits']) < 1e-6
    with P.split_operands():
        ys = RM.resnet_forward(sd, arch, x)
    out['fp_resnet_logits'] = {'split': rel_err(ys, y), 'sensitivity': max(rel_err(RM.resnet_forward(sd, arch, perturbed(x, s)), y) for s in range(3))}
    for v in out.values():
        v['limit'] = 1.05 * v['split'] + 2.0 * v['sensitivity']
        v['formula'] = '1.05 * split + 2 * sensitivity'
    return out


CHAINED = {'chained_cifar_b100': ('cifar', 100, 1), 'chained_cifar_b7': ('cifar', 7, 1), 'chained_imagenet_ls1_b6': ('imagenet_ls1', 6, 2)}


def chained_cases(only=None):
    """The networks of test_chained_one_bit_layers_equal_the_unchained_network (bench.py's models, ls-1 activations: no search,
    integer convolutions): against the oracle's logits of the same model the GPU differs by the fp32 order of operations of the
    stem (MIOpen / lsq_stem_conv_pool), the folded batch norms and the scale sums only: north_star's 1e-4 for that, plus
    2 * sensitivity of the first four samples (the ones the test compares) for what the network does with such noise.
    Observed on the MI355X: 1e-6 (CIFAR, MIOpen 3x3 stem), 4.5e-7 (ImageNet ls-1)."""
    import bench
    out = {}
    for key, (which, batch, seed) in CHAINED.items():
        if only is not None and key not in only:
            continue
        arch = bench.cifar_arch() if which == 'cifar' else bench.imagenet_arch('ls-1', 2)
        model = bench.build_model(arch, torch.device('cpu'))
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        size = 32 if which == 'cifar' else 224
        x = torch.randn(batch, 3, size, size, generator=torch.Generator().manual_seed(seed))[:4]
        y = RM.resnet_forward(sd, arch, x)
        sens = max(rel_err(RM.resnet_forward(sd, arch, perturbed(x, s)), y) for s in range(3))
        out[key] = {'sensitivity': sens, 'limit': TOL + 2.0 * sens,
                    'formula': '1e-4 (north_star\'s bound on a layer: the fp32 stem and scale sums are MIOpen\'s / the kernels\' order of operations, '
                               'not the CPU\'s) + 2 * sensitivity (no search, exact integer convolutions: nothing else to move)'}
    return out


def main():
    torch.set_num_threads(4)
    out = conv_layers()
    blk = block_case()
    for k, v in blk.items():
        v['limit'] = 1.05 * v['tiebreak'] + 2.0 * v['sensitivity']
        v['formula'] = '1.05 * tiebreak + 2 * sensitivity'
    out.update(blk)
    nets = net_cases()
    modular = ('imagenet_ls1w_ls2a', 'imagenet_ls1w_lsTa', 'imagenet_ls1w_gf2a', 'cifar100_ls1')    # test_resnet18_every_layer_and_logits
    fused = ('imagenet_ls1w_ls2a', 'cifar100_ls1', 'imagenet_ls1w_fpa')                              # test_fused_blocks_agree_with_modular_path

    def worst(tags, a, b):
        return max(1.05 * nets[t][a] + 2.0 * nets[t][b] for t in tags)
    out['resnet_logits'] = {'limit': worst(modular, 'tiebreak', 'sensitivity'), 'formula': 'max over configs of 1.05 * tiebreak + 2 * sensitivity'}
    out['resnet_logits_cos'] = {'limit': worst(modular, 'tiebreak_cos', 'sensitivity_cos'), 'formula': out['resnet_logits']['formula']}
    out['fused_logits'] = {'limit': worst(fused, 'tiebreak', 'sensitivity'), 'formula': out['resnet_logits']['formula']}
    out['fused_cos_ref'] = {'limit': worst(fused, 'tiebreak_cos', 'sensitivity_cos'), 'formula': out['resnet_logits']['formula']}
    out['fused_cos_modular'] = {'limit': max(2.0 * nets[t]['sensitivity_cos'] for t in fused),
                                'formula': 'GPU against GPU (same solver on both sides): max over configs of 2 * sensitivity'}
    out['block_cos_modular'] = {'limit': 2.0 * blk['block_cos']['sensitivity'], 'formula': 'GPU against GPU: 2 * sensitivity of the block'}
    out.update(fp_cases())
    out.update(chained_cases())
    for k, v in out.items():
        if 'cos' in k:
            v['limit'] = max(v['limit'], 1e-9)
    doc = {'note': 'limits of the free-running GPU parity assertions, derived on the CPU from the oracle and the reference fixtures '
                   '(tests/golden/make_free_limits.py); tiebreak = exact-argmin oracle against the reference, sensitivity = the '
                   'exact-argmin oracle against itself on an input scaled by (1 + eps), |eps| <= 2^-21',
           'limits': out, 'networks': nets}
    path = os.path.join(HERE, 'free_limits.json')
    with open(path, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    for k, v in sorted(out.items()):
        print(f"{k:24s} limit {v['limit']:.3e}  " + '  '.join(f'{a} {b:.3e}' for a, b in v.items() if a in ('tiebreak', 'sensitivity', 'split')))
    for t, v in nets.items():
        print(t, {a: float('%.3e' % b) for a, b in v.items()})


if __name__ == '__main__':
    main()
