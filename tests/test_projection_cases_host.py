"""tests/golden/projection_cases.py on the host (no GPU): the cases of tests/test_gpu_pointwise_variants.py reach every kernel
lsq_pointwise_conv can launch, the added cases of tests/test_gpu_proj_fused.py reach the multi-tile path of the fused kernel, the
integer-grid operands make fp32 exact, and no tensor is large.  ``pointwise_variant`` and ``proj_grid`` restate the entry points'
selection code (a GPU test cannot see which instantiation ran); the statements they restate are pinned in the sources here, so
a change of the selection fails this file instead of silently moving a case to another kernel."""

import os
import re

import pytest
import torch

import projection_cases as PC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ml-quant_amd', 'csrc')


def _source(name: str) -> str:
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r'\s+', ' ', f.read())


# ---------------------------------------------------------------------------------------------------- lsq_pointwise_conv
def test_pointwise_cases_reach_every_kernel():
    assert len(PC.ALL_VARIANTS) == 17
    reached = {PC.pointwise_variant(*case) for case, _ in PC.PW_CASES}
    assert reached == PC.ALL_VARIANTS, sorted(PC.ALL_VARIANTS - reached)


@pytest.mark.parametrize('case, variant', PC.PW_CASES, ids=[PC.pw_id(c) for c, _ in PC.PW_CASES])
def test_pointwise_case_reaches_the_variant_it_was_chosen_for(case, variant):
    assert PC.pointwise_variant(*case) == variant
    assert (PC.generic_routes(*case) != frozenset()) == (variant == ('generic',))
    n, c, h, w, o, stride = case
    assert c % 64 == 0 and o % 64 == 0 and c <= PC.MAX_CHANNELS      # (what the entry point admits; what keeps the grid sums exact)


def test_generic_kernel_is_reached_by_each_route_alone():
    routes = [PC.generic_routes(*case) for case, variant in PC.PW_CASES if variant == ('generic',)]
    for route in ('not_pow2', 'o_gt_512', 'pair_refused'):
        assert frozenset({route}) in routes, route
    # the refusal of the pair load: stride 2, an even output width, an odd input width
    refused = [case for case, _ in PC.PW_CASES if PC.generic_routes(*case) == {'pair_refused'}]
    assert all(s == 2 and PC.out_size(w, s) % 2 == 0 and w % 2 == 1 for (n, c, h, w, o, s) in refused)


def test_pointwise_cases_cover_the_chunk_counts_and_both_strides():
    assert {64, 128, 192, 320, 512} <= {case[1] for case, _ in PC.PW_CASES}
    for n_ot in (1, 2, 4, 8):             # per NOT: a stride-2 case without the pair loads (odd Wo); overall: stride 1 and 3
        assert any(v[:3] == ('all', n_ot, False) and case[5] == 2 for case, v in PC.PW_CASES)
    assert {1, 2, 3} <= {case[5] for case, _ in PC.PW_CASES}
    # a partial last 64-pixel tile in every all-tiles variant's VEC4 = false case, and images that end inside a tile
    for case, v in PC.PW_CASES:
        n, c, h, w, o, s = case
        if v[0] == 'all' and not v[3]:
            assert (n * PC.out_size(h, s) * PC.out_size(w, s)) % 64 != 0, case


def test_pointwise_variant_restates_the_entry_point():
    src = _source('lsq_pointwise.hip')
    for statement in ('a.Ho = (H - 1) / stride + 1;', 'a.Wo = (W - 1) / stride + 1;', 'const long long blocks = (a.P + 63) / 64;',
                      'const int n_ot = O / 64;', 'const bool pair_ok = stride != 2 || (a.Wo & 1) || (W & 1) == 0;',
                      'if (n_ot <= 8 && (n_ot & (n_ot - 1)) == 0 && pair_ok) {', 'long long min_wgs = 256;',
                      'while (per_wg > 1 && blocks * (n_ot / per_wg) < min_wgs) per_wg >>= 1;',
                      'const bool vec4 = ((a.Ho * a.Wo) & 3) == 0;', 'if (a.s == 2 && (a.Wo & 1) == 0 && a.P >= 2) {'):
        assert statement in src, statement


# -------------------------------------------------------------------------------------------------- lsq_xnor_conv2d_proj
def _grid(case):
    ho, wo = PC.fused_out_hw(case)
    return PC.proj_grid(case[0], ho, wo, case[4])


def test_fused_cases_reach_the_multi_tile_path():
    grids = {name: _grid(case) for name, case in PC.FUSED_CASES.items()}
    for o in (128, 256, 512):
        assert any(case[4] == o and grids[name][3] >= 2 for name, case in PC.FUSED_CASES.items()), o
    assert any(most >= 3 for _, _, _, most in grids.values())
    assert any(fewest != most for _, _, fewest, most in grids.values())
    assert all(most >= 2 for _, _, _, most in grids.values())
    partial = {name for name, case in PC.FUSED_CASES.items() if (case[0] * PC.fused_out_hw(case)[0] * PC.fused_out_hw(case)[1]) % 32}
    assert PC.FUSED_PARTIAL in partial
    # a wave's step from tile to tile, 32 x waves pixels, spans more than one whole image: d_n > 1 in the kernel's advance()
    assert any(32 * grids[name][1] > 2 * PC.fused_out_hw(case)[0] * PC.fused_out_hw(case)[1] for name, case in PC.FUSED_CASES.items())
    assert grids['o512_140t'][:2] == (140, 128) and grids['o512_274t'] == (274, 128, 2, 3) and grids['o256_264t'][:2] == (264, 256)
    assert grids['o128_526t'][:2] == (526, 512) and grids['o512_c512_s1'][:2] == (138, 128)
    assert set(PC.FUSED_ANCHORED) <= set(PC.FUSED_CASES) and PC.FUSED_BOTH_SCHEMES in PC.FUSED_CASES
    assert any(case[1] != case[5] for case in PC.FUSED_CASES.values())              # Cp != C
    assert any(case[3] == 1 for case in PC.FUSED_CASES.values())                    # a stride-1 consumer


def test_proj_grid_on_the_existing_cases_is_one_tile_per_wave():
    """What the added cases are for: the five shapes tests/test_gpu_proj_fused.py had give gx = 1 and at most one tile per wave."""
    for n, ho, wo, o in ((3, 6, 6, 128), (2, 5, 3, 256), (1, 4, 4, 512), (5, 4, 4, 512), (2, 6, 6, 64)):
        tiles, waves, fewest, most = PC.proj_grid(n, ho, wo, o)
        assert waves == 8 and most == 1 and tiles <= 8


def test_cp_cases_cover_every_admitted_cp():
    assert {case[5] for case in PC.CP_CASES.values()} == set(range(64, 513, 64))
    assert PC.CP_CASES['c512_cp512'][1] == 512 and PC.CP_CASES['c512_cp512'][5] == 512
    for case in list(PC.CP_CASES.values()) + list(PC.FUSED_CASES.values()):
        n, c, (h, w), s, o, cp, (hx, wx) = case
        assert (PC.out_size(hx, 2), PC.out_size(wx, 2)) == PC.fused_out_hw(case)     # the projection lands on the consumer's pixels
        assert c in (64, 128, 256, 512) and cp % 64 == 0 and cp <= PC.MAX_CHANNELS and o % 32 == 0


def test_proj_grid_restates_launch_proj():
    src = _source('lsq_xnor_mfma.hip')
    for statement in ('#define LSQ_PROJ_SHAPE 8, 2', 'const long long ntiles = ((long long)a.N * a.Ho * a.Wo + 31) >> 5; '
                      'const int n_ot = a.O / 32; long long gx = (256 + n_ot - 1) / n_ot; '
                      'if (gx * NWAVES > ntiles) gx = (ntiles + NWAVES - 1) / NWAVES;',
                      'const int tstride = gridDim.x * NWAVES;', 'int tile = wid * gridDim.x + blockIdx.x;',
                      'const int nxt = tile + tstride;'):
        assert statement in src, statement
    assert PC.PROJ_WAVES == 8


# ------------------------------------------------------------------------------------------------------------ the operands
def test_grid_operands_are_integers_in_range_and_fp32_is_exact():
    c = max(case[1] for case, _ in PC.PW_CASES)
    assert c == PC.MAX_CHANNELS == max(case[5] for case in PC.CP_CASES.values())
    x = PC.grid_operands('pc.host.x', (96, c), *PC.X_RANGE)
    w = PC.grid_operands('pc.host.w', (c, 128), *PC.W_RANGE)
    b = PC.grid_operands('pc.host.b', (128,), *PC.B_RANGE)
    for t, (lo, hi) in ((x, PC.X_RANGE), (w, PC.W_RANGE), (b, PC.B_RANGE)):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and lo <= float(t.min()) and float(t.max()) <= hi
    assert (float(x.min()), float(x.max())) == PC.X_RANGE and (float(w.min()), float(w.max())) == PC.W_RANGE
    assert PC.X_RANGE[1] * PC.W_RANGE[1] * c + PC.B_RANGE[1] < 2 ** 15
    exact = x.double() @ w.double() + b.double()
    assert torch.equal(x @ w + b, exact.float()) and torch.equal(exact.float().double(), exact)
    # any order: the channels reversed and summed one by one
    acc = torch.zeros((96, 128))
    for k in reversed(range(c)):
        acc = acc + x[:, k:k + 1] * w[k:k + 1]
    assert torch.equal(acc + b, exact.float())
    assert torch.equal(PC.grid_operands('pc.host.x', (96, c), *PC.X_RANGE), x)        # seeded: the same tensor every time


def test_no_tensor_of_a_case_is_large():
    for case, _ in PC.PW_CASES:
        assert max(PC.pw_bytes(*case).values()) < PC.MAX_TENSOR_BYTES, case
    for name, case in {**PC.FUSED_CASES, **PC.CP_CASES}.items():
        assert max(PC.fused_bytes(case).values()) < PC.MAX_TENSOR_BYTES, name
