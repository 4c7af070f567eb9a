"""tests/golden/proj_half_cases.py and the table row of liblsq_hip_conv_proj_half.so on the host (no GPU, no built library).

  * the anchor property of the small integer grid: for every shape of projection_cases.PW_CASES the exact projection is an
    integer of magnitude at most 256, so it -- and every operand -- survives the round trip through bf16 and through fp16
    unchanged: on the GPU the 16-bit result must EQUAL it;
  * the sub-library's header, table row and Makefile agree (tests/test_sublib_table_host.py does this generically; here the
    names the issue fixes are spelled out);
  * kernel selection: the one rule lsq_pointwise_conv_half adds to lsq_pointwise_conv's, the alignment fallback, is restated in
    proj_half_cases.half_variant and pinned in the source; which variant every case reaches is shown for aligned tensors (the
    fp32 mirror's) and for tensors that start one element into a storage."""

import os
import re

import pytest
import torch

import proj_half_cases as PH
import projection_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ml-quant_amd', 'csrc')


def _read(*parts) -> str:
    with open(os.path.join(*parts)) as f:
        return f.read()


def _exact(case):
    """The projection of a case's grid operands in fp64: a strided slice and one matmul per image."""
    n, c, h, w, o, stride = case
    x, wt, b = PH.grid_operands(case)
    xs = x[:, :, ::stride, ::stride].double()
    ho, wo = xs.shape[2:]
    y = torch.matmul(wt.double(), xs.reshape(n, c, ho * wo)).reshape(n, o, ho, wo) + b.double().view(1, -1, 1, 1)
    return x, wt, b, y


@pytest.mark.parametrize('case', [c for c, _ in PC.PW_CASES], ids=[PC.pw_id(c) for c, _ in PC.PW_CASES])
def test_the_anchor_is_exact_in_both_types(case):
    x, wt, b, y = _exact(case)
    for t, (lo, hi) in ((x, PH.X_RANGE), (wt, PH.W_RANGE), (b, PH.B_RANGE)):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and lo <= float(t.min()) and float(t.max()) <= hi
    assert float(y.abs().max()) <= PH.ANCHOR_MAX
    assert torch.equal(y, y.round()) and torch.equal(y.float().double(), y)
    for dtype in (torch.bfloat16, torch.float16):
        assert torch.equal(y.float().to(dtype).double(), y), dtype           # the 16-bit rounding of the result is the identity
        assert torch.equal(x.to(dtype).float(), x), dtype                    # and the input converts exactly
    # the bound does not rest on luck: |x| |w| C + |b| may exceed it, the seeded sums do not
    assert PH.X_RANGE[1] * PH.W_RANGE[1] * case[1] + PH.B_RANGE[1] >= float(y.abs().max())


def test_every_integer_up_to_the_anchor_bound_is_a_value_of_both_types():
    ints = torch.arange(-PH.ANCHOR_MAX, PH.ANCHOR_MAX + 1, dtype=torch.float32)
    for dtype in (torch.bfloat16, torch.float16):
        assert torch.equal(ints.to(dtype).float(), ints)
    assert float(torch.tensor(257.0).to(torch.bfloat16)) != 257.0            # (the bound is bf16's, not a loose one)


def test_the_operands_are_seeded_and_tagged_per_case():
    case = PC.PW_CASES[15][0]
    assert case == (3, 64, 8, 8, 64, 2)
    a, b = PH.grid_operands(case), PH.grid_operands(case)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert torch.equal(a[0], PC.grid_operands('projh.3x64x8x8x64s2.x', (3, 64, 8, 8), *PH.X_RANGE))
    assert torch.equal(a[1], PC.grid_operands('projh.3x64x8x8x64s2.w', (64, 64), *PH.W_RANGE))
    assert torch.equal(a[2], PC.grid_operands('projh.3x64x8x8x64s2.b', (64,), *PH.B_RANGE))


# ------------------------------------------------------------------------------------------------- the sub-library's row
def test_the_table_row_the_header_and_the_makefile_agree():
    from quant import _hip, _sublibs
    s = _sublibs.BY_DIR['conv_proj_half']
    assert _sublibs.soname(s) == 'liblsq_hip_conv_proj_half.so' and s.header == 'lsq_hip_conv_proj_half.h'
    assert s.version_symbol == 'lsq_conv_proj_half_abi_version' and s.version == 1
    assert list(s.prototypes) == ['lsq_conv_proj_half_abi_version', 'lsq_pointwise_conv_half', 'lsq_xnor_conv2d_proj_half']
    header = _read(ROOT, 'include', s.header)
    assert re.search(r'#define\s+LSQ_CONV_PROJ_HALF_ABI_VERSION\s+1\b', header)
    for symbol in s.prototypes:
        assert re.search(r'\b' + symbol + r'\s*\(', header), symbol
        assert re.fullmatch(s.pattern, symbol), symbol
    # lsq_proj_half: lsq_proj's fields, x untyped
    body = re.search(r'typedef struct lsq_proj_half \{(.*?)\} lsq_proj_half;', header, flags=re.S).group(1)
    assert re.search(r'const void\*\s*x;', body)
    fields = [n for n, _ in _sublibs.ProjHalf._fields_]
    assert fields == [n for n, _ in _sublibs.Proj._fields_] == ['x', 'w', 'bias', 'C', 'H', 'W', 'stride', 'post']
    assert [t for _, t in _sublibs.ProjHalf._fields_] == [t for _, t in _sublibs.Proj._fields_]
    # the header says that the fused call rounds once and the two launches round the shortcut first
    flat = re.sub(r'[\s*]+', ' ', header)
    assert 'rounds once' in flat and 'rounds the shortcut to 16 bits first' in flat and 'NOT bit-equal' in flat
    mk = _read(CSRC, 'conv_proj_half', 'Makefile')
    assert re.search(r'^NAME := conv_proj_half$', mk, flags=re.M) and 'include ../sublib.mk' in mk and '-llsq_hip' in mk
    assert re.search(r'^SRCS := lsq_conv_proj_half\.hip$', mk, flags=re.M)
    assert os.path.exists(os.path.join(CSRC, 'conv_proj_half', 'lsq_conv_proj_half.hip'))
    assert _hip.CONV_PROJ_HALF_ABI_VERSION == 1 and callable(_hip.conv_proj_half_lib)
    assert _hip.conv_proj_half_library_path() == os.path.join(ROOT, 'ml-quant_amd', 'lib', 'liblsq_hip_conv_proj_half.so')
    assert callable(_hip.pointwise_conv_half) and callable(_hip.xnor_conv2d_proj_half)


def test_the_sub_library_has_no_kernel_of_its_own():
    src = _read(CSRC, 'conv_proj_half', 'lsq_conv_proj_half.hip')
    assert '__global__' not in src and 'hipLaunchKernelGGL' not in src and '<<<' not in src
    assert 'lsq::pointwise_conv_half(' in src and 'lsq::xnor_conv2d_proj_half(' in src


# ---------------------------------------------------------------------------------------------------- kernel selection
def _flat(name: str) -> str:
    return re.sub(r'\s+', ' ', _read(CSRC, name))


def test_selection_is_one_function_for_every_element_type_plus_the_alignment_rule():
    src = _flat('lsq_pointwise.hip')
    # one templated host function holds the selection statements tests/test_projection_cases_host.py pins, once
    for statement in ('const bool pair_ok = stride != 2 || (a.Wo & 1) || (W & 1) == 0;',
                      'if (n_ot <= 8 && (n_ot & (n_ot - 1)) == 0 && pair_ok) {',
                      'while (per_wg > 1 && blocks * (n_ot / per_wg) < min_wgs) per_wg >>= 1;',
                      'const bool vec4 = ((a.Ho * a.Wo) & 3) == 0;', 'if (a.s == 2 && (a.Wo & 1) == 0 && a.P >= 2) {'):
        assert src.count(statement) == 1, statement
    assert 'return pointwise_conv(x, N, C, H, W, w, bias, O, stride, y, stream);' in src          # lsq_pointwise_conv forwards to it
    # the addition: wide accesses only where the pointers allow them
    for statement in ('const bool x_wide = sizeof(T) == 4 || (reinterpret_cast<uintptr_t>(a.x) & 3) == 0;',
                      'const bool y_wide = sizeof(T) == 4 || (reinterpret_cast<uintptr_t>(a.y) & 7) == 0;',
                      'if (x_wide) launch_vec<NOT, true>(a, grid, st, vec4 && y_wide); '
                      'else launch_vec<NOT, false>(a, grid, st, vec4 && y_wide);'):
        assert statement in src, statement


def test_the_fused_kernel_admits_a_projection_with_16_bit_io():
    src = _flat('lsq_xnor_mfma.hip')
    assert 'static_assert(kF32 || (FP4 && !CHAIN), ' in src and '!CHAIN && !PROJ' not in src
    assert 'xnor_mfma_kernel<2, GG, 9, NWAVES, WPC, false, true, true, T>' in src
    assert '#define LSQ_PROJ_SHAPE 8, 2' in src                                  # the launch shape stays launch_proj's


@pytest.mark.parametrize('case, variant', PC.PW_CASES, ids=[PC.pw_id(c) for c, _ in PC.PW_CASES])
def test_the_variant_every_case_reaches(case, variant):
    assert PH.half_variant(case) == variant == PC.pointwise_variant(*case)         # aligned tensors: the fp32 selection
    off = PH.half_variant(case, x_addr=2, y_addr=2)                                # one element into a storage
    assert off == (variant if variant == ('generic',) else ('all', variant[1], False, False))
    assert PH.half_variant(case, x_addr=4, y_addr=4) == (variant if variant == ('generic',) else variant[:3] + (False,))
    assert PH.half_variant(case, x_addr=2, y_addr=8) == (variant if variant == ('generic',) else variant[:2] + (False, variant[3]))


def test_aligned_cases_reach_every_kernel_and_the_unaligned_cases_are_what_they_claim():
    assert {PH.half_variant(case) for case, _ in PC.PW_CASES} == PC.ALL_VARIANTS
    pairs_vec4, no_pairs = PH.UNALIGNED_CASES
    assert PH.half_variant(pairs_vec4) == ('all', 1, True, True) and PH.half_variant(pairs_vec4, 2, 2) == ('all', 1, False, False)
    smaller = [c for c, v in PC.PW_CASES if v[0] == 'all' and v[2] and v[3]
               and max(PC.pw_bytes(*c).values()) < max(PC.pw_bytes(*pairs_vec4).values())]
    assert not smaller                                                            # the smallest PAIRS + VEC4 case
    assert PH.half_variant(no_pairs)[:3] == ('all', 1, False)
    assert all(c in [k for k, _ in PC.PW_CASES] for c in PH.UNALIGNED_CASES)
