"""tests/golden/resident_shapes.py on the host (no GPU): the table of shapes that take the row-resident quantizer and the
launcher's conditions are restated there; the statements restated are pinned in the sources here, so a change of the selection
fails this file instead of silently moving a case of tests/test_gpu_quant_resident.py to another kernel."""

import os
import re

import resident_shapes as RS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ml-quant_amd', 'csrc')


def _source(name: str) -> str:
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r'\s+', ' ', f.read())


def test_the_table_restates_the_launcher():
    src = _source('lsq_act_fused.hip')
    rows = ', '.join('{%d, %d, %d}' % s for s in sorted(RS.RESIDENT_SHAPES, key=lambda s: -s[0]))
    for statement in ('static constexpr int kResidentShapes[][3] = {%s};' % rows,
                      'if (a.cg != a.C) return false;',
                      'if (a.win_sh && !(a.debug & 16) && resident_shape(a)) {',
                      'const int e = resident_act_quant(a, vec, need, st);',
                      'const int vec = HW % 2 == 0 ? 2 : 1;',
                      'if (!a.win_sh || a.forced || a.greedy || HW % 3 == 0 || (a.cg & 63) != 0 || a.C > kBnCap || '
                      '(long long)a.Gt * (HW / vec) > T) return kFusedNotEligible;',
                      'if (vec == 1 && vecf == 1 && need <= 5) hipLaunchKernelGGL((aq_resident_kernel<T, 5, 1, 1>)',
                      'else if (vec == 2 && vecf == 4 && need > 5 && need <= 9) hipLaunchKernelGGL((aq_resident_kernel<T, 9, 2, 4>)',
                      'if (HW % 4 == 0 && (items4 <= T || items4 >= 4 * T)) vec = 4;', 'else if (HW % 2 == 0) vec = 2;',
                      'const long long ntrip = (M / 4 + 2) / 3;', 'const long long need = (ntrip + T - 1) / T;',
                      'constexpr int T = 512;', 'constexpr int kBnCap = 1024;'):
        assert statement in src, statement
    assert RS.THREADS == 512 and RS.BN_CAP == 1024


def test_every_gated_shape_has_a_kernel_and_fits_one_item_per_lane():
    for (c, h, w) in RS.RESIDENT_SHAPES:
        kern = RS.resident_kernel(c, h, w)
        assert kern in RS.RESIDENT_KERNELS, (c, h, w, kern)
        u, vec, vecf = kern
        vec_two_read, need = RS.two_read_launch(c, h, w)
        assert vecf == vec_two_read and need <= u                  # the fall-back of single rows is the two-read kernel's own body
        assert (c // 64) * (h * w // vec) <= RS.THREADS and (h * w) % vec == 0 and (h * w) % 3 != 0
        assert 64 * vec <= 128                                     # resident values per lane: well inside 256 VGPRs


def test_cases_of_the_gpu_test_sit_on_both_sides_of_the_selection():
    taken = {case: RS.takes_resident_form(*case[1:]) for case in RS.CASES}
    assert taken == {(3, 512, 7, 7): True, (3, 256, 14, 14): True, (3, 128, 28, 28): False, (2, 64, 14, 14): False,
                     (2, 64, 28, 28): False}
    # 56 x 56 and 28 x 28 keep the two-read kernels whatever the table says: no instantiation takes them
    assert RS.resident_kernel(64, 56, 56) is None and RS.resident_kernel(128, 28, 28) is None
    # the shorter rows: 28 x 28 x 64 would fit an instantiation but is not in the measured table, 14 x 14 x 64 has none
    assert RS.resident_kernel(64, 28, 28) == (9, 2, 4) and RS.resident_kernel(64, 14, 14) is None
    # grouped convolutions and channel counts that are no multiple of 64 are never resident
    assert not RS.takes_resident_form(512, 7, 7, groups=2) and RS.resident_kernel(96, 7, 7) is None
