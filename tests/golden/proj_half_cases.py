"""Cases and operands of the 16-bit projection-shortcut tests, shared by tests/test_proj_half_host.py (which proves the anchor
property on the host) and tests/test_gpu_proj_half.py (lsq_pointwise_conv_half, lsq_xnor_conv2d_proj_half).

The shapes are those of tests/golden/projection_cases.py: kernel selection in lsq_pointwise_conv_half is the same function of
(N, C, H, W, O, stride) as in lsq_pointwise_conv, so ``projection_cases.pointwise_variant`` keeps describing which kernel a case
launches -- with one addition, the alignment fallback restated in ``half_variant`` below.

The exact anchor.  With x in [-2, 2], w in [-1, 1], bias in [-8, 8] (integers) and at most 512 channels every partial sum of
sum_c w x + b is an integer, and the results of all PW_CASES stay at or below 256 in magnitude (tests/test_proj_half_host.py
asserts it; the worst is 97).  Integers up to 256 are exactly representable in bf16 (8 significand bits: every integer up to
2^8) and in fp16 (11 bits), so the 16-bit rounding of the result is the identity and the operands themselves convert exactly: a
single wrong product cannot hide in the rounding.  The [-8, 8] x [-4, 4] grid of projection_cases is not used for this: its
results reach thousands, where bf16 is spaced 16 apart or more."""

import projection_cases as PC

X_RANGE, W_RANGE, B_RANGE = (-2, 2), (-1, 1), (-8, 8)
ANCHOR_MAX = 256            # every integer of at most this magnitude is a bf16 and an fp16 value


def grid_operands(case):
    """(x [N, C, H, W], w [O, C], bias [O]) of a PW_CASES shape on the small integer grid, fp32; tags projh.<pw_id>.x / .w / .b."""
    n, c, h, w, o, stride = case
    tag = 'projh.' + PC.pw_id(case)
    return (PC.grid_operands(tag + '.x', (n, c, h, w), *X_RANGE), PC.grid_operands(tag + '.w', (o, c), *W_RANGE),
            PC.grid_operands(tag + '.b', (o,), *B_RANGE))


def half_variant(case, x_addr: int = 0, y_addr: int = 0):
    """The kernel lsq_pointwise_conv_half launches for a case whose x and y start at these byte addresses: the variant of
    ``projection_cases.pointwise_variant`` except that the 8-byte pair load needs x 4-byte aligned and the 8-byte store y 8-byte
    aligned (csrc/lsq_pointwise.hip, launch_all: ``x_wide``, ``y_wide``); the generic kernel has scalar accesses only."""
    v = PC.pointwise_variant(*case)
    if v == ('generic',):
        return v
    return ('all', v[1], v[2] and x_addr % 4 == 0, v[3] and y_addr % 8 == 0)


# the two cases of the alignment test: the smallest PAIRS + VEC4 case and one without pair loads
UNALIGNED_CASES = ((3, 64, 8, 8, 64, 2), (2, 128, 10, 6, 256, 2))
