"""Which activation shapes the single-launch ls-2 / ls-T quantizer takes in its row-resident form (one read of the row, its
clamped values in registers from the load to the last plane word; csrc/lsq_act_fused.hip, Impl::run_resident) -- restated from
the host launcher for tests/test_quant_resident_host.py, which pins the statements restated here in the sources, and for
tests/test_gpu_quant_resident.py, which needs to know which kernel a case reaches (a GPU test cannot see that)."""

THREADS = 512
BN_CAP = 1024

#: (C, H, W), one group: fused_act_quant's kResidentShapes -- the shapes whose launches measured faster in the kernel trace
RESIDENT_SHAPES = frozenset({(512, 7, 7), (256, 14, 14)})

#: (U, VEC, VECF) of the aq_resident_kernel instantiations resident_act_quant can launch
RESIDENT_KERNELS = frozenset({(5, 1, 1), (9, 2, 4)})

#: (N, C, H, W) of the GPU test: the three ResNet-18 row shapes below 56 x 56 and two shorter rows of the same H W
CASES = ((3, 512, 7, 7), (3, 256, 14, 14), (3, 128, 28, 28), (2, 64, 14, 14), (2, 64, 28, 28))


def two_read_launch(c, h, w, groups=1):
    """(vec, need) of fused_act_quant's own launch: pixels per lane of pass 2 and key triples per lane of pass 1."""
    hw, m = h * w, c * h * w
    gt = groups * ((c // groups + 63) // 64)
    vec = 1
    items4 = gt * (hw // 4)
    if hw % 4 == 0 and (items4 <= THREADS or items4 >= 4 * THREADS):
        vec = 4
    elif hw % 2 == 0:
        vec = 2
    ntrip = (m // 4 + 2) // 3
    return vec, (ntrip + THREADS - 1) // THREADS


def resident_kernel(c, h, w, groups=1):
    """The (U, VEC, VECF) resident_act_quant launches for a shape under a symmetric clamp, or None (kFusedNotEligible)."""
    hw, cg = h * w, c // groups
    gt = groups * ((cg + 63) // 64)
    vecf, need = two_read_launch(c, h, w, groups)
    vec = 2 if hw % 2 == 0 else 1
    if hw % 3 == 0 or cg % 64 != 0 or c > BN_CAP or gt * (hw // vec) > THREADS:
        return None
    if vec == 1 and vecf == 1 and need <= 5:
        return (5, 1, 1)
    if vec == 2 and vecf == 4 and 5 < need <= 9:
        return (9, 2, 4)
    return None


def takes_resident_form(c, h, w, groups=1):
    """fused_act_quant's choice for a windowed (symmetric-clamp) ls-2 / ls-T launch with lsq_debug_fused_mode 0."""
    return groups == 1 and (c, h, w) in RESIDENT_SHAPES and resident_kernel(c, h, w, groups) is not None
