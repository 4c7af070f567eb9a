"""Cases of the train-mode batch-norm fold (include/lsq_hip_bn_train.h), shared by tests/test_bn_train_host.py,
tests/test_gpu_bn_train.py and tests/test_gpu_bn_train_module.py.  Data only: the tests build their inputs from it.

A case: the shape of x; the activation scheme and its clamp bound (-1: none); whether the batch norm has gamma / beta; its
momentum (None: the cumulative average); ``offset``, the fp32 elements x starts behind a 16-byte boundary.  ``reaches`` says
which path of the kernels the case is there for."""

import collections

Case = collections.namedtuple('Case', 'id N C H W scheme alpha affine momentum offset reaches')

CASES = [
    Case('m2', 2, 3, 1, 1, 'ls-1', 2.0, True, 0.1, 0, 'two values per channel, the fewest torch accepts'),
    Case('odd_hw', 1, 20, 7, 7, 'ls-2', 2.0, False, None, 0, 'H W = 49: 4-byte accesses, one sample'),
    Case('c130', 5, 130, 4, 4, 'gf-3', 1.5, True, 0.1, 0, 'C past one plane word; 16-byte accesses, 64 runs per workgroup'),
    Case('run30', 3, 8, 5, 6, 'ls-T', 2.0, True, None, 0, 'a run of 30: H W % 4 != 0'),
    Case('slabs', 12, 2, 16, 16, 'fp', 2.0, True, 0.1, 0, 'several slabs per channel (the tests read how many)'),
    Case('sliced', 3, 4, 4, 4, 'ls-2', 2.0, False, 0.1, 1, 'H W % 4 == 0 on runs that are not 16-byte aligned'),
    Case('long_run', 2, 3, 33, 32, 'ls-1', -1.0, True, 0.1, 0, 'a run of 264 16-byte accesses: a lane takes more than one'),
]
BY_ID = {c.id: c for c in CASES}

SCHEMES = ('ls-1', 'ls-2', 'ls-T', 'gf-3', 'fp')

# geometry classes of tests/golden/train_step_cases.py the module test runs a bn -> QuantConv2d pair on (each accepted by
# hip_train.supported): the baseline, fp activations on the wide patch kernel with two weight planes, a 5 x 5 kernel with ls-2
# activations, stride 2 with an unread row, the matrix-core XNOR forward, fp activations under the clamp
MODULE_CASES = ('base3x3', 'wide_patch', 'k5_many', 's2_3x5', 'xnor64', 'k1x3_wide')
