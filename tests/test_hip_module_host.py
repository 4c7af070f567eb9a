"""quant.binary.hip_module / hip_train_common on the host (no GPU, CPU tensors): the workspace retention policy and the
cache invalidation hooks ``QuantConv2d`` and ``QuantLinear`` share, and the call sequence of the train steps' activation
quantization against a recording fake of the binding."""

import pytest
import torch
import torch.nn as nn

from quant import _hip
from quant.binary import QuantLinear
from quant.binary.binary_conv import QuantConv2d
from quant.binary.hip_train_common import step_act_quant

CLAMP = {'kind': 'symmetric', 'alpha': 2}
MAKE = {'conv': lambda xs='ls-2', mode='off': QuantConv2d(xs, 'ls-1', 4, 6, 3, CLAMP, mode, padding=1),
        'linear': lambda xs='ls-2', mode='off': QuantLinear(xs, 'ls-1', 8, 6, CLAMP, mode)}


@pytest.mark.parametrize('kind', list(MAKE))
def test_a_kind_keeps_the_new_entry_and_the_three_inserted_before_it(kind):
    m = MAKE[kind]()
    m._hip_cache['w'] = packed = object()
    other = m._workspace('sup', (0,), object)
    made = []

    def make():
        made.append(object())
        return made[-1]

    for i in range(1, 7):
        assert m._workspace('act', (i, 'stream'), make) is made[-1] and len(made) == i
        held = [k for k in m._hip_cache if isinstance(k, tuple) and k[0] == 'act']
        assert held == [('act', j, 'stream') for j in range(max(1, i - 3), i + 1)]
        assert m._workspace('act', (i, 'stream'), make) is made[i - 1] and len(made) == i      # a hit: same object, no make()
        assert m._hip_cache['w'] is packed and m._hip_cache[('sup', 0)] is other
    assert m._workspace('act', (1, 'stream'), make) is not made[0]                                 # evicted: made again
    assert len(made) == 7


@pytest.mark.parametrize('kind', list(MAKE))
def test_every_invalidation_hook_empties_the_cache(kind):
    m = MAKE[kind]()

    def fill():
        m._hip_cache['w'] = object()
        m._workspace('act', (1,), object)

    fill()
    assert m.eval() is m and len(m._hip_cache) == 2          # eval() keeps packed weights and workspaces
    assert m.train(False) is m and len(m._hip_cache) == 2
    m.train(True)
    assert m._hip_cache == {}
    fill()
    m.load_state_dict(MAKE[kind]().state_dict())
    assert m._hip_cache == {}
    for cast in (nn.Module.double, nn.Module.float):
        fill()
        assert cast(m) is m and m._hip_cache == {}
    fill()
    replica = m._replicate_for_data_parallel()
    assert replica._hip_cache == {} and replica._hip_cache is not m._hip_cache and len(m._hip_cache) == 2
    assert type(m._hip_cache) is dict


class _RecordingHip:
    """Stands in for quant._hip: ``act_quant`` records its ``forced`` argument and writes known scales."""

    def __init__(self, solved):
        self.solved, self.forced = solved, []

    def act_quant(self, x, geom, scheme, k, skip, alpha, planes, scales, forced=None, pre=None):
        assert (scheme, k, skip, alpha, pre) == (self.scheme, self.solved.shape[0], 3, 2.0, None)
        self.forced.append(None if forced is None else forced.clone())
        scales.copy_(self.solved if forced is None else forced)


def _step(kind, xs, mode, forced=None):
    m = MAKE[kind](xs, mode)
    xq, n = m.x_approximate, 5
    xq._forced_scales = forced
    tracked = []
    xq.moving_avg_module.register_forward_pre_hook(lambda mod, args: tracked.append(args[0].clone()))
    fake = _RecordingHip(torch.arange(1, 1 + xq.n_planes * n, dtype=torch.float32).view(xq.n_planes, n) / 8)
    fake.scheme = xq.hip_scheme
    c = 4 if kind == 'conv' else 8
    geom = _hip.make_geom(n, c, 1, 1, 6, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    xscales = step_act_quant(m, torch.zeros((n, c, 1, 1)), geom, torch.zeros(xq.n_planes, dtype=torch.int64), fake)
    return xq, fake, tracked, xscales, n


@pytest.mark.parametrize('xs', ('ls-2', 'ls-T'))
@pytest.mark.parametrize('kind', list(MAKE))
def test_step_quantization_call_sequence(kind, xs):
    xq, fake, tracked, xscales, n = _step(kind, xs, 'off')
    assert fake.forced == [None] and tracked == [] and torch.equal(xscales, fake.solved)

    xq, fake, tracked, xscales, n = _step(kind, xs, 'eval_only')
    mean = fake.solved[:xq.num_scaling_factors].mean(1)
    assert fake.forced == [None] and len(tracked) == 1 and torch.equal(tracked[0], mean)
    assert torch.equal(xscales, fake.solved)                 # trained on the batch's own scales

    xq, fake, tracked, xscales, n = _step(kind, xs, 'train_and_eval')
    assert len(fake.forced) == 2 and fake.forced[0] is None and len(tracked) == 1 and torch.equal(tracked[0], mean)
    want = xq.plane_scales(xq.moving_avg_module.moving_average.view(-1, 1).expand(-1, n))
    assert torch.equal(xq.moving_avg_module.moving_average, mean)          # (the first update copies the batch mean)
    assert fake.forced[1].shape == (xq.n_planes, n) and torch.equal(fake.forced[1], want) and torch.equal(xscales, want)

    given = torch.full((xq.num_scaling_factors, n), 0.75)
    for mode in ('off', 'train_and_eval'):
        xq, fake, tracked, xscales, n = _step(kind, xs, mode, forced=given)
        assert len(fake.forced) == 1 and torch.equal(fake.forced[0], xq.plane_scales(given)) and tracked == []
        assert torch.equal(xscales, xq.plane_scales(given))


@pytest.mark.parametrize('wgrad', (False, True))
@pytest.mark.parametrize('xs', ('ls-2', 'fp'))
def test_both_train_step_forwards_run_against_a_stubbed_binding(xs, wgrad, monkeypatch):
    """The whole forward of ``_QuantConv2dStep`` and ``_QuantLinearStep`` on CPU tensors, the binding's launches stubbed:
    the module's train-step workspace is used unless the convolution's planes belong to the step (``WGRAD_KERNEL``)."""
    from quant.binary import hip_train, hip_train_linear
    monkeypatch.setattr(hip_train, 'WGRAD_KERNEL', wgrad)
    monkeypatch.setattr(hip_train_linear, 'WGRAD_KERNEL', wgrad)
    monkeypatch.setattr(_hip, 'stream_ptr', lambda device=None: 0)
    monkeypatch.setattr(_hip, 'act_plane_words', lambda geom: 4)
    monkeypatch.setattr(_hip, 'act_quant', lambda x, g, s, k, skip, a, planes, scales, forced=None, pre=None: scales.fill_(0.5))
    monkeypatch.setattr(_hip, 'pack_weight', lambda w, g, sc: (torch.zeros(4, dtype=torch.int64),
                                                               torch.zeros((sc.shape[0], g.O, g.KH * g.KW), dtype=torch.int32)))
    monkeypatch.setattr(_hip, 'xnor_conv2d', lambda *a, **k: None)
    monkeypatch.setattr(_hip, 'signw_conv2d', lambda *a, **k: None)
    monkeypatch.setattr(_hip, 'linear_xnor', lambda planes, k, xsc, t, wb, wsum, wsc, b, m, f, o: torch.zeros(m, o))
    monkeypatch.setattr(_hip, 'linear_signw', lambda x, a, wb, wsc, b, m, f, o: torch.zeros(m, o))
    conv, lin = MAKE['conv'](xs), MAKE['linear'](xs)
    assert hip_train.train_step_forward(conv, torch.randn(2, 4, 5, 5, requires_grad=True)).shape == (2, 6, 5, 5)
    assert hip_train_linear.train_step_forward(lin, torch.randn(2, 3, 8, requires_grad=True)).shape == (2, 3, 6)
    kinds = [[kk[0] for kk in m._hip_cache if isinstance(kk, tuple)] for m in (conv, lin)]
    binary = xs != 'fp'
    assert kinds == [['train_planes'] * (binary and not wgrad), ['train_planes'] * binary]
