"""``chain.FIXED_SCALES`` through the modules: residual blocks with moving-average activation scales give the same bits with
the consumer's quantizer in the producer's epilogue (lsq_xnor_conv2d_chain_fixed) as with a launch of its own; the record on
an inner tensor; a record voided by an in-place edit of the tensor or by a change of the moving average."""

import pytest
import torch

import detgen

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SCHEMES = ('ls-1', 'ls-2', 'ls-T', 'gf-2')


def _blocks(xq, double_shortcut):
    """Two stride-1 blocks (64 channels) and a stride-2 block with a projection, eval mode, every activation quantizer on
    moving averages that differ from layer to layer."""
    from quant.models import resnet
    clamp = {'kind': 'symmetric', 'alpha': 2}
    blocks = [resnet.XnorBasicBlock(cin, cout, xq, 'ls-1', ['prelu', 'relu'], stride=stride, double_shortcut=double_shortcut,
                                    clamp=clamp, moving_average_mode='eval_only')
              for cin, cout, stride in ((64, 64, 1), (64, 64, 1), (64, 128, 2))]
    for i, b in enumerate(blocks):
        detgen.fill_module(b, seed=20 + i)
        with torch.no_grad():
            for j, conv in enumerate((b.conv1, b.conv2)):
                conv.w_approximate.v1.copy_(conv.weight.abs().mean(dim=(1, 2, 3)))
                avg = conv.x_approximate.moving_avg_module.moving_average
                avg.copy_(torch.tensor([0.9, 0.4])[:avg.numel()] * (1.0 + 0.1 * (2 * i + j)))
    for cur, nxt in zip(blocks, blocks[1:]):
        cur.__dict__['chain_next'] = (nxt.bn1, nxt.conv1)              # (what QResNet sets)
    return [b.eval().to(DEV) for b in blocks]


def _run(blocks, x, on, monkeypatch, between=None):
    """(output of block 0, output of the stack); ``between(out0)`` runs between block 0 and block 1."""
    from quant.binary import chain
    monkeypatch.setattr(chain, 'FIXED_SCALES', on)
    with torch.no_grad():
        first = blocks[0](x)
        rec = chain.pending(first)
        undo = between(first) if between is not None else None
        out = blocks[2](blocks[1](first))
        if undo is not None:
            undo()
    return first, rec, out


@pytest.mark.parametrize('double_shortcut', [False, True])
@pytest.mark.parametrize('xq', SCHEMES)
def test_blocks_give_the_same_bits(xq, double_shortcut, monkeypatch):
    blocks = _blocks(xq, double_shortcut)
    x = detgen.normal('chain_fixed.block.x', (3, 64, 8, 8), scale=1.0).to(DEV)
    first_off, rec_off, off = _run(blocks, x, False, monkeypatch)
    first_on, rec_on, on = _run(blocks, x, True, monkeypatch)
    assert rec_off is None
    assert rec_on is not None and rec_on.consumer is blocks[1].conv1 and rec_on.units is None
    assert torch.equal(rec_on.scales.cpu(), blocks[1].conv1.x_approximate.eval_scales(3).cpu().float())
    assert torch.equal(first_on, first_off) and torch.equal(on, off)
    assert torch.equal(blocks[1].conv1.last_act_scales, rec_on.scales)


def _edit(first):
    first.mul_(-0.5)


def _new_average(blocks):
    def between(first):
        avg = blocks[1].conv1.x_approximate.moving_avg_module.moving_average
        avg.mul_(2.0)
        return lambda: avg.mul_(0.5)                                    # (exact both ways)
    return between


@pytest.mark.parametrize('what', ['tensor_edited', 'average_changed'])
def test_a_stale_record_is_not_used(what, monkeypatch):
    blocks = _blocks('ls-2', True)
    x = detgen.normal('chain_fixed.block.x', (3, 64, 8, 8), scale=1.0).to(DEV)
    between = _edit if what == 'tensor_edited' else _new_average(blocks)
    _, _, plain = _run(blocks, x, False, monkeypatch)
    _, _, off = _run(blocks, x, False, monkeypatch, between)
    _, rec, on = _run(blocks, x, True, monkeypatch, between)
    assert rec is not None and rec.scales is not None
    assert torch.equal(on, off) and not torch.equal(off, plain)
