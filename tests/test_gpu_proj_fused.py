"""lsq_xnor_conv2d_proj (include/lsq_hip_conv_proj.h; csrc/lsq_xnor_mfma.hip, the PROJ instantiations): the XNOR convolution
that computes the projection shortcut of a down-sampling block in its residual registers.

Reference: the two launches it replaces, lsq_pointwise_conv followed by lsq_xnor_conv2d with the projection's output as the
residual tensor.  The fused kernel runs the same chain of fp32 MFMAs on the same operand pairs and the same epilogue, so every
comparison is torch.equal -- no tolerance.  CASES are the smallest shapes with tiles of 32 pixels that straddle images, a partial
last tile, 4 / 8 / 16 out-channel tiles, 1 / 2 / 4 chunks of 64 projection channels, and a stride-1 consumer of a stride-2
projection; every one of them launches ONE workgroup per out-channel tile, so no wave of theirs sees a second tile.

The wave that walks on to a second and third tile (advance(), the next tile's request, xo / yoff and the gather recomputed), every
projection channel count 64 .. 512 (odd step counts of the ping-pong gather; C = Cp = 512, the largest LDS request) and Cp != C
are the cases of tests/golden/projection_cases.py (FUSED_CASES, CP_CASES; tests/test_projection_cases_host.py proves what they
launch).  Besides the two launches they are held to an anchor that does not involve lsq_pointwise_conv: with integer-grid
projection operands the shortcut is exact in fp64 and as fp32 in any summation order, and the fused result must equal the plain
lsq_xnor_conv2d output combined with it by the epilogue's own single fp32 operations."""

import pytest
import torch

import detgen
import projection_cases as PC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
LS2, LST = 2, 3

# name: (N, consumer C, consumer input H x W, consumer stride, O, projection Cp, projection input H x W)
CASES = {
    'c64_o128': (3, 64, (12, 12), 2, 128, 64, (12, 12)),       # 108 pixels: tiles straddle images, the last one is partial
    'c128_o256': (2, 128, (10, 6), 2, 256, 128, (10, 6)),      # odd Wo, 30 pixels: one partial tile
    'c256_o512_n1': (1, 256, (8, 8), 2, 512, 256, (8, 8)),     # 16 pixels, 16 out-channel tiles
    'c256_o512_n5': (5, 256, (8, 8), 2, 512, 256, (8, 8)),     # 80 pixels: several tiles
    'c64_o64_pre': (2, 64, (6, 6), 1, 64, 64, (12, 12)),       # stride-1 consumer, projection input at stride 2
}


def _hip():
    from quant import _hip
    return _hip


ALL_CASES = {**CASES, **PC.FUSED_CASES, **PC.CP_CASES}
MARGIN = 256            # floats on either side of a guarded output


def _operands(name, scheme, grid=False):
    """grid: the projection's x, w and bias on the integer grid of projection_cases.grid_operands (the shortcut is then exact)."""
    hip = _hip()
    n, c, (h, w), s, o, cp, (hx, wx) = ALL_CASES[name]
    geom = hip.make_geom(n, c, h, w, o, 3, 3, (s, s), (1, 1), (1, 1), 1)
    x = detgen.normal(f'proj.{name}.x', (n, c, h, w), scale=1.2).to(DEV)
    planes = torch.zeros((2 * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xs = torch.empty((2, n), dtype=torch.float32, device=DEV)
    hip.act_quant(x, geom, scheme, 2, 3, 2.0, planes, xs)
    wt = detgen.uniform(f'proj.{name}.w', (o, c, 3, 3), -0.5, 0.5).to(DEV)
    wsc = wt.abs().mean(dim=(1, 2, 3))[None].contiguous()
    wbits, wsum = hip.pack_weight(wt, geom, wsc)
    ho, wo = hip.out_hw(geom)
    if grid:
        px = PC.grid_operands(f'proj.{name}.gpx', (n, cp, hx, wx), *PC.X_RANGE)
        pw = PC.grid_operands(f'proj.{name}.gpw', (o, cp), *PC.W_RANGE)
        pb = PC.grid_operands(f'proj.{name}.gpb', (o,), *PC.B_RANGE)
    else:
        px = detgen.normal(f'proj.{name}.px', (n, cp, hx, wx), scale=0.9)
        pw = detgen.normal(f'proj.{name}.pw', (o, cp), scale=cp ** -0.5)
        pb = detgen.normal(f'proj.{name}.pb', (o,), scale=0.3)
    return dict(hip=hip, geom=geom, planes=planes, xs=xs, wbits=wbits, wsum=wsum, wsc=wsc,
                bias=detgen.normal(f'proj.{name}.b', (o,), scale=0.2).to(DEV), px=px.to(DEV), pw=pw.to(DEV), pb=pb.to(DEV),
                slope=detgen.uniform(f'proj.{name}.slope', (o,), 0.05, 0.4).to(DEV), yshape=(n, o, ho, wo))


def _two_launches(cs, act, post, with_bias):
    hip = cs['hip']
    sc = hip.pointwise_conv(cs['px'], cs['pw'], cs['pb'] if with_bias else None, 2)
    assert sc.shape == cs['yshape']
    y = torch.full(cs['yshape'], float('nan'), device=DEV)
    hip.xnor_conv2d(cs['planes'], 2, cs['xs'], cs['wbits'], cs['wsum'], cs['wsc'], cs['bias'], cs['geom'], y, relu=act == 'relu',
                    res_pre=None if post else sc, res_post=sc if post else None, prelu=cs['slope'] if act == 'prelu' else None)
    return y


def _fused(cs, act, post, with_bias):
    hip = cs['hip']
    y = torch.full(cs['yshape'], float('nan'), device=DEV)
    took = hip.xnor_conv2d_proj(cs['planes'], 2, cs['xs'], cs['wbits'], cs['wsum'], cs['wsc'], cs['bias'], cs['geom'], y,
                                (cs['px'], cs['pw'], cs['pb'] if with_bias else None, 2, post), relu=act == 'relu',
                                prelu=cs['slope'] if act == 'prelu' else None)
    assert took, 'lsq_xnor_conv2d_proj refused a geometry it documents as supported'
    return y


@pytest.mark.parametrize('scheme', [LS2, LST], ids=['ls-2', 'ls-T'])
@pytest.mark.parametrize('name', list(CASES))
def test_fused_equals_pointwise_then_xnor(name, scheme):
    cs = _operands(name, scheme)
    for act in ('none', 'relu', 'prelu'):
        for post in (False, True):
            for with_bias in (True, False):
                want = _two_launches(cs, act, post, with_bias)
                got = _fused(cs, act, post, with_bias)
                assert not torch.isnan(want).any()
                assert torch.equal(got, want), (name, scheme, act, post, with_bias, float((got - want).abs().max()))


def test_res_post_tensor_beside_a_res_pre_projection():
    cs = _operands('c64_o64_pre', LS2)
    hip = cs['hip']
    other = detgen.normal('proj.other', cs['yshape'], scale=0.7).to(DEV)
    sc = hip.pointwise_conv(cs['px'], cs['pw'], cs['pb'], 2)
    want, got = torch.empty(cs['yshape'], device=DEV), torch.empty(cs['yshape'], device=DEV)
    hip.xnor_conv2d(cs['planes'], 2, cs['xs'], cs['wbits'], cs['wsum'], cs['wsc'], cs['bias'], cs['geom'], want, relu=True,
                    res_pre=sc, res_post=other)
    assert hip.xnor_conv2d_proj(cs['planes'], 2, cs['xs'], cs['wbits'], cs['wsum'], cs['wsc'], cs['bias'], cs['geom'], got,
                                (cs['px'], cs['pw'], cs['pb'], 2, False), relu=True, res_post=other)
    assert torch.equal(got, want)


def test_two_runs_give_the_same_bits():
    cs = _operands('c64_o128', LS2)
    first = _fused(cs, 'relu', True, True)
    second = _fused(cs, 'relu', True, True)
    assert torch.equal(first, second)


# ---- waves that walk over several tiles, every Cp, the anchor (tests/golden/projection_cases.py) -------------------------------
# (act, projection as res_post, projection bias)
EPILOGUES = (('relu', True, True), ('prelu', False, True), ('none', True, False))
MULTI = [(name, LS2) for name in PC.FUSED_CASES] + [(PC.FUSED_BOTH_SCHEMES, LST)]


def _equals_two_launches(cs, where):
    for act, post, with_bias in EPILOGUES:
        want = _two_launches(cs, act, post, with_bias)
        got = _fused(cs, act, post, with_bias)
        assert not torch.isnan(want).any()
        assert torch.equal(got, want), (where, act, post, with_bias, float((got - want).abs().max()))


@pytest.mark.parametrize('name, scheme', MULTI, ids=[f'{n}-{"ls-2" if s == LS2 else "ls-T"}' for n, s in MULTI])
def test_multi_tile_waves_equal_pointwise_then_xnor(name, scheme):
    _equals_two_launches(_operands(name, scheme), (name, scheme))


@pytest.mark.parametrize('name', list(PC.CP_CASES))
def test_every_projection_channel_count_equals_pointwise_then_xnor(name):
    _equals_two_launches(_operands(name, LS2), name)          # (_fused asserts that the call was taken: a refusal or a launch error fails)


def test_two_runs_of_a_multi_tile_launch_give_the_same_bits():
    cs = _operands(PC.FUSED_PARTIAL, LS2)
    first = _fused(cs, 'relu', True, True)
    second = _fused(cs, 'relu', True, True)
    assert torch.equal(first, second)


def _plain(cs, act):
    """lsq_xnor_conv2d without any residual."""
    y = torch.full(cs['yshape'], float('nan'), device=DEV)
    cs['hip'].xnor_conv2d(cs['planes'], 2, cs['xs'], cs['wbits'], cs['wsum'], cs['wsc'], cs['bias'], cs['geom'], y, relu=act == 'relu',
                          prelu=cs['slope'] if act == 'prelu' else None)
    assert not torch.isnan(y).any()
    return y


def _shortcut_exact(cs, with_bias):
    """The projection of integer-grid operands in fp64 (a strided slice and one matmul per image), cast to fp32: exact."""
    xs = cs['px'][:, :, ::2, ::2].double()
    n, cp, ho, wo = xs.shape
    sc = torch.matmul(cs['pw'].double(), xs.reshape(n, cp, ho * wo)).reshape(cs['yshape'])
    if with_bias:
        sc = sc + cs['pb'].double().view(1, -1, 1, 1)
    assert torch.equal(sc.float().double(), sc) and float(sc.abs().max()) < 2 ** 15
    return sc.float()


def _act(v, act, slope):
    if act == 'relu':
        return torch.relu(v)
    if act == 'prelu':
        return torch.where(v > 0, v, slope.view(1, -1, 1, 1) * v)
    return v


@pytest.mark.parametrize('name', list(PC.CP_CASES) + list(PC.FUSED_ANCHORED))
def test_fused_equals_plain_xnor_combined_with_the_exact_shortcut(name):
    """The anchor without lsq_pointwise_conv.  res_post: fused == plain(act) + sc; res_pre: fused == act(plain(no act) + sc) -- the
    epilogue's own single fp32 operations (one add; max(., 0); one product with the channel's slope) on the same two fp32 values."""
    cs = _operands(name, LS2, grid=True)
    for with_bias in (True, False):
        sc = _shortcut_exact(cs, with_bias)
        for act in ('relu', 'prelu', 'none'):
            got = _fused(cs, act, True, with_bias)
            want = _plain(cs, act) + sc
            assert torch.equal(got, want), (name, 'res_post', act, with_bias, float((got - want).abs().max()))
        base = _plain(cs, 'none')
        for act in ('relu', 'prelu'):
            got = _fused(cs, act, False, with_bias)
            want = _act(base + sc, act, cs['slope'])
            assert torch.equal(got, want), (name, 'res_pre', act, with_bias, float((got - want).abs().max()))


def test_multi_tile_launch_writes_all_of_y_and_nothing_else():
    cs = _operands(PC.FUSED_PARTIAL, LS2)
    hip = cs['hip']
    want = _fused(cs, 'relu', True, True)
    buf = torch.full((want.numel() + 2 * MARGIN,), float('nan'), device=DEV)
    inside = buf[MARGIN:MARGIN + want.numel()]
    assert inside.data_ptr() % 16 == 0
    assert hip.xnor_conv2d_proj(cs['planes'], 2, cs['xs'], cs['wbits'], cs['wsum'], cs['wsc'], cs['bias'], cs['geom'],
                                inside.view(cs['yshape']), (cs['px'], cs['pw'], cs['pb'], 2, True), relu=True)
    assert torch.isnan(buf[:MARGIN]).all() and torch.isnan(buf[MARGIN + want.numel():]).all(), 'written outside y'
    assert not torch.isnan(inside).any(), 'outputs left unwritten'
    assert torch.equal(inside.view(cs['yshape']), want)


def _conv_module(cin, cout, stride, seed):
    from quant.binary.binary_conv import QuantConv2d
    conv = QuantConv2d('ls-2', 'ls-1', cin, cout, 3, {'kind': 'symmetric', 'alpha': 3}, stride=stride, padding=1, bias=True)
    detgen.fill_module(conv, seed=seed)
    with torch.no_grad():
        conv.w_approximate.v1.copy_(conv.weight.abs().mean(dim=(1, 2, 3)))
    return conv.eval().to(DEV)


@pytest.mark.parametrize('switch', [1, 2], ids=['popcount', 'int8'])
def test_debug_implementations_refuse_and_python_falls_back(switch, monkeypatch):
    hip = _hip()
    conv = _conv_module(64, 128, 2, seed=3)
    x = detgen.normal('proj.dbg.x', (2, 64, 12, 12), scale=1.1).to(DEV)
    from quant.binary.binary_conv import ProjectionShortcut
    proj = ProjectionShortcut(x, detgen.normal('proj.dbg.pw', (128, 64), scale=0.125).to(DEV),
                              detgen.normal('proj.dbg.pb', (128,), scale=0.3).to(DEV), 2)
    answers = []
    real = hip.xnor_conv2d_proj
    monkeypatch.setattr(hip, 'xnor_conv2d_proj', lambda *a, **k: answers.append(real(*a, **k)) or answers[-1])
    with torch.no_grad():
        fused = conv.fused_forward(x, relu=True, res_post=proj)
        with hip.debug_switches(xnor_popcount=switch):
            fallback = conv.fused_forward(x, relu=True, res_post=proj)
    assert answers == [True, False]
    assert torch.equal(fused, fallback)


@pytest.mark.parametrize('double_shortcut', [True, False])
def test_block_with_and_without_the_fused_projection(double_shortcut, monkeypatch):
    from quant.models import resnet
    hip = _hip()
    block = resnet.XnorBasicBlock(64, 128, 'ls-2', 'ls-1', ['prelu', 'relu'], stride=2, double_shortcut=double_shortcut,
                                  clamp={'kind': 'symmetric', 'alpha': 3})
    detgen.fill_module(block, seed=5)
    with torch.no_grad():
        for conv in (block.conv1, block.conv2):
            conv.w_approximate.v1.copy_(conv.weight.abs().mean(dim=(1, 2, 3)))
    block.eval().to(DEV)
    x = detgen.normal('proj.block.x', (3, 64, 12, 12), scale=1.0).to(DEV)
    monkeypatch.setattr(hip, 'PROJ_FUSED_SHAPES', frozenset({(64, 128)}))      # (whatever the measured gate says: take the kernel)
    answers = []
    real = hip.xnor_conv2d_proj
    monkeypatch.setattr(hip, 'xnor_conv2d_proj', lambda *a, **k: answers.append(real(*a, **k)) or answers[-1])
    with torch.no_grad():
        fused = block(x)
        monkeypatch.setattr(resnet, 'FUSE_PROJECTION', False)
        plain = block(x)
    assert answers == [True]
    assert torch.equal(fused, plain)


def test_resnet18_logits_with_and_without_the_fused_projection(monkeypatch):
    import bench
    from quant.models import resnet
    hip = _hip()
    model = bench.build_model(bench.imagenet_arch('ls-2'), DEV)
    x = detgen.normal('proj.net.x', (2, 3, 64, 64), scale=1.0).to(DEV)
    monkeypatch.setattr(hip, 'PROJ_FUSED_SHAPES', frozenset({(64, 128), (128, 256), (256, 512)}))
    answers = []
    real = hip.xnor_conv2d_proj
    monkeypatch.setattr(hip, 'xnor_conv2d_proj', lambda *a, **k: answers.append(real(*a, **k)) or answers[-1])
    with torch.no_grad():
        fused = model(x)
        monkeypatch.setattr(resnet, 'FUSE_PROJECTION', False)
        plain = model(x)
    assert answers == [True, True, True]
    assert torch.equal(fused, plain)
