"""lsq_xnor_conv2d_half (include/lsq_hip_conv_xnor_half.h; the __bf16 / _Float16 instantiations of csrc/lsq_xnor_mfma.hip and
csrc/lsq_xnor_conv.hip) and QuantConv2d's ``xnor_half`` switch on the GPU.

Reference of every kernel test: the unchanged lsq_xnor_conv2d on the same operands with ``res.float()`` residuals, followed by
``.to(dtype)``.  The 16-bit kernels run the same fp32 arithmetic on the same values (a 16-bit residual widens exactly) and round
once at the store, so every comparison is torch.equal on the raw 16-bit patterns -- no tolerance.  The geometries, plane counts and
epilogues are tests/golden/conv_xnor_half_cases.py; tests/test_conv_xnor_half_host.py proves what they launch."""

import ctypes
import functools

import pytest
import torch

import conv_train_half_cases as H
import conv_xnor_half_cases as C
import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
CODES = {torch.bfloat16: 1, torch.float16: 2}
GF, LS1 = 4, 1
E_WORKSPACE, E_UNSUPPORTED = -5, -6


def _hip():
    from quant import _hip
    return _hip


def _bits(y):
    assert y.dtype in (torch.bfloat16, torch.float16)
    return y.contiguous().view(torch.int16)


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(_bits(got), _bits(want))


def _geom(g):
    return _hip().make_geom(g.N, g.C, g.H, g.W, g.O, g.k, g.k, g.stride, g.pad, g.dil, g.groups)


@functools.lru_cache(maxsize=4)
def _operands(gid, kx, kw):
    """Planes / scales of ``kx`` greedy activation planes and ``kw`` weight planes of the geometry, bias, slopes, fp32 residuals."""
    hip, g = _hip(), C.BY_ID[gid]
    geom = _geom(g)
    x = detgen.normal(f'xnorhalf.{gid}.x', (g.N, g.C, g.H, g.W), scale=1.2).to(DEV)
    planes = torch.zeros((kx * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xs = torch.empty((kx, g.N), dtype=torch.float32, device=DEV)
    hip.act_quant(x, geom, GF, kx, 3, 2.0, planes, xs)
    wt = detgen.uniform(f'xnorhalf.{gid}.w', (g.O, g.C // g.groups, g.k, g.k), -0.5, 0.5).to(DEV)
    v1 = wt.abs().mean(dim=(1, 2, 3))
    wsc = torch.stack([v1 * 0.5 ** q for q in range(kw)]).contiguous()
    wbits, wsum = hip.pack_weight(wt, geom, wsc)
    shape = (g.N, g.O) + tuple(hip.out_hw(geom))
    return dict(geom=geom, planes=planes, xs=xs, wbits=wbits, wsum=wsum, wsc=wsc, kx=kx, shape=shape,
                bias=detgen.normal(f'xnorhalf.{gid}.b', (g.O,), scale=0.2).to(DEV),
                slope=detgen.uniform(f'xnorhalf.{gid}.slope', (g.O,), 0.05, 0.4).to(DEV),
                slope1=torch.tensor([0.25], device=DEV),
                res_pre=detgen.normal(f'xnorhalf.{gid}.rpre', shape, scale=0.7).to(DEV),
                res_post=detgen.normal(f'xnorhalf.{gid}.rpost', shape, scale=0.7).to(DEV))


def _epilogue(cs, epi, dtype):
    bias, pre, act, post = epi
    return dict(bias=cs['bias'] if bias else None, relu=act == 'relu',
                prelu={'prelu': cs['slope'], 'prelu1': cs['slope1']}.get(act),
                res_pre=cs['res_pre'].to(dtype) if pre else None, res_post=cs['res_post'].to(dtype) if post else None)


def _comparator(cs, dtype, bias=None, relu=False, prelu=None, res_pre=None, res_post=None):
    """lsq_xnor_conv2d on .float() residuals, then .to(dtype); also returns the fp32 tensor."""
    y32 = torch.full(cs['shape'], float('nan'), device=DEV)
    _hip().xnor_conv2d(cs['planes'], cs['kx'], cs['xs'], cs['wbits'], cs['wsum'], cs['wsc'], bias, cs['geom'], y32, relu,
                       None if res_pre is None else res_pre.float(), None if res_post is None else res_post.float(), prelu)
    assert not torch.isnan(y32).any()
    return y32.to(dtype), y32


def _half(cs, dtype, bias=None, relu=False, prelu=None, res_pre=None, res_post=None):
    return _hip().xnor_conv2d_half(cs['planes'], cs['kx'], cs['xs'], cs['wbits'], cs['wsum'], cs['wsc'], bias, cs['geom'], dtype,
                                   relu, res_pre, res_post, prelu)


def _check(gid, kx, kw, epi, where):
    cs = _operands(gid, kx, kw)
    for name, dtype in DTYPES.items():
        e = _epilogue(cs, epi, dtype)
        want, _ = _comparator(cs, dtype, **e)
        got = _half(cs, dtype, **e)
        differ = (_bits(got) != _bits(want)).sum().item()
        print(f'{where} {gid} kx={kx} kw={kw} {name} {epi}: {differ} of {want.numel()} outputs differ')
        assert differ == 0 and got.dtype == dtype


# ------------------------------------------------------------------------------------------------ the bit contract
@pytest.mark.parametrize('kx, kw', C.PLANES, ids=[f'kx{a}_kw{b}' for a, b in C.PLANES])
@pytest.mark.parametrize('gid', [g.id for g in C.GEOMS])
def test_bit_contract_with_the_full_epilogue(gid, kx, kw):
    _check(gid, kx, kw, C.FULL, 'full')


@pytest.mark.parametrize('kx, kw', C.EPILOGUE_PLANES, ids=[f'kx{a}_kw{b}' for a, b in C.EPILOGUE_PLANES])
@pytest.mark.parametrize('gid', C.EPILOGUE_GEOMS)
def test_bit_contract_of_every_epilogue(gid, kx, kw):
    for name, epi in C.EPILOGUES.items():
        _check(gid, kx, kw, epi, name)


@pytest.mark.parametrize('gid', [g.id for g in C.MFMA])
def test_both_implementations_give_the_same_bits(gid):
    """lsq_debug_xnor_impl(1) forces the popcount kernel; (2), the int8 comparator, takes the fp4 kernel in the 16-bit entry."""
    hip = _hip()
    kx, kw = (2, 1) if gid == C.MULTI_TILE else (3, 2)
    cs = _operands(gid, kx, kw)
    for name, dtype in DTYPES.items():
        e = _epilogue(cs, C.FULL, dtype)
        default = _half(cs, dtype, **e)
        for mode in (1, 2):
            old = hip.xnor_impl(mode)
            try:
                forced = _half(cs, dtype, **e)
            finally:
                hip.xnor_impl(old)
            differ = (_bits(forced) != _bits(default)).sum().item()
            print(f'{gid} {name} impl {mode}: {differ} outputs differ from the default')
            assert differ == 0
        assert _same(default, _comparator(cs, dtype, **e)[0])


# ------------------------------------------------------------------------------------------------ rounding
def _aligned_operands():
    """The first geometry with activations and weights that mostly agree: x[n, c, h, w] has the sign q[c] (a few samples
    flipped), out-channel o's weights q[c] with o of them flipped -- so an interior pixel's (b * s) is 576 - 2 (mismatches),
    every second out-channel negated.  One activation plane, one weight plane."""
    hip, g = _hip(), C.MFMA[0]
    geom = _geom(g)
    q = torch.where(detgen.uniform('xnorhalf.round.q', (g.C,)) < 0.5, -1.0, 1.0)
    flip = torch.where(detgen.uniform('xnorhalf.round.flip', (g.N, g.C, g.H, g.W)) < 0.004, -1.0, 1.0)
    x = (q[None, :, None, None] * flip).to(DEV)
    wt = q[None, :, None, None].repeat(g.O, 1, 3, 3)
    flat = wt.view(g.O, -1)
    for o in range(g.O):
        flat[o, :o] *= -1.0
        if o % 2:
            flat[o] *= -1.0
    planes = torch.zeros((hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xs = torch.empty((1, g.N), dtype=torch.float32, device=DEV)
    hip.act_quant(x, geom, LS1, 1, 3, -1.0, planes, xs)
    ones = torch.ones((1, g.O), device=DEV)
    wbits, wsum = hip.pack_weight(wt.to(DEV), geom, ones)
    return dict(geom=geom, planes=planes, xs=xs, wbits=wbits, wsum=wsum, wsc=ones, kx=1,
                shape=(g.N, g.O) + tuple(hip.out_hw(geom)))


def test_rounding_ties_overflow_and_subnormals():
    cs = _aligned_operands()
    cs['xs'].fill_(1.0)
    # unit scales, no bias: integers up to 576, among them exact ties of bf16 (8 significant bits: 4 k + 2 above 512)
    _, y32 = _comparator(cs, torch.bfloat16)
    assert bool((y32 == y32.round()).all()) and float(y32.abs().max()) <= 576
    a = y32.abs()
    ties = ((a > 512) & (a % 4 == 2)) | ((a > 256) & (a < 512) & (a % 2 == 1))
    print(f'rounding: {int(ties.sum())} exact bf16 ties among {y32.numel()} integer outputs, max |y| = {float(a.max())}')
    assert int(ties.sum()) >= 1
    ties_up = ties & ((a - 2) % 8 == 0)            # (a tie between an even and an odd significand either way)
    assert int(ties_up.sum()) >= 1 and int((ties & ~ties_up).sum()) >= 1
    for xscale, what in ((1.0, 'ties'), (200.0, 'fp16 overflow'), (1e-7, 'fp16 subnormals'), (1e-21, 'bf16 subnormals')):
        cs['xs'].fill_(xscale)
        wsc = torch.full_like(cs['wsc'], 1e-20 if what == 'bf16 subnormals' else 1.0)
        cw = dict(cs, wsc=wsc)
        for name, dtype in DTYPES.items():
            want, y32 = _comparator(cw, dtype)
            got = _half(cw, dtype)
            differ = (_bits(got) != _bits(want)).sum().item()
            tiny = torch.finfo(dtype).tiny
            sub = int(((want.float().abs() < tiny) & (want != 0)).sum())
            print(f'rounding {what} {name}: {differ} outputs differ; {int(torch.isinf(want).sum())} inf, {sub} subnormal')
            assert differ == 0
            if what == 'fp16 overflow' and dtype == torch.float16:
                assert bool(torch.isinf(want).any()) and float(y32.abs().max()) > 65504
            if what.split()[0] == name and 'subnormals' in what:
                assert sub >= 1
    cs['xs'].fill_(1.0)


# ------------------------------------------------------------------------------------------------ workspace, refusals
def _raw_call(cs, dtype_code, y, ws, ws_bytes):
    hip = _hip()
    hip.lib()
    return hip.conv_xnor_half_lib().lsq_xnor_conv2d_half(
        cs['planes'].data_ptr(), cs['kx'], cs['xs'].data_ptr(), cs['wbits'].data_ptr(), cs['wsum'].data_ptr(), cs['wsc'].shape[0],
        cs['wsc'].data_ptr(), cs['bias'].data_ptr(), ctypes.byref(cs['geom']), 0, None, None, None, dtype_code, y.data_ptr(), None if ws is None else ws.data_ptr(), ws_bytes, hip.stream_ptr(torch.device(DEV)))


@pytest.mark.parametrize('gid', ['m128_s2', 'p24_o20'])
def test_workspace_content_does_not_matter_and_refusals_write_nothing(gid):
    hip = _hip()
    cs = _operands(gid, 3, 2)
    need = C.workspace_bytes(C.BY_ID[gid], 3, 2)
    assert hip.conv_xnor_half_lib().lsq_xnor_conv2d_half_workspace_bytes(ctypes.byref(cs['geom']), 3, 2) == need > 0
    for name, dtype in DTYPES.items():
        want, _ = _comparator(cs, dtype, bias=cs['bias'])
        ws = torch.full((need // 4,), float('nan'), device=DEV)
        y = torch.full(cs['shape'], 7.0, dtype=dtype, device=DEV)
        assert _raw_call(cs, CODES[dtype], y, ws, need) == 0
        assert _same(y, want)
        sentinel = torch.full(cs['shape'], 7.0, dtype=dtype, device=DEV)
        for w, nbytes in ((None, need), (ws, need - 1), (ws, 0)):
            y = sentinel.clone()
            assert _raw_call(cs, CODES[dtype], y, w, nbytes) == E_WORKSPACE
            torch.cuda.synchronize()
            assert _same(y, sentinel)
        misaligned = torch.empty((need + 4,), dtype=torch.uint8, device=DEV)[2:]
        y = sentinel.clone()
        assert _raw_call(cs, CODES[dtype], y, misaligned, need) == E_WORKSPACE
        for code in (0, 3, -1):
            assert _raw_call(cs, code, y, ws, need) == E_UNSUPPORTED
        torch.cuda.synchronize()
        assert _same(y, sentinel)


@pytest.mark.parametrize('gid', ['m64_tail', 'p24_o20'])
def test_unaligned_y_and_residuals(gid):
    """y and both residuals at an odd element offset of a larger buffer (2-byte aligned, no more): the same bits, and the
    elements around y keep their sentinel."""
    cs = _operands(gid, 2, 1)
    n = 1
    for d in cs['shape']:
        n *= d
    for name, dtype in DTYPES.items():
        e = _epilogue(cs, C.FULL, dtype)
        want = _half(cs, dtype, **e)
        bufs = {k: torch.full((n + 8,), 3.0, dtype=dtype, device=DEV) for k in ('y', 'res_pre', 'res_post')}
        views = {k: b[3:3 + n].view(cs['shape']) for k, b in bufs.items()}
        assert all(v.data_ptr() % 4 == 2 for v in views.values())
        views['res_pre'].copy_(e['res_pre'])
        views['res_post'].copy_(e['res_post'])
        hip = _hip()
        code = hip.conv_xnor_half_lib().lsq_xnor_conv2d_half(
            cs['planes'].data_ptr(), 2, cs['xs'].data_ptr(), cs['wbits'].data_ptr(), cs['wsum'].data_ptr(), 1, cs['wsc'].data_ptr(),
            cs['bias'].data_ptr(), ctypes.byref(cs['geom']), hip.ACT_PRELU_CHANNEL, e['prelu'].data_ptr(), views['res_pre'].data_ptr(),
            views['res_post'].data_ptr(), CODES[dtype], views['y'].data_ptr(), None, 0, hip.stream_ptr(torch.device(DEV)))
        assert code == 0
        differ = (_bits(views['y']) != _bits(want)).sum().item()
        print(f'unaligned {gid} {name}: {differ} outputs differ')
        assert differ == 0
        assert bool((bufs['y'][:3] == 3.0).all()) and bool((bufs['y'][3 + n:] == 3.0).all())


def test_non_temporal_residual_loads():
    """The one large case: residual plus output exceed the Infinity Cache in 16-bit, so the residual is read with the
    non-temporal hint."""
    hip, g = _hip(), C.STREAM
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < 4 << 30:
        pytest.skip(f'needs 4 GiB of free device memory for about 1 GB of tensors, {free >> 20} MiB are free')
    assert 2 * 2 * C.outputs(g) > C.INFINITY_CACHE_BYTES
    geom = _geom(g)
    gen = torch.Generator(device=DEV).manual_seed(1234)
    x = torch.randn((g.N, g.C, g.H, g.W), device=DEV, generator=gen)
    planes = torch.zeros((2 * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    xs = torch.empty((2, g.N), dtype=torch.float32, device=DEV)
    hip.act_quant(x, geom, GF, 2, 3, 2.0, planes, xs)
    del x
    wt = detgen.uniform('xnorhalf.stream.w', (g.O, g.C, 3, 3), -0.5, 0.5).to(DEV)
    wsc = wt.abs().mean(dim=(1, 2, 3))[None].contiguous()
    wbits, wsum = hip.pack_weight(wt, geom, wsc)
    shape = (g.N, g.O) + tuple(hip.out_hw(geom))
    cs = dict(geom=geom, planes=planes, xs=xs, wbits=wbits, wsum=wsum, wsc=wsc, kx=2, shape=shape)
    for name, dtype in DTYPES.items():
        res = torch.randn(shape, device=DEV, generator=gen, dtype=torch.float32).to(dtype)
        got = _half(cs, dtype, res_post=res)
        want, y32 = _comparator(cs, dtype, res_post=res)
        del y32
        same = torch.equal(_bits(got), _bits(want))
        print(f'non-temporal {name}: {2 * 2 * C.outputs(g) >> 20} MiB of residual + output, equal: {same}')
        assert same
        del res, got, want


# ------------------------------------------------------------------------------------------------ QuantConv2d
CLAMP = {'kind': 'symmetric', 'alpha': 2}


def _module(xq, ws, cin, cout, seed, **kw):
    from quant.binary.binary_conv import QuantConv2d
    m = QuantConv2d(xq, ws, cin, cout, 3, CLAMP, padding=1, **kw)
    detgen.fill_module(m, seed=seed)
    with torch.no_grad():
        for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight, ws)):
            buf.copy_(v)
    return m.eval().to(DEV)


@pytest.fixture
def counters(monkeypatch):
    """Calls of the kernels' wrappers and of the torch passes a 16-bit fused_forward composes."""
    hip = _hip()
    names = {'xnor': (hip, 'xnor_conv2d'), 'xnor_half': (hip, 'xnor_conv2d_half'), 'act_half': (hip, 'act_quant_half'),
             'add': (torch.Tensor, '__add__'), 'relu': (torch, 'relu'), 'prelu': (torch.nn.functional, 'prelu')}
    calls = {name: 0 for name in names}

    def counted(name, real):
        def f(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return f

    for name, (owner, attr) in names.items():
        monkeypatch.setattr(owner, attr, counted(name, getattr(owner, attr)))
    return calls


def _set_average(m):
    avg = m.x_approximate.moving_avg_module.moving_average
    with torch.no_grad():
        avg.copy_(torch.tensor([0.9 * 0.5 ** q for q in range(avg.numel())]).view_as(avg))


@pytest.mark.parametrize('xq', ['ls-1', 'ls-2', 'gf-3'])
@pytest.mark.parametrize('dt', DTYPES)
def test_plain_forward_gives_the_bits_of_the_switch_off(dt, xq, counters):
    dtype = DTYPES[dt]
    kw = dict(moving_average_mode='eval_only') if xq == 'ls-2' else {}
    m = _module(xq, 'ls-1' if xq != 'gf-3' else 'ls-2', 64, 70, seed=91, **kw)
    if xq == 'ls-2':
        _set_average(m)
    m.act_half = True
    x = detgen.normal(f'xnorhalf.mod.{xq}', (5, 64, 9, 9), scale=1.3).to(DEV).to(dtype)
    with torch.no_grad():
        off = m(x)
        assert (counters['xnor'], counters['xnor_half']) == (1, 0)
        m.xnor_half = True
        on = m(x)
        assert (counters['xnor'], counters['xnor_half']) == (1, 1)
    print(f'{xq} {dt}: {(_bits(on) != _bits(off)).sum().item()} outputs differ between xnor_half on and off')
    assert _same(on, off)


@pytest.mark.parametrize('dt', DTYPES)
def test_fused_forward_is_one_launch_rounded_once(dt, counters):
    hip = _hip()
    dtype = DTYPES[dt]
    m = _module('ls-2', 'ls-1', 64, 96, seed=92, moving_average_mode='eval_only')
    _set_average(m)
    m.act_half = m.xnor_half = True
    x = detgen.normal('xnorhalf.fused.x', (5, 64, 9, 9), scale=1.3).to(DEV).to(dtype)
    res = detgen.normal('xnorhalf.fused.res', (5, 96, 9, 9), scale=1.0).to(DEV).to(dtype)
    slopes = detgen.uniform('xnorhalf.fused.slope', (96,), 0.05, 0.4).to(DEV)
    geom = m._geom_of(x, hip)
    for kwargs in (dict(relu=True, res_pre=res), dict(prelu=slopes, res_post=res)):
        before = dict(counters)
        with torch.no_grad():
            y = m.fused_forward(x, **kwargs)
        took = {k: counters[k] - before[k] for k in counters}
        print(f'fused_forward {dt} {sorted(kwargs)}: calls {took}')
        assert took == {'xnor': 0, 'xnor_half': 1, 'act_half': 1, 'add': 0, 'relu': 0, 'prelu': 0}
        # the fp32 kernel composition on the same planes, rounded once
        k = m.x_approximate.n_planes
        planes = torch.zeros((k * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
        out = torch.empty((k, 5), device=DEV)
        hip.act_quant(x.float(), geom, m.x_approximate.hip_scheme, k, 3, float(torch.tensor(2.0).to(dtype)), planes, out,
                      m.last_act_scales)
        wbits, wsum, wscales, _ = m._packed_weights(geom, hip)
        ref = torch.empty((5, 96, 9, 9), device=DEV)
        hip.xnor_conv2d(planes, k, m.last_act_scales, wbits, wsum, wscales, m.bias.detach(), geom, ref, kwargs.get('relu', False),
                        None if 'res_pre' not in kwargs else res.float(), None if 'res_post' not in kwargs else res.float(),
                        kwargs.get('prelu'))
        differ = (_bits(y) != _bits(ref.to(dtype))).sum().item()
        print(f'fused_forward {dt}: {differ} outputs differ from the fp32 composition rounded once')
        assert differ == 0 and y.dtype == dtype


@pytest.mark.parametrize('dt', DTYPES)
def test_operands_the_epilogue_does_not_take_stay_on_the_composition(dt, counters):
    dtype = DTYPES[dt]
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    m = _module('ls-1', 'ls-1', 64, 70, seed=93)
    m.act_half = True
    x = detgen.normal('xnorhalf.stay.x', (5, 64, 9, 9), scale=1.3).to(DEV).to(dtype)
    res = detgen.normal('xnorhalf.stay.res', (5, 70, 9, 9), scale=1.0).to(DEV)
    fp = _module('fp', 'ls-1', 64, 70, seed=94)
    fp.fp_half = True
    with torch.no_grad():
        for mod, r in ((m, res.to(other)), (m, res.float()), (m, res.to(dtype)[:, :, :1, :1]), (fp, res.to(dtype))):
            mod.xnor_half = False
            want = mod.fused_forward(x, relu=True, res_pre=r)
            before = counters['add']
            mod.xnor_half = True
            got = mod.fused_forward(x, relu=True, res_pre=r)
            assert counters['add'] - before == 1                    # (the torch composition)
            assert got.dtype == want.dtype and torch.equal(got, want)
    assert counters['xnor_half'] == 3                               # (m's plain convolution inside the composition)


@pytest.mark.parametrize('dtype', H.DTYPES, ids=lambda t: H.DTYPE_NAMES[t])
def test_train_step_gives_the_bits_of_the_switch_off(dtype, counters):
    case = H.BY_ID['s2_3x5']
    d = H.inputs(case.id, dtype)
    results = []
    for on in (False, True):
        conv = H.make_module(case)
        conv.hip_train_half = True
        conv.xnor_half = on
        conv = conv.to(DEV).train()
        x = d['x'].to(DEV).requires_grad_()
        y = conv(x)
        y.backward(d['gy'].to(DEV))
        results.append((y.detach(), x.grad, conv.weight.grad, conv.bias.grad))
    assert (counters['xnor'], counters['xnor_half']) == (1, 1)
    for name, a, b in zip(('y', 'grad_x', 'grad_w', 'grad_b'), *results):
        print(f'train step {H.DTYPE_NAMES[dtype]} {name}: equal {torch.equal(a, b)}')
        assert a.dtype == b.dtype and torch.equal(a, b), name


def test_defaults_are_the_parents(counters):
    from quant.binary.binary_conv import QuantConv2d
    assert QuantConv2d.xnor_half is False
    m = _module('ls-1', 'ls-1', 64, 70, seed=95)
    m.act_half = True
    x = detgen.normal('xnorhalf.default.x', (5, 64, 9, 9), scale=1.3).to(DEV).to(torch.bfloat16)
    res = detgen.normal('xnorhalf.default.res', (5, 70, 9, 9), scale=1.0).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        y = m.fused_forward(x, relu=True, res_pre=res)
        assert (counters['act_half'], counters['xnor'], counters['xnor_half'], counters['add'], counters['relu']) == (1, 1, 0, 1, 1)
        ref = torch.relu(m(x) + res)
    assert torch.equal(y, ref)
    assert counters['xnor_half'] == 0
