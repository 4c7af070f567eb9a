"""lsq_signw_conv2d_half (liblsq_hip_conv_half.so) and QuantConv2d('fp', w) with bf16 / fp16 inputs on the GPU: every case of
tests/golden/conv_half_cases.py against fp64; the 16-bit output as the fp32 output rounded once; bf16 against
lsq_signw_conv2d; unaligned inputs, the output buffer, determinism; refused calls that write nothing; fp16 / bf16 subnormals
through the matrix instruction (known answer); the module's dispatch and weight cache, and the paths that stay on torch.

Every test prints the figure it asserts on (pytest -s shows them)."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_half_cases as C
import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BOUND = 1e-5      # |y - y64| <= BOUND * max |y64|: the project's bound for these kernels
E_NULL, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -5, -6
DTYPES = C.DTYPES
IDS = [c.id for c in C.CASES]


def _hip():
    from quant import _hip
    return _hip


def _geom(c):
    return _hip().make_geom(c.N, c.C, c.H, c.W, c.O, c.KH, c.KW, c.stride, c.pad, c.dil, c.groups)


_OPERANDS = {}


def _operands(cid, dt):
    """Operands of a case on the GPU, made once and shared (nothing below writes into them)."""
    key = (cid, dt)
    if key not in _OPERANDS:
        hip = _hip()
        c = C.BY_ID[cid]
        w, wsc, _, b = C.weights(cid)
        g = _geom(c)
        wbits, _ = hip.pack_weight(w.to(DEV), g, wsc.to(DEV))
        _OPERANDS[key] = dict(c=c, g=g, x=C.batch(cid, dt).to(DEV), wbits=wbits, wsc=wsc.to(DEV), b=None if b is None else b.to(DEV),
                              alpha=C.alpha_in(C.ALPHAS[c.alpha], DTYPES[dt]), dtype=DTYPES[dt])
    return _OPERANDS[key]


def _run(p, x=None, out_dtype=torch.float32, alpha=None, planes=None):
    wsc = p['wsc'] if planes is None else p['wsc'][:planes].contiguous()
    return _hip().signw_conv2d_half(p['x'] if x is None else x, p['alpha'] if alpha is None else alpha, p['wbits'], wsc, p['b'],
                                    p['g'], out_dtype=out_dtype)


def _bits(y):
    return y.contiguous().view(torch.int32 if y.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize('cid', IDS)
@pytest.mark.parametrize('dt', DTYPES)
def test_kernel_against_fp64(dt, cid):
    """Every case x both types, fp32 output.  Only the fp32 rounding of the accumulation is left: 1e-5 of max |y64|."""
    p = _operands(cid, dt)
    y = _run(p)
    y64 = C.reference(cid, dt)
    assert y.dtype == torch.float32 and y.shape == y64.shape
    err = (y.cpu().double() - y64).abs().max().item()
    scale = y64.abs().max().item()
    print(f'fp64 {cid} {dt} plan={p["c"].plan} alpha={p["alpha"]}: max err / max|y64| = {err / scale:.3e}')
    assert err <= BOUND * scale, (cid, err / scale)


@pytest.mark.parametrize('planes', (1, 2, 3, 8))
@pytest.mark.parametrize('cid', ('gf8_patch', 'gf8_general'))
@pytest.mark.parametrize('dt', DTYPES)
def test_sixteen_bit_output_is_the_fp32_output_rounded_once(dt, cid, planes):
    """One launch without a workspace, and two, three and eight launches with the fp32 sum in the workspace."""
    p = _operands(cid, dt)
    y32 = _run(p, planes=planes)
    y16 = _run(p, out_dtype=p['dtype'], planes=planes)
    assert y16.dtype == p['dtype']
    differ = (_bits(y16) != _bits(y32.to(p['dtype']))).sum().item()
    print(f'{cid} {dt} {planes} planes: {differ} outputs differ from the fp32 result rounded once')
    assert differ == 0


@pytest.mark.parametrize('alpha', (-1.0, 2.0))
@pytest.mark.parametrize('cid', [c.id for c in C.CASES if c.plan & C.PATCH])
def test_bf16_equals_the_fp32_kernel_on_the_patch_paths(cid, alpha):
    """The same values (torch.equal: -0 == +0) as lsq_signw_conv2d on x.float(), with and without the 3x3 fast path's
    prepared weights, wherever both libraries take a patch kernel."""
    hip = _hip()
    p = _operands(cid, 'bf16')
    c = p['c']
    assert C.fp32_patch(c)
    y = _run(p, alpha=alpha)
    kw = p['wsc'].shape[0]
    for wprep in (None, hip.signw_prepare_weight(p['wbits'], kw, p['g'])):
        ref = torch.empty_like(y)
        hip.signw_conv2d(p['x'].float(), alpha, p['wbits'], p['wsc'], p['b'], p['g'], ref, wprep=wprep)
        differ = (y != ref).sum().item()
        print(f'{cid} alpha={alpha} prepared={wprep is not None}: {differ} values differ from lsq_signw_conv2d(x.float())')
        assert torch.equal(y, ref)


@pytest.mark.parametrize('cid', ('p1_wide', 's2_wide', 's2_narrow', 'k5_narrow', 'long_row', 'proj_wide'))
@pytest.mark.parametrize('dt', DTYPES)
def test_address_and_layout(dt, cid):
    """x one element off its allocation's alignment gives the same bits; y inside a guard-filled buffer with an odd element
    count: guards intact; two calls give the same bits."""
    hip = _hip()
    p = _operands(cid, dt)
    x = p['x']
    y32, y16 = _run(p), _run(p, out_dtype=p['dtype'])
    buf = torch.zeros((x.numel() + 1,), dtype=x.dtype, device=DEV)
    xo = buf[1:].view(x.shape)
    xo.copy_(x)
    assert xo.data_ptr() % 4 == 2 and xo.is_contiguous()
    again32, again16 = _run(p, x=xo), _run(p, x=xo, out_dtype=p['dtype'])
    d32, d16 = (_bits(again32) != _bits(y32)).sum().item(), (_bits(again16) != _bits(y16)).sum().item()
    print(f'{cid} {dt}: x offset by one element: {d32} fp32 and {d16} 16-bit outputs differ')
    assert d32 == 0 and d16 == 0
    same = torch.equal(_bits(_run(p)), _bits(y32)) and torch.equal(_bits(_run(p, out_dtype=p['dtype'])), _bits(y16))
    print(f'{cid} {dt}: a second call gives the same bits: {same}')
    assert same
    # the output buffer: an odd element count, guards of 3 elements on both sides (a 16-bit y then starts 2 bytes off a dword)
    lib = hip.conv_half_lib()
    kw, g = p['wsc'].shape[0], p['g']
    for out_dtype, want in ((p['dtype'], y16), (torch.float32, y32)):
        n = want.numel()
        guard = 3 if (n + 6) % 2 else 4
        out = torch.full((n + 3 + guard,), 77.0, dtype=out_dtype, device=DEV)
        assert out.numel() % 2 == 1
        ydt = hip.LINEAR_HALF_DTYPES[out_dtype]
        need = int(lib.lsq_signw_conv2d_half_workspace_bytes(ctypes.byref(g), kw, ydt))
        ws = torch.empty((max(need, 4),), dtype=torch.uint8, device=DEV)
        rc = lib.lsq_signw_conv2d_half(x.data_ptr(), hip.LINEAR_HALF_DTYPES[x.dtype], p['alpha'], p['wbits'].data_ptr(), kw,
                                       p['wsc'].data_ptr(), hip.ptr(p['b']), ctypes.byref(g), out[3:].data_ptr(), ydt,
                                       ws.data_ptr(), ws.numel(), hip.stream_ptr(DEV))
        torch.cuda.synchronize()
        intact = bool((out[:3] == 77.0).all() and (out[3 + n:] == 77.0).all())
        inner = (_bits(out[3:3 + n]) != _bits(want).view(-1)).sum().item()
        print(f'{cid} {dt} y {out_dtype}: code {rc}, guards intact: {intact}, {inner} outputs differ')
        assert rc == 0 and intact and inner == 0


def test_refused_calls_write_nothing():
    hip = _hip()
    p = _operands('gf8_patch', 'bf16')
    lib = hip.conv_half_lib()
    code = hip.LINEAR_HALF_DTYPES
    bf, fp, f32 = code[torch.bfloat16], code[torch.float16], code[torch.float32]
    g = p['g']
    c = p['c']
    n = c.N * c.O * C.out_hw(c)[0] * C.out_hw(c)[1]
    bad = hip.make_geom(c.N, c.C, c.H, c.W, c.O, 3, 3, (1, 1), (1, 1), (1, 1), 3)           # 16 channels, 3 groups
    empty = hip.make_geom(c.N, c.C, 2, 2, c.O, 5, 5, (1, 1), (1, 1), (1, 1), 1)
    # (geometry, x dtype, y dtype, planes, workspace bytes offered, expected)
    refusals = ((g, f32, f32, 1, 4 * n, E_UNSUPPORTED), (g, bf, fp, 1, 4 * n, E_UNSUPPORTED), (g, bf, f32, 9, 4 * n, E_UNSUPPORTED),
                (g, bf, f32, 0, 4 * n, E_UNSUPPORTED), (g, bf, bf, 8, 4 * n - 1, E_WORKSPACE), (g, bf, bf, 2, 0, E_WORKSPACE),
                (bad, bf, f32, 1, 4 * n, E_SHAPE), (empty, bf, f32, 1, 4 * n, E_SHAPE), (None, bf, f32, 1, 4 * n, E_NULL))
    for geom, xdt, ydt, planes, wbytes, expected in refusals:
        y = torch.full((n,), 123.0, device=DEV)
        ws = torch.full((n,), -5.0, device=DEV)
        rc = lib.lsq_signw_conv2d_half(p['x'].data_ptr(), xdt, 2.0, p['wbits'].data_ptr(), planes, p['wsc'].data_ptr(), hip.ptr(p['b']),
                                       None if geom is None else ctypes.byref(geom), y.data_ptr(), ydt,
                                       ws.data_ptr() if wbytes else None, wbytes, hip.stream_ptr(DEV))
        torch.cuda.synchronize()
        print(f'x dtype {xdt}, y dtype {ydt}, planes {planes}, workspace {wbytes}: code {rc}')
        assert rc == expected
        assert (y == 123.0).all() and (ws == -5.0).all()
    with pytest.raises(TypeError):
        hip.signw_conv2d_half(p['x'].float(), 2.0, p['wbits'], p['wsc'], p['b'], g)


@pytest.mark.parametrize('dt', DTYPES)
def test_subnormal_known_answer(dt):
    """64 channels of the smallest subnormal of the type against an all +1 1x1 plane of scale 1: 64 * 2^-24 (fp16) or
    64 * 2^-133 (bf16) exactly -- the matrix instruction does not flush 16-bit subnormals."""
    hip = _hip()
    dtype = DTYPES[dt]
    tiny = 2.0 ** -24 if dt == 'fp16' else 2.0 ** -133
    n, ch, h, w, o = 2, 64, 3, 5, 4
    x = torch.full((n, ch, h, w), tiny, dtype=torch.float64).to(dtype).to(DEV)
    assert float(x.double().min()) == tiny
    g = hip.make_geom(n, ch, h, w, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    wsc = torch.ones((1, o), device=DEV)
    wbits, _ = hip.pack_weight(torch.ones((o, ch, 1, 1), device=DEV), g, wsc)
    for alpha in (-1.0, 2.0):
        y = hip.signw_conv2d_half(x, alpha, wbits, wsc, None, g, out_dtype=torch.float32)
        print(f'{dt} alpha={alpha}: 64 subnormals sum to {y.double().min().item():.6e} .. {y.double().max().item():.6e}, '
              f'expected {64 * tiny:.6e}')
        assert y.shape == (n, o, h, w) and (y.double() == 64 * tiny).all()


@pytest.mark.parametrize('cid', ('p1_narrow', 'proj_wide'))
@pytest.mark.parametrize('dt', DTYPES)
def test_without_a_bound_nan_and_inf_pass_as_they_are(dt, cid):
    """The identity (a negative bound, or +inf: a bound above fp16's range) issues no min / max: a NaN and a -inf activation
    make exactly the outputs whose taps read them non-finite, and every other output keeps its bits."""
    p = _operands(cid, dt)
    c = p['c']
    x = p['x'].clone()
    x[0, 1, 2, 2] = float('nan')
    x[c.N - 1, 0, 0, 0] = float('-inf')
    hit = torch.zeros(x.shape, dtype=torch.float64)
    hit[0, 1, 2, 2] = hit[c.N - 1, 0, 0, 0] = 1.0
    reached = F.conv2d(hit, torch.ones((c.O, c.C // c.groups, c.KH, c.KW), dtype=torch.float64), None, c.stride, c.pad, c.dil,
                       c.groups) > 0
    clean = _run(p, alpha=-1.0).cpu()
    for alpha in (-1.0, float('inf')):
        y = _run(p, x=x, alpha=alpha).cpu()
        finite = torch.isfinite(y)
        same = torch.equal(_bits(y)[~reached], _bits(clean)[~reached])
        print(f'{cid} {dt} alpha={alpha}: {int(reached.sum())} outputs read the NaN / -inf, {int((~finite).sum())} are not finite; '
              f'the others keep their bits: {same}')
        assert reached.any() and not reached.all() and torch.equal(~finite, reached) and same


# ------------------------------------------------------------------------------------------------ QuantConv2d
CLAMPS = ({'kind': 'identity'}, {'kind': 'symmetric', 'alpha': 2}, {'kind': 'symmetric', 'alpha': 1.3})
# (in channels, out channels, kernel, padding, stride, H = W, N): patch wide, patch strided wide, a 1x1 of a ragged chunk
LAYERS = ((64, 70, 3, 1, 1, 9, 5), (64, 70, 3, 1, 2, 9, 5), (65, 40, 1, 0, 1, 7, 5))


def _module(ws, cin, cout, ksz, clamp, seed, bias=True, **kw):
    from quant.binary.binary_conv import QuantConv2d
    m = QuantConv2d('fp', ws, cin, cout, ksz, clamp, bias=bias, **kw)
    detgen.fill_module(m, seed=seed)
    if ws != 'fp':
        with torch.no_grad():
            for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight, ws)):
                buf.copy_(v)
    return m


@pytest.fixture
def counters(monkeypatch):
    hip = _hip()
    names = {'half': 'signw_conv2d_half', 'signw': 'signw_conv2d', 'pack': 'pack_weight', 'prep': 'signw_prepare_weight'}
    calls = {name: 0 for name in names}
    real = {name: getattr(hip, attr) for name, attr in names.items()}

    def counted(name):
        def f(*a, **k):
            calls[name] += 1
            return real[name](*a, **k)
        return f

    for name, attr in names.items():
        monkeypatch.setattr(hip, attr, counted(name))
    return calls


def _input(name, layer, dtype):
    cin, _, _, _, _, hw, n = layer
    return detgen.normal(name, (n, cin, hw, hw), scale=1.3).to(DEV).to(dtype)


@pytest.mark.parametrize('dt', DTYPES)
def test_default_module_stays_on_torch(dt, counters):
    m = _module('ls-1', 64, 70, 3, CLAMPS[1], seed=51, padding=1).eval().to(DEV)
    x = _input('qconvhalf.default', LAYERS[0], DTYPES[dt])
    with torch.no_grad(), torch.autocast('cuda', dtype=x.dtype):      # (fp32 weights: torch itself needs the autocast)
        assert not m._wants_hip(x)
        y, ref = m(x), m._forward_torch(x)
    print(f'default {dt}: lsq_signw_conv2d_half {counters["half"]} calls, lsq_signw_conv2d {counters["signw"]} calls')
    assert torch.equal(y, ref) and y.dtype == x.dtype
    assert (counters['half'], counters['signw']) == (0, 0)


@pytest.mark.parametrize('li', range(len(LAYERS)))
@pytest.mark.parametrize('ws', ('ls-1', 'ls-2', 'ls-T', 'gf-3'))
@pytest.mark.parametrize('dt', DTYPES)
def test_module_forward(dt, ws, li, counters):
    """With fp_half: one kernel call and one weight pack (no prepared weight image: only lsq_signw_conv2d reads one), output dtype = input dtype, the same bits under an autocast of the
    type, within one rounding of the output type, (2^-8 | 2^-11) + 1e-5 of max |y64|, of the fp64 oracle; the cast route
    (fp_half_kernel = False) gives the same bits for bf16 on the patch layers."""
    i = ('ls-1', 'ls-2', 'ls-T', 'gf-3').index(ws)
    layer = LAYERS[li]
    cin, cout, ksz, pad, stride = layer[:5]
    clamp = CLAMPS[(i + li) % 3]
    m = _module(ws, cin, cout, ksz, clamp, seed=61 + i, bias=(i + li) % 2 == 0, padding=pad, stride=stride).eval().to(DEV)
    m.fp_half = True
    x = _input(f'qconvhalf.x.{i}', layer, DTYPES[dt])
    assert m._wants_hip(x)
    with torch.no_grad():
        y = m(x)
        assert (counters['half'], counters['signw'], counters['pack']) == (1, 0, 1)
        with torch.autocast('cuda', dtype=x.dtype):
            ya = m(x)
        assert (counters['half'], counters['signw'], counters['pack'], counters['prep']) == (2, 0, 1, 0)
        m.fp_half_kernel = False                  # the cast route asks for the fast path's weight image: built now, once
        y_cast = m(x)
        y_cast2 = m(x)
        assert (counters['half'], counters['signw'], counters['pack'], counters['prep']) == (2, 2, 1, 1)
        assert torch.equal(_bits(y_cast), _bits(y_cast2))
    assert y.dtype == x.dtype and ya.dtype == x.dtype and y_cast.dtype == x.dtype
    assert torch.equal(_bits(ya), _bits(y))
    alpha = m._alpha_in(x.dtype)
    xc = x.cpu().float()
    xc = xc.clamp(-alpha, alpha) if alpha >= 0 else xc
    wq = P.quantize_weight(m.weight.detach().cpu(), ws, [b.cpu() for b in m.w_approximate.cached_scales()])
    y64 = F.conv2d(xc.double(), wq.double(), None if m.bias is None else m.bias.detach().cpu().double(), stride, pad)
    err = ((y.cpu().double() - y64).abs().max() / y64.abs().max()).item()
    bound = (2.0 ** -8 if x.dtype == torch.bfloat16 else 2.0 ** -11) + BOUND
    differ_cast = (_bits(y) != _bits(y_cast)).sum().item()
    print(f'{ws} {dt} layer {layer} alpha={alpha}: max err / max|y64| = {err:.3e} (bound {bound:.3e}); {differ_cast} outputs differ '
          'from the cast route')
    assert err <= bound
    if dt == 'bf16' and li < 2:                   # (both libraries on a patch kernel: the same fp32 values, rounded once)
        assert differ_cast == 0


@pytest.mark.parametrize('dt', DTYPES)
def test_fused_forward_composes_on_a_sixteen_bit_input(dt, counters):
    """fused_forward with a batch norm in front, ReLU and a residual: the composition of the modules around m(x)."""
    layer = LAYERS[0]
    dtype = DTYPES[dt]
    m = _module('ls-2', 64, 70, 3, CLAMPS[1], seed=81, padding=1).eval().to(DEV)
    m.fp_half = True
    bn = torch.nn.BatchNorm2d(64).eval().to(DEV)
    with torch.no_grad():
        bn.running_mean.copy_(detgen.normal('qconvhalf.bn.m', (64,), scale=0.1))
        bn.running_var.copy_(detgen.uniform('qconvhalf.bn.v', (64,), 0.5, 1.5))
    x = _input('qconvhalf.fused', layer, dtype)
    res = detgen.normal('qconvhalf.res', (5, 70, 9, 9), scale=1.0).to(DEV).to(dtype)
    with torch.no_grad():
        y = m.fused_forward(x, pre_bn=bn, relu=True, res_pre=res)
        assert (counters['half'], counters['signw']) == (1, 0)
        ref = torch.relu(m(bn(x)) + res)
    print(f'fused_forward {dt}: {(_bits(y) != _bits(ref)).sum().item()} outputs differ from the composition')
    assert y.dtype == dtype and torch.equal(_bits(y), _bits(ref))
    assert (counters['half'], counters['signw']) == (2, 0)


@pytest.mark.parametrize('dt', DTYPES)
def test_channels_last_inputs_are_copied_first(dt, counters):
    m = _module('gf-3', 64, 70, 3, CLAMPS[1], seed=82, padding=1).eval().to(DEV)
    m.fp_half = True
    x = _input('qconvhalf.cl', LAYERS[0], DTYPES[dt])
    xl = x.to(memory_format=torch.channels_last)
    assert not xl.is_contiguous()
    with torch.no_grad():
        y, yl = m(x), m(xl)
    print(f'channels-last {dt}: {(_bits(y) != _bits(yl)).sum().item()} outputs differ from the contiguous copy')
    assert counters['half'] == 2 and counters['signw'] == 0
    assert torch.equal(_bits(y), _bits(yl))


def test_sixteen_bit_paths_that_stay_on_torch(counters):
    """Train mode, an input that wants a gradient, 16-bit weights, an autocast of the other type, fp weights: the torch
    formulation, neither convolution kernel -- with fp_half set."""
    x = detgen.normal('qconvhalf.torch.x', (3, 64, 6, 6), scale=1.2).to(DEV)
    bf, fp = torch.bfloat16, torch.float16

    def mod(ws, seed):
        m = _module(ws, 64, 20, 3, CLAMPS[1], seed=seed, padding=1).to(DEV)
        m.fp_half = True
        return m

    cases = [
        (mod('ls-1', 91).train(), x.to(bf), bf, False),
        (mod('gf-3', 92).eval(), x.to(bf).requires_grad_(True), bf, True),
        (mod('ls-1', 93).eval().bfloat16(), x.to(bf), None, False),
        (mod('ls-1', 94).eval(), x.to(fp), bf, False),
        (mod('fp', 95).eval(), x.to(bf), bf, False),
    ]
    for m, xin, autocast, grad in cases:
        with torch.set_grad_enabled(grad), torch.autocast('cuda', dtype=autocast or bf, enabled=autocast is not None):
            assert not m._wants_hip(xin)
            y = m(xin)
            ref = m._forward_torch(xin)
        assert torch.equal(y, ref)
    print(f'calls: lsq_signw_conv2d_half {counters["half"]}, lsq_signw_conv2d {counters["signw"]}')
    assert (counters['half'], counters['signw']) == (0, 0)
