"""lsq_linear_signw_half (liblsq_hip_linear_half.so) and QuantLinear('fp', w) with bf16 / fp16 inputs on the GPU: the kernel
against fp64 for every weight depth, the three clamps and the three kernels; the 16-bit output as the fp32 output rounded
once; bf16 against lsq_linear_signw; the output buffer, the workspace and unaligned inputs; determinism; refused calls that
write nothing; fp16 / bf16 subnormals through the matrix instruction (known answer); the module's dispatch and weight
cache, and the paths that must stay on torch.

Every test prints the figure it asserts on (pytest -s shows them)."""

import pytest
import torch
import torch.nn.functional as F

import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BOUND = 1e-5      # |y - y64| <= BOUND * max |y64|
E_UNSUPPORTED = -6
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
ALPHAS = (-1.0, 2.0, 1.3)         # identity, a bound both types hold, a bound neither holds (bf16: 1.296875, fp16: 1.2998046875)


def _hip():
    from quant import _hip
    return _hip


def _wscales(w, ws):
    """Scales [kw, O] of the sign planes lsq_pack_weight writes (ls-T: two planes of one scale) and the oracle's list."""
    o, f = w.shape
    try:
        sc = P.weight_scales(w.view(o, f, 1, 1), ws)
    except RuntimeError:              # rows too short for the scale solve (F = 1): any positive scales serve the kernel test
        k = {'ls-1': 1, 'ls-2': 2, 'ls-T': 1}.get(ws) or int(ws[3:])
        sc = [torch.full((o,), 0.6 ** q) for q in range(k)]
    planes = [sc[0], sc[0]] if ws == 'ls-T' else list(sc)
    return torch.stack(planes).contiguous(), sc


_CASES = {}


def _case(m, f, o, ws, dtype, alpha, bias, seed):
    """Operands on the GPU and the fp64 oracle F.linear(x16.clamp(-a, a).double(), w_q.double(), bias.double()); computed
    once per distinct case and shared (nothing below writes into a case)."""
    key = (m, f, o, ws, dtype, alpha, bias, seed)
    if key in _CASES:
        return _CASES[key]
    hip = _hip()
    x = detgen.normal(f'linhalf.x.{seed}', (m, f), seed=seed, scale=1.2).to(dtype)
    w = detgen.uniform(f'linhalf.w.{seed}', (o, f), -0.5, 0.5, seed=seed)
    wsc, sc = _wscales(w, ws)
    g = hip.make_geom(1, f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    wbits, _ = hip.pack_weight(w.to(DEV).view(o, f, 1, 1), g, wsc.to(DEV))
    b = detgen.normal(f'linhalf.b.{seed}', (o,), seed=seed, scale=0.5) if bias else None
    xd = x.to(DEV)
    xc = xd.clamp(-alpha, alpha) if alpha >= 0 else xd
    assert xc.dtype == dtype
    wq = P.quantize_weight(w.view(o, f, 1, 1), ws, sc).view(o, f)
    y64 = F.linear(xc.double(), wq.double().to(DEV), None if b is None else b.double().to(DEV)).cpu()
    c = dict(x=xd, wbits=wbits, wsc=wsc.to(DEV), b=None if b is None else b.to(DEV), alpha=alpha, m=m, f=f, o=o, dtype=dtype,
             y64=y64)
    if len(_CASES) >= 8:
        _CASES.pop(next(iter(_CASES)))
    _CASES[key] = c
    return c


def _run(c, x=None, out_dtype=torch.float32):
    return _hip().linear_signw_half(c['x'] if x is None else x, c['alpha'], c['wbits'], c['wsc'], c['b'], c['m'], c['f'], c['o'],
                                    out_dtype=out_dtype)


def _check(c, y, what=''):
    y64 = c['y64']
    err = (y.cpu().double() - y64).abs().max().item()
    scale = y64.abs().max().item()
    print(f'{what} M={c["m"]} F={c["f"]} O={c["o"]} {c["dtype"]} alpha={c["alpha"]}: max err / max|y64| = {err / scale:.3e}')
    assert err <= BOUND * scale, (c['m'], c['f'], c['o'], err / scale)
    return err / scale


def _bits(y):
    return y.contiguous().view(torch.int32 if y.dtype == torch.float32 else torch.int16)


WS = ('ls-1', 'ls-2', 'ls-T', 'gf-2', 'gf-3', 'gf-8')
FS = (1, 63, 64, 65, 800)
OS = (1, 10, 33, 1000)
MS = (1, 7, 16, 256)


@pytest.mark.parametrize('ws', WS)
@pytest.mark.parametrize('fi', range(len(FS)))
@pytest.mark.parametrize('dt', DTYPES)
def test_kernel_against_fp64(dt, ws, fi):
    """Both types x every weight depth x every feature count, fp32 output; out-features, rows, clamp and bias rotate so that
    every value of each meets several depths.  Only the fp32 rounding of the accumulation is left: 1e-5 of max |y64| is the
    project's bound, lsq_linear_signw's measured 2e-6 the guide."""
    wi, di = WS.index(ws), list(DTYPES).index(dt)
    f, o, m = FS[fi], OS[(fi + wi) % 4], MS[(fi + 2 * wi) % 4]
    c = _case(m, f, o, ws, DTYPES[dt], ALPHAS[(fi + wi + di) % 3], bias=(fi // 2 + wi) % 2 == 0, seed=100 * wi + fi)
    _check(c, _run(c), f'fp64 {ws}')


TILED = [(1000, 65, 1033, 'gf-3'), (2040, 72, 2050, 'ls-2'), (300, 1, 4100, 'ls-T')]


@pytest.mark.parametrize('i', range(len(TILED)))
@pytest.mark.parametrize('dt', DTYPES)
def test_tiled_kernel_edges(dt, i):
    """64 x 64 tiles, 128 x 128 tiles and the F = 1 edge, ragged rows and columns; fp32 and 16-bit output."""
    m, f, o, ws = TILED[i]
    assert _tile_class(m, o) == ('small', 'big', 'small')[i]
    c = _case(m, f, o, ws, DTYPES[dt], ALPHAS[(i + 1) % 3], bias=i % 2 == 0, seed=300 + i)
    y32 = _run(c)
    _check(c, y32, f'tiled {ws}')
    y16 = _run(c, out_dtype=c['dtype'])
    assert torch.equal(_bits(y16), _bits(y32.to(c['dtype'])))


def _tile_class(m, o):
    from quant.binary import QuantLinear
    return QuantLinear._tile_class(m, o)


SHAPES3 = [(16, 800, 1000), (1024, 136, 1000), (2048, 136, 2048)]       # split, 64 x 64 tiles, 128 x 128 tiles


@pytest.mark.parametrize('shape', SHAPES3)
@pytest.mark.parametrize('ws', ('ls-1', 'ls-2', 'gf-3', 'gf-8'))
@pytest.mark.parametrize('dt', DTYPES)
def test_sixteen_bit_output_is_the_fp32_output_rounded_once(dt, ws, shape):
    """One, two, three and eight planes (one, one, two and four launches): no intermediate is ever rounded to 16 bits."""
    m, f, o = shape
    assert _tile_class(m, o) == ('split', 'small', 'big')[SHAPES3.index(shape)]
    wi = WS.index(ws)
    c = _case(m, f, o, ws, DTYPES[dt], ALPHAS[(wi + 1) % 3], bias=wi % 2 == 0, seed=800 + wi)
    y32, y16 = _run(c), _run(c, out_dtype=c['dtype'])
    assert y16.dtype == c['dtype'] and y32.dtype == torch.float32
    diff = (_bits(y16) != _bits(y32.to(c['dtype']))).sum().item()
    print(f'rounded once {ws} {shape} {dt}: {diff} of {m * o} outputs differ')
    assert diff == 0
    _check(c, y32, f'rounded once {ws}')


@pytest.mark.parametrize('shape', SHAPES3)
@pytest.mark.parametrize('alpha', (-1.0, 2.0))
def test_bf16_equals_the_fp32_kernel(shape, alpha):
    """lsq_linear_signw on x.float() adds, besides the same hi products in the same order, lo products that are all zero
    (values, not bit patterns: adding +0 turns a -0 into +0)."""
    m, f, o = shape
    i = SHAPES3.index(shape)
    c = _case(m, f, o, ('gf-3', 'ls-2', 'ls-1')[i], torch.bfloat16, alpha, bias=i != 1, seed=900 + i)
    y = _run(c)
    ref = _hip().linear_signw(c['x'].float(), alpha, c['wbits'], c['wsc'], c['b'], m, f, o)
    differ = (y != ref).sum().item()
    print(f'bf16 vs lsq_linear_signw {shape} alpha={alpha}: {differ} of {m * o} values differ')
    assert torch.equal(y, ref)


# ------------------------------------------------------------------------------------------------ output buffer, alignment
def _raw_call(c, x_ptr, y_ptr, ydt, kw=None, xdt=None, ws=None, stream=None):
    hip = _hip()
    code = hip.LINEAR_HALF_DTYPES
    return hip.linear_half_lib().lsq_linear_signw_half(
        x_ptr, code[c['dtype']] if xdt is None else xdt, c['alpha'], c['wbits'].data_ptr(),
        c['wsc'].shape[0] if kw is None else kw, c['wsc'].data_ptr(), None if c['b'] is None else c['b'].data_ptr(),
        c['m'], c['f'], c['o'], y_ptr, code[ydt], None if ws is None else ws.data_ptr(), 0 if ws is None else 4 * ws.numel(), stream)


@pytest.mark.parametrize('ws', ('ls-2', 'gf-3'))
@pytest.mark.parametrize('dt', DTYPES)
def test_sixteen_bit_output_buffer_at_a_two_byte_offset(dt, ws):
    """y with odd O and odd M * O at an address 2 bytes past a dword inside a NaN-filled buffer: written exactly in place,
    nothing beside it touched (its first and last element share a dword with the padding).  gf-3: the fp32 running sum in a
    workspace of exactly the size the library asks for, inside a sentinel-filled buffer of its own."""
    m, f, o = 7, 65, 33
    dtype = DTYPES[dt]
    c = _case(m, f, o, ws, dtype, 2.0, bias=True, seed=500)
    hip = _hip()
    pad = 37
    buf = torch.full((pad + m * o + pad,), float('nan'), dtype=dtype, device=DEV)
    y_ptr = buf.data_ptr() + 2 * pad
    assert y_ptr % 4 == 2 and (m * o) % 2 == 1
    need = hip.linear_half_lib().lsq_linear_signw_half_workspace_bytes(m, o, c['wsc'].shape[0], hip.LINEAR_HALF_DTYPES[dtype])
    assert need == (4 * m * o if ws == 'gf-3' else 0)
    wsbuf = torch.full((pad + need // 4 + pad,), 12345.0, device=DEV)
    work = wsbuf[pad:pad + need // 4] if need else None
    assert _raw_call(c, c['x'].data_ptr(), y_ptr, dtype, ws=work) == 0
    torch.cuda.synchronize()
    y = buf[pad:pad + m * o].view(m, o)
    assert not torch.isnan(y).any()
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + m * o:]).all()
    assert (wsbuf[:pad] == 12345.0).all() and (wsbuf[pad + need // 4:] == 12345.0).all()
    assert torch.equal(_bits(y), _bits(_run(c).to(dtype)))


@pytest.mark.parametrize('shape', SHAPES3)
@pytest.mark.parametrize('dt', DTYPES)
def test_unaligned_input_gives_the_same_bits(dt, shape):
    """x at an address 2 bytes past a 16-byte boundary against the aligned x, with F % 8 == 0: the 2-byte and the 16-byte
    load paths of each of the three kernels."""
    m, f, o = shape
    i = SHAPES3.index(shape)
    assert f % 8 == 0
    c = _case(m, f, o, ('gf-3', 'ls-2', 'ls-1')[i], DTYPES[dt], ALPHAS[(i + 2) % 3], bias=True, seed=900 + i)
    assert c['x'].data_ptr() % 16 == 0
    xbuf = torch.empty((m * f + 1,), dtype=c['dtype'], device=DEV)
    xbuf[1:] = c['x'].view(-1)
    xu = xbuf[1:].view(m, f)
    assert xu.data_ptr() % 16 == 2
    for out_dtype in (torch.float32, c['dtype']):
        assert torch.equal(_bits(_run(c, xu, out_dtype)), _bits(_run(c, out_dtype=out_dtype)))


@pytest.mark.parametrize('shape', [(16, 4096, 4096, 'ls-2'), (1024, 136, 1000, 'gf-3')])
@pytest.mark.parametrize('dt', DTYPES)
def test_two_calls_give_the_same_bits(dt, shape):
    m, f, o, ws = shape
    c = _case(m, f, o, ws, DTYPES[dt], -1.0, bias=True, seed=600 + m)
    for out_dtype in (torch.float32, c['dtype']):
        y1, y2 = _run(c, out_dtype=out_dtype), _run(c, out_dtype=out_dtype)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            y3 = _run(c, out_dtype=out_dtype)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for y in (y2, y3):
            assert torch.equal(_bits(y1), _bits(y))


def test_refused_calls_write_nothing():
    c = _case(16, 128, 40, 'gf-8', torch.bfloat16, 2.0, bias=True, seed=700)
    work = torch.empty((16 * 40,), device=DEV)
    for ydt, kw in ((torch.float32, dict(kw=9)), (torch.bfloat16, dict(kw=9)), (torch.float32, dict(xdt=0)),
                    (torch.bfloat16, dict(xdt=0)), (torch.float16, {})):
        y = torch.full((16, 40), 12345.0, dtype=ydt, device=DEV)
        assert _raw_call(c, c['x'].data_ptr(), y.data_ptr(), ydt, ws=work, **kw) == E_UNSUPPORTED, (ydt, kw)
        torch.cuda.synchronize()
        assert (y == 12345.0).all()
    with pytest.raises(TypeError):
        _run(c, out_dtype=torch.float16)


@pytest.mark.parametrize('dt', DTYPES)
def test_subnormal_activations_known_answer(dt):
    """One row of 64 subnormals k * (smallest subnormal), k = 1 .. 64, against an all +1 ls-1 plane of scale 1: the exact sum
    2080 * (smallest subnormal) if the matrix instruction takes subnormal A operands as they are, exactly 0 if it flushes
    them; nothing else passes.  Measured on an MI355X: the exact sum, for fp16 and for bf16 (the header says so)."""
    hip = _hip()
    dtype = DTYPES[dt]
    tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133
    x = (torch.arange(1, 65, dtype=torch.float64) * tiny).to(dtype).view(1, 64)
    assert torch.equal(x.double(), torch.arange(1, 65, dtype=torch.float64).view(1, 64) * tiny)
    assert (x.float().abs() < torch.finfo(dtype).tiny).all()
    g = hip.make_geom(1, 64, 1, 1, 1, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    ones = torch.ones((1, 1), device=DEV)
    wbits, _ = hip.pack_weight(torch.full((1, 64, 1, 1), 0.5, device=DEV), g, ones)
    y = hip.linear_signw_half(x.to(DEV), -1.0, wbits, ones, None, 1, 64, 1, out_dtype=torch.float32)
    got, exact = y.item(), 2080 * tiny
    print(f'{dt} subnormals: got {got!r}, exact sum {exact!r}: {"kept" if got == exact else "flushed" if got == 0 else "?"}')
    assert got in (exact, 0.0)
    # the same row scaled into the normal range, so that a wrong plane or row would show
    yn = hip.linear_signw_half((x.double() / tiny).to(dtype).to(DEV), -1.0, wbits, ones, None, 1, 64, 1,
                               out_dtype=torch.float32)
    assert yn.item() == 2080.0


# ------------------------------------------------------------------------------------------------ QuantLinear('fp', w)
def _module(ws, f, o, clamp, seed, bias=True, xq='fp'):
    from quant.binary import QuantLinear
    m = QuantLinear(xq, ws, f, o, clamp, bias=bias)
    detgen.fill_module(m, seed=seed)
    with torch.no_grad():
        for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight.view(o, f, 1, 1), ws)):
            buf.copy_(v)
    return m


@pytest.fixture
def counters(monkeypatch):
    hip = _hip()
    calls = {'half': 0, 'signw': 0, 'pack': 0}
    real = {'half': hip.linear_signw_half, 'signw': hip.linear_signw, 'pack': hip.pack_weight}

    def counted(name):
        def f(*a, **k):
            calls[name] += 1
            return real[name](*a, **k)
        return f

    monkeypatch.setattr(hip, 'linear_signw_half', counted('half'))
    monkeypatch.setattr(hip, 'linear_signw', counted('signw'))
    monkeypatch.setattr(hip, 'pack_weight', counted('pack'))
    calls['real'] = real
    return calls


def _kernel_reference(m, x, counters):
    """The fp32-output kernel result on the module's own packed planes, cast to x's type."""
    hip = _hip()
    wbits, _, wscales = m._packed_weights(hip)
    rows = x.detach().reshape(-1, m.in_features).contiguous()
    bias = None if m.bias is None else m.bias.detach()
    y32 = counters['real']['half'](rows, m._alpha(), wbits, wscales, bias, rows.shape[0], m.in_features, m.out_features,
                                   out_dtype=torch.float32)
    return y32.to(x.dtype).view(*x.shape[:-1], m.out_features)


def _expect_one_forward(m, x, counters, before):
    rows = x.numel() // m.in_features
    took_kernel = m._tile_class(rows, m.out_features) in m.half_kernel_classes
    assert counters['half'] - before[0] == (1 if took_kernel else 0)
    assert counters['signw'] - before[1] == (0 if took_kernel else 1)


CLAMPS = ({'kind': 'identity'}, {'kind': 'symmetric', 'alpha': 2}, {'kind': 'symmetric', 'alpha': 1.3})


@pytest.mark.parametrize('shape', [(9, 100), (4, 3, 100), (2, 5, 7, 65)])
@pytest.mark.parametrize('ws', ('ls-1', 'ls-2', 'gf-3'))
@pytest.mark.parametrize('dt', DTYPES)
def test_quant_linear_eval_takes_sixteen_bit_inputs(dt, ws, shape, counters):
    i = ('ls-1', 'ls-2', 'gf-3').index(ws)
    clamp = CLAMPS[(i + len(shape)) % 3]
    f, o = shape[-1], 70
    m = _module(ws, f, o, clamp, seed=31 + i, bias=len(shape) != 3).eval().to(DEV)
    x = detgen.normal(f'qlinhalf.x.{i}', shape, scale=1.3).to(DEV).to(DTYPES[dt])
    with torch.no_grad():
        y = m(x)
    _expect_one_forward(m, x, counters, (0, 0))
    assert y.shape == (*shape[:-1], o) and y.dtype == x.dtype
    ref = _kernel_reference(m, x, counters)
    assert torch.equal(_bits(y), _bits(ref))
    with torch.no_grad(), torch.autocast('cuda', dtype=x.dtype):
        ya = m(x)
    assert ya.dtype == x.dtype and torch.equal(_bits(ya), _bits(y))
    assert counters['half'] + counters['signw'] == 2
    # and against fp64, at the resolution of the 16-bit output plus the kernel's: rounding to nearest moves a value by at most
    # half an ulp, 2^-8 of it for bf16 (8 significant bits) and 2^-11 for fp16 (11)
    wq = P.quantize_weight(m.weight.detach().cpu().view(o, f, 1, 1), ws, [b.cpu() for b in m.w_approximate.cached_scales()])
    xc = x.cpu().clamp(-clamp['alpha'], clamp['alpha']) if clamp['kind'] == 'symmetric' else x.cpu()
    y64 = F.linear(xc.double(), wq.view(o, f).double(), None if m.bias is None else m.bias.detach().cpu().double())
    err = ((y.cpu().double() - y64).abs().max() / y64.abs().max()).item()
    print(f'module {dt} {ws} {shape}: max err / max|y64| = {err:.3e}')
    assert err <= (2.0 ** -8 if x.dtype == torch.bfloat16 else 2.0 ** -11) + BOUND, err
    assert not hasattr(m, 'last_act_scales')


@pytest.mark.parametrize('dt', DTYPES)
def test_quant_linear_eval_takes_strided_sixteen_bit_inputs(dt, counters):
    f, o = 100, 40
    m = _module('ls-2', f, o, CLAMPS[1], seed=45).eval().to(DEV)
    h = detgen.normal('qlinhalf.stride.h', (6, 5, f), scale=1.3).to(DEV).to(DTYPES[dt])
    wide = detgen.normal('qlinhalf.stride.w', (4, 3, f + 7), scale=1.3).to(DEV).to(DTYPES[dt])
    for x in (h[:, 0], wide[..., :f], wide[..., 7:]):
        assert not x.is_contiguous()
        before = (counters['half'], counters['signw'])
        with torch.no_grad():
            y = m(x)
        _expect_one_forward(m, x, counters, before)
        assert y.shape == (*x.shape[:-1], o) and y.dtype == x.dtype
        assert torch.equal(_bits(y), _bits(_kernel_reference(m, x.contiguous(), counters)))


def test_fp32_and_sixteen_bit_forwards_share_the_packed_weights(counters):
    m = _module('ls-2', 200, 50, CLAMPS[1], seed=41).eval().to(DEV)
    x = detgen.normal('qlinhalf.cache.x', (6, 200)).to(DEV)
    with torch.no_grad():
        y32 = m(x)
        assert (counters['pack'], counters['signw'], counters['half']) == (1, 1, 0)       # fp32: lsq_linear_signw as before
        before = (counters['half'], counters['signw'])
        yb = m(x.bfloat16())
        _expect_one_forward(m, x, counters, before)
        yh = m(x.half())
        assert counters['pack'] == 1
    assert y32.dtype == torch.float32 and yb.dtype == torch.bfloat16 and yh.dtype == torch.float16
    # the 16-bit forwards see x rounded into their type (|x16 - x| <= eps |x|, eps = 2^-8 / 2^-11; the clamp does not widen
    # that) and round y once (eps |y|): |y16 - y32| <= eps (sum_f |x_f| |w_q[o][f]| + |y|) + the fp32 kernels' own 1e-5
    with torch.no_grad():
        wq = m.w_approximate(m.weight.view(50, 200, 1, 1)).view(50, 200)
        reach = F.linear(x.abs(), wq.abs()) + y32.abs()
    for y16, eps in ((yb, 2.0 ** -8), (yh, 2.0 ** -11)):
        excess = ((y16.float() - y32).abs() - eps * reach).max().item()
        print(f'{y16.dtype} against the fp32 forward: largest |y16 - y32| - eps * reach = {excess:.3e}')
        assert excess <= 2 * BOUND * y32.abs().max().item()


def test_sixteen_bit_paths_that_stay_on_torch(counters):
    """Train mode, an input that wants a gradient, 16-bit weights, binary activations, an autocast of another type: the torch
    formulation (whatever torch makes of the types), never the kernels."""
    x = detgen.normal('qlinhalf.torch.x', (5, 3, 96), scale=1.2).to(DEV)
    bf, fp = torch.bfloat16, torch.float16
    cases = [
        (_module('ls-1', 96, 20, CLAMPS[1], seed=51).to(DEV).train(), x.to(bf), bf, False),
        (_module('ls-2', 96, 20, CLAMPS[1], seed=52).eval().to(DEV), x.to(bf).requires_grad_(True), bf, True),
        (_module('ls-1', 96, 20, CLAMPS[1], seed=53).eval().to(DEV).bfloat16(), x.to(bf), None, False),
        (_module('ls-1', 128, 20, CLAMPS[1], seed=54, xq='ls-2').eval().to(DEV), x.to(bf).reshape(5, 3 * 96)[:, :128].contiguous(),
         bf, False),
        (_module('ls-1', 96, 20, CLAMPS[1], seed=55).eval().to(DEV), x.to(fp), bf, False),
    ]
    for mod, xin, autocast, grad in cases:
        with torch.set_grad_enabled(grad), torch.autocast('cuda', dtype=autocast or bf, enabled=autocast is not None):
            assert not mod._wants_hip(xin)
            y = mod(xin)
            ref = mod._forward_torch(xin)
        assert torch.equal(y, ref)
    assert (counters['half'], counters['signw']) == (0, 0)
