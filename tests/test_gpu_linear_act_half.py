"""lsq_linear_act_quant_half (liblsq_hip_linear_act_half.so) and QuantLinear with binary activations on bf16 / fp16 inputs on
the GPU: the planes against a CPU fp32 restatement of the chain and against lsq_act_quant on x.float(); the scales against
the fp64 mean of the fp32 magnitudes; invariance to the batch, determinism; zeros, -0.0, subnormals, pre-filled planes, guard
words, unaligned rows, refused calls; the module's dispatch, both routes, the counters and the paths that stay on torch.

Every test prints the figure it asserts on (pytest -s shows them)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}
ALPHAS = (-1.0, 2.0, 1.3)         # identity, a bound both types hold, a bound neither holds (bf16: 1.296875, fp16: 1.2998046875)
LS1, LS2, LST, GF = 1, 2, 3, 4
E_UNSUPPORTED = -6
# |v - v64| <= SCALE_BOUND * v64 against the fp64 mean of the fp32 magnitudes: derived, not measured -- the fp32 sum of 8
# non-negative terms carries at most 7 roundings of 2^-24, the final conversion to fp32 one more
SCALE_BOUND = 2.0 ** -21
GUARD = 5                         # words / floats around planes and scales
SENTINEL_WORD, SENTINEL_SCALE = 0x5A5A5A5A5A5A5A5A, 12345.0


def _hip():
    from quant import _hip
    return _hip


def _rounded(alpha, dtype):
    return torch.tensor(alpha, dtype=dtype).item() if alpha >= 0 else alpha


def _nw(L):
    return (L + 63) // 64


def _quant(x, scheme, k, alpha, forced=None, fill=SENTINEL_WORD):
    """The kernel on x [N, L] (on the GPU) with `alpha` already a value of x's type; planes pre-filled with `fill`, planes and
    scales inside guard words that must come back untouched.  Returns (planes [k, N, nw] int64, scales [k, N]) on the CPU."""
    hip = _hip()
    n, L = x.shape
    words = k * n * _nw(L)
    pbuf = torch.full((GUARD + words + GUARD,), fill, dtype=torch.int64, device=DEV)
    pbuf[:GUARD] = SENTINEL_WORD
    pbuf[GUARD + words:] = SENTINEL_WORD
    sbuf = torch.full((GUARD + k * n + GUARD,), SENTINEL_SCALE, device=DEV)
    planes, scales = pbuf[GUARD:GUARD + words], sbuf[GUARD:GUARD + k * n].view(k, n)
    hip.linear_act_quant_half(x, scheme, k, alpha, planes, scales, forced)
    torch.cuda.synchronize()
    assert (pbuf[:GUARD] == SENTINEL_WORD).all() and (pbuf[GUARD + words:] == SENTINEL_WORD).all()
    assert (sbuf[:GUARD] == SENTINEL_SCALE).all() and (sbuf[GUARD + k * n:] == SENTINEL_SCALE).all()
    return planes.view(k, n, _nw(L)).cpu(), scales.cpu().clone()


def _chain(xf, alpha, scales):
    """CPU fp32 restatement of the chain on xf [N, L] fp32 with scales [k, N]: (bits [k, N, L] bool, |res_q| [k, N, L] fp32)."""
    c = xf.clamp(-alpha, alpha) if alpha >= 0 else xf
    result, res = torch.zeros_like(c), c.clone()
    bits, mags = [], []
    for q in range(scales.shape[0]):
        v = scales[q].view(-1, 1)
        b = (c - result) >= 0
        bits.append(b)
        mags.append(res.abs())
        result = result + torch.where(b, v, -v)
        res = res - torch.where(res >= 0, v, -v)
    return torch.stack(bits), torch.stack(mags)


def _pack(bits):
    """[k, N, L] bool -> [k, N, nw] int64: bit i of word w is element 64 w + i, bits past L are 0."""
    k, n, L = bits.shape
    padded = np.zeros((k, n, _nw(L) * 64), dtype=np.uint8)
    padded[:, :, :L] = bits.numpy()
    words = np.packbits(padded.reshape(k, n, _nw(L), 64), axis=-1, bitorder='little').view('<u8').reshape(k, n, _nw(L))
    return torch.from_numpy(words.view(np.int64).copy())


def _act_quant_reference(x, scheme, k, alpha, scales):
    """lsq_act_quant on x.float() with the given scales: the existing kernel is the reference for the layout."""
    hip = _hip()
    n, L = x.shape
    geom = hip.make_geom(n, L, 1, 1, 1, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    planes = torch.zeros((k * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    out = torch.empty((k, n), device=DEV)
    hip.act_quant(x.float(), geom, scheme, k, 3, alpha, planes, out, scales.to(DEV).contiguous())
    torch.cuda.synchronize()
    return planes.view(k, n, _nw(L)).cpu()


def _check_scales(scales, mags, what, check=True):
    """Each v_q against the fp64 mean of the fp32 magnitudes built from the kernel's own earlier scales."""
    v64 = mags.double().mean(dim=2)
    rel = ((scales.double() - v64).abs() / v64.clamp_min(1e-300)).max().item()
    print(f'{what}: max |v - v64| / v64 = {rel:.3e} (bound {SCALE_BOUND:.3e})')
    assert not check or ((scales.double() - v64).abs() <= SCALE_BOUND * v64).all(), (what, rel)
    return rel


_X = {}


def _rows(n, L, dtype, seed):
    """x [n, L] of the type on the GPU; computed once per distinct case and shared (nothing writes into it)."""
    key = (n, L, dtype, seed)
    if key not in _X:
        if len(_X) >= 6:
            _X.pop(next(iter(_X)))
        _X[key] = detgen.normal(f'actquanthalf.x.{seed}', (n, L), seed=seed, scale=1.2).to(dtype).to(DEV)
    return _X[key]


# (name, LSQ_SCHEME_*, k, scales given)
CASES = [('ls-1', LS1, 1, False), ('gf-1', GF, 1, False), ('gf-3', GF, 3, False), ('gf-8', GF, 8, False),
         ('ls-1 given', LS1, 1, True), ('ls-2 given', LS2, 2, True), ('ls-T given', LST, 2, True), ('gf-3 given', GF, 3, True)]
LS = (1, 63, 64, 65, 800, 4104, 70001)
NS = (1, 7, 300)


def _given(k, n, seed):
    """Per-sample scales of a decreasing chain, the ternary pair equal."""
    base = detgen.uniform(f'actquanthalf.v.{seed}', (1, n), 0.5, 1.1, seed=seed)
    return torch.cat([base * 0.55 ** q for q in range(k)]).contiguous()


@pytest.mark.parametrize('ci', range(len(CASES)))
@pytest.mark.parametrize('dt', DTYPES)
def test_planes_and_scales(dt, ci):
    """Every row length (a word minus one, a word, a word plus one, one element; one wave a row with 16-byte loads; one
    workgroup a row with the row kept in LDS; one workgroup a row read again per plane) x batch sizes and clamps in
    rotation: planes equal the CPU chain with the kernel's own scales and lsq_act_quant's on x.float() with those scales;
    computed scales within the derived bound of the fp64 mean; given scales copied."""
    name, scheme, k, given = CASES[ci]
    dtype, di = DTYPES[dt], list(DTYPES).index(dt)
    for li, L in enumerate(LS):
        n = NS[(li + ci + di) % 3] if L < 70001 else (1, 7)[(ci + di) % 2]
        alpha = _rounded(ALPHAS[(li + ci + 2 * di) % 3], dtype)
        x = _rows(n, L, dtype, seed=li)
        forced = _given(2 if scheme == LST else k, n, seed=ci)
        if scheme == LST:
            forced = forced[[0, 0]].contiguous()
        planes, scales = _quant(x, scheme, k, alpha, forced.to(DEV) if given else None)
        bits, mags = _chain(x.cpu().float(), alpha, scales)
        wrong = (planes != _pack(bits)).sum().item()
        ref = _act_quant_reference(x, scheme, k, alpha, scales)
        wrong_ref = (planes != ref).sum().item()
        print(f'{name} {dt} N={n} L={L} alpha={alpha}: {wrong} words differ from the CPU chain, {wrong_ref} from lsq_act_quant')
        assert wrong == 0 and torch.equal(planes, ref)
        if given:
            assert torch.equal(scales, forced)
        else:
            _check_scales(scales, mags, f'{name} {dt} N={n} L={L}')


@pytest.mark.parametrize('dt', DTYPES)
def test_rows_read_again_with_sixteen_byte_loads(dt):
    """A row beyond what a workgroup keeps in LDS whose length is a multiple of 8 (the planes test's long row is odd)."""
    dtype = DTYPES[dt]
    n, L, k = 3, 20000, 3
    x = _rows(n, L, dtype, seed=20)
    alpha = _rounded(1.3, dtype)
    planes, scales = _quant(x, GF, k, alpha)
    bits, mags = _chain(x.cpu().float(), alpha, scales)
    assert torch.equal(planes, _pack(bits))
    _check_scales(scales, mags, f'gf-3 {dt} N={n} L={L}')


@pytest.mark.parametrize('dt', DTYPES)
def test_scale_of_a_long_row(dt):
    dtype = DTYPES[dt]
    L = (1 << 20) + 3
    x = _rows(1, L, dtype, seed=30)
    for name, scheme, k in (('ls-1', LS1, 1), ('gf-2', GF, 2)):
        planes, scales = _quant(x, scheme, k, 2.0)
        bits, mags = _chain(x.cpu().float(), 2.0, scales)
        assert torch.equal(planes, _pack(bits))
        _check_scales(scales, mags, f'{name} {dt} L={L}')


@pytest.mark.parametrize('dt', DTYPES)
def test_ls1_scales_against_lsq_act_quant(dt):
    """How many ls-1 scales are bit-equal to lsq_act_quant(x.float()): printed, not asserted (the two kernels add in
    different orders); the new kernel's are within the bound of the fp64 mean, the other's distance is printed beside it."""
    hip = _hip()
    dtype = DTYPES[dt]
    equal = total = 0
    for n, L in ((300, 800), (7, 4104), (64, 4096)):
        x = _rows(n, L, dtype, seed=40)
        _, scales = _quant(x, LS1, 1, 2.0)
        geom = hip.make_geom(n, L, 1, 1, 1, 1, 1, (1, 1), (0, 0), (1, 1), 1)
        planes = torch.zeros((hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
        ref = torch.empty((1, n), device=DEV)
        hip.act_quant(x.float(), geom, LS1, 1, 3, 2.0, planes, ref)
        ref = ref.cpu()
        equal += (scales.view(torch.int32) == ref.view(torch.int32)).sum().item()
        total += n
        mags = x.cpu().float().clamp(-2, 2).abs().unsqueeze(0)
        _check_scales(scales, mags, f'ls-1 {dt} N={n} L={L}')
        _check_scales(ref, mags, f'lsq_act_quant ls-1 {dt} N={n} L={L}', check=False)
    print(f'ls-1 {dt}: {equal} of {total} scales bit-equal to lsq_act_quant(x.float())')


@pytest.mark.parametrize('L', (800, 4104, 20000))
@pytest.mark.parametrize('dt', DTYPES)
def test_a_rows_result_does_not_depend_on_the_batch(dt, L):
    """The same row alone and as row 0, 150 and 299 of a batch: the same scale bits and plane words; two runs: the same bits."""
    dtype = DTYPES[dt]
    batch = _rows(300, L, dtype, seed=50).clone()
    row = batch[17].clone()
    for r in (0, 150, 299):
        batch[r] = row
    alpha = _rounded(1.3, dtype)
    for name, scheme, k in (('ls-1', LS1, 1), ('gf-3', GF, 3)):
        p1, s1 = _quant(row.view(1, L), scheme, k, alpha)
        pb, sb = _quant(batch, scheme, k, alpha)
        pb2, sb2 = _quant(batch, scheme, k, alpha)
        differ = sum((sb[:, r].view(torch.int32) != s1[:, 0].view(torch.int32)).sum().item() + (pb[:, r] != p1[:, 0]).sum().item()
                     for r in (0, 150, 299, 17))
        print(f'{name} {dt} L={L}: {differ} scale / plane words differ between the row alone and in the batch')
        assert differ == 0
        assert torch.equal(pb, pb2) and torch.equal(sb.view(torch.int32), sb2.view(torch.int32))


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize('dt', DTYPES)
def test_zero_rows_and_negative_zero(dt):
    """An all-zero row and a row of -0.0: scale 0, every bit 1 up to L, 0 past it (planes pre-filled with zeros AND with ones)."""
    dtype = DTYPES[dt]
    for L in (65, 800, 4104):
        x = torch.zeros((2, L), dtype=dtype)
        x[1] = -0.0
        assert (x[1].view(torch.int16) == -32768).all()
        want = _pack(torch.ones((1, 2, L), dtype=torch.bool))
        for name, scheme, k in (('ls-1', LS1, 1), ('gf-3', GF, 3)):
            for fill in (0, -1):
                planes, scales = _quant(x.to(DEV), scheme, k, 2.0, fill=fill)
                print(f'{name} {dt} L={L} fill={fill}: scales {scales.flatten().tolist()}, last word {planes[0, 1, -1].item():#x}')
                assert (scales == 0).all() and not torch.signbit(scales).any()
                assert all(torch.equal(planes[q:q + 1], want) for q in range(k))


@pytest.mark.parametrize('dt', DTYPES)
def test_negative_subnormals(dt):
    """64 negative subnormals -k * (smallest subnormal), k = 1 .. 64: every bit 0 (a flushed value would be -0.0: bit 1), the
    scale within the bound of their fp64 mean (a flushed row would give 0)."""
    dtype = DTYPES[dt]
    tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133
    x = (-torch.arange(1, 65, dtype=torch.float64) * tiny).to(dtype).view(1, 64)
    assert torch.equal(x.double(), -torch.arange(1, 65, dtype=torch.float64).view(1, 64) * tiny)
    assert (x.float().abs() < torch.finfo(dtype).tiny).all()
    planes, scales = _quant(x.to(DEV), LS1, 1, -1.0)
    v64 = 32.5 * tiny
    print(f'{dt} subnormals: plane word {planes.item():#x}, scale {scales.item()!r}, fp64 mean {v64!r}')
    assert planes.item() == 0
    assert abs(scales.item() - v64) <= SCALE_BOUND * v64
    planes, scales = _quant((-x).to(DEV), GF, 2, 2.0)
    assert planes[0].item() == -1 and abs(scales[0].item() - v64) <= SCALE_BOUND * v64


@pytest.mark.parametrize('dt', DTYPES)
def test_prefilled_planes_come_out_with_zero_tails(dt):
    """planes pre-filled with all ones: every word is written in full, the bits past L are 0."""
    dtype = DTYPES[dt]
    for L in (1, 63, 65, 4104 + 5):
        x = _rows(7, L, dtype, seed=60)
        for scheme, k, forced in ((LS1, 1, None), (GF, 3, None), (LS2, 2, _given(2, 7, 3).to(DEV))):
            ones, _ = _quant(x, scheme, k, 2.0, forced, fill=-1)
            zeros, _ = _quant(x, scheme, k, 2.0, forced, fill=0)
            assert torch.equal(ones, zeros)
            if L % 64:
                tail = ones[..., -1] >> (L % 64)        # (arithmetic shift: a set top bit would show as -1)
                print(f'{dt} L={L} scheme={scheme}: tail bits {tail.abs().max().item()}')
                assert (tail == 0).all()


@pytest.mark.parametrize('dt', DTYPES)
def test_unaligned_rows_give_the_same_bits(dt):
    """x at an odd element offset with odd L (2-byte loads) against the aligned copy; and, with L % 8 == 0, the 2-byte loads
    of a misaligned x against the 16-byte loads of the aligned one."""
    dtype = DTYPES[dt]
    alpha = _rounded(1.3, dtype)
    for n, L in ((7, 801), (3, 4105), (7, 800), (3, 4104), (2, 20000)):
        x = _rows(n, L, dtype, seed=70)
        assert x.data_ptr() % 16 == 0
        buf = torch.empty((n * L + 1,), dtype=dtype, device=DEV)
        buf[1:] = x.view(-1)
        xu = buf[1:].view(n, L)
        assert xu.data_ptr() % 16 == 2 and xu.is_contiguous()
        for scheme, k in ((LS1, 1), (GF, 3)):
            pa, sa = _quant(x, scheme, k, alpha)
            pu, su = _quant(xu, scheme, k, alpha)
            differ = (pa != pu).sum().item() + (sa.view(torch.int32) != su.view(torch.int32)).sum().item()
            print(f'{dt} N={n} L={L} scheme={scheme}: {differ} words differ between the aligned and the offset rows')
            assert differ == 0


def test_refused_calls_write_nothing():
    hip = _hip()
    n, L = 7, 800
    x = _rows(n, L, torch.bfloat16, seed=80)
    code = hip.LINEAR_HALF_DTYPES
    for scheme, k, xdt, forced in ((LS2, 2, code[torch.bfloat16], False), (LST, 2, code[torch.bfloat16], False),
                                   (LS1, 1, code[torch.float32], False), (GF, 3, code[torch.float32], True)):
        planes = torch.full((k * n * _nw(L),), SENTINEL_WORD, dtype=torch.int64, device=DEV)
        scales = torch.full((k, n), SENTINEL_SCALE, device=DEV)
        given = _given(k, n, 1).to(DEV) if forced else None
        rc = hip.linear_act_half_lib().lsq_linear_act_quant_half(x.data_ptr(), xdt, n, L, scheme, k, 2.0, hip.ptr(given),
                                                                 planes.data_ptr(), scales.data_ptr(), None)
        torch.cuda.synchronize()
        print(f'scheme={scheme} k={k} dtype={xdt}: code {rc}')
        assert rc == E_UNSUPPORTED
        assert (planes == SENTINEL_WORD).all() and (scales == SENTINEL_SCALE).all()
    with pytest.raises(ValueError):
        hip.linear_act_quant_half(x, LS2, 2, 2.0, torch.zeros((2 * n * _nw(L),), dtype=torch.int64, device=DEV),
                                  torch.zeros((2, n), device=DEV))


# ------------------------------------------------------------------------------------------------ QuantLinear
CLAMPS = ({'kind': 'identity'}, {'kind': 'symmetric', 'alpha': 2})
BOUND = 1e-5      # the fp32 kernels' own error against fp64, of max |y64| (tests/test_gpu_linear_half.py)


def _module(xq, ws, f, o, clamp, seed, bias=True, **kw):
    from quant.binary import QuantLinear
    m = QuantLinear(xq, ws, f, o, clamp, bias=bias, **kw)
    detgen.fill_module(m, seed=seed)
    with torch.no_grad():
        for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight.view(o, f, 1, 1), ws)):
            buf.copy_(v)
    return m


@pytest.fixture
def counters(monkeypatch):
    hip = _hip()
    names = {'half': 'linear_act_quant_half', 'act': 'act_quant', 'pack': 'pack_weight', 'xnor': 'linear_xnor'}
    calls = {name: 0 for name in names}
    real = {name: getattr(hip, attr) for name, attr in names.items()}

    def counted(name):
        def f(*a, **k):
            calls[name] += 1
            return real[name](*a, **k)
        return f

    for name, attr in names.items():
        monkeypatch.setattr(hip, attr, counted(name))
    calls['real'] = real
    return calls


def _bits(y):
    return y.contiguous().view(torch.int32 if y.dtype == torch.float32 else torch.int16)


def _set_average(m, seed):
    """A tracked moving average as training would leave it (decreasing scales)."""
    avg = m.x_approximate.moving_avg_module.moving_average
    with torch.no_grad():
        avg.copy_(torch.tensor([0.9 * 0.5 ** q + 0.01 * seed for q in range(avg.numel())]).view_as(avg))


@pytest.mark.parametrize('shape', [(9, 128), (4, 3, 128), (5, 100)])
@pytest.mark.parametrize('xq', ('ls-2', 'ls-T', 'gf-3', 'ls-1'))
@pytest.mark.parametrize('dt', DTYPES)
def test_given_scales_match_the_fp32_forward_bit_for_bit(dt, xq, shape, counters):
    """Moving average 'eval_only': the planes of x16 are those of x16.float() (the clamp bounds none / 2 are values of both
    types), so m(x16) is the fp32 forward's result rounded once -- on both routes."""
    i = ('ls-2', 'ls-T', 'gf-3', 'ls-1').index(xq)
    clamp = CLAMPS[(i + len(shape) + shape[0]) % 2]
    f, o = shape[-1], 70
    m = _module(xq, ('ls-1', 'ls-2', 'gf-3', 'ls-T')[i], f, o, clamp, seed=61 + i, bias=i % 2 == 0,
                moving_average_mode='eval_only').eval().to(DEV)
    _set_average(m, i)
    x = detgen.normal(f'qlinacthalf.x.{i}', shape, scale=1.3).to(DEV).to(DTYPES[dt])
    assert m._wants_hip(x)
    with torch.no_grad():
        y = m(x)
        assert (counters['half'], counters['act'], counters['xnor'], counters['pack']) == (1, 0, 1, 1)
        scales = m.last_act_scales.clone()
        y32 = m(x.float())
        assert (counters['half'], counters['act'], counters['pack']) == (1, 1, 1)     # one weight pack, shared
        m.act_half_kernel = False
        y_cast = m(x)
        assert (counters['half'], counters['act'], counters['pack']) == (1, 2, 1)
    assert y.dtype == x.dtype and y.shape == (*shape[:-1], o) and y32.dtype == torch.float32
    differ = (_bits(y) != _bits(y32.to(x.dtype))).sum().item()
    differ_cast = (_bits(y) != _bits(y_cast)).sum().item()
    print(f'{xq} {dt} {shape} {clamp["kind"]}: {differ} outputs differ from the fp32 forward rounded once, {differ_cast} from the '
          'cast route')
    assert differ == 0 and differ_cast == 0
    assert torch.equal(scales, m.last_act_scales) and scales.shape == (m.x_approximate.n_planes, shape[0])


@pytest.mark.parametrize('shape', [(9, 128), (4, 3, 128), (5, 100)])
@pytest.mark.parametrize('xq', ('ls-1', 'gf-3'))
@pytest.mark.parametrize('dt', DTYPES)
def test_free_running_forward(dt, xq, shape, counters):
    """m(x16) is lsq_linear_xnor on lsq_act_quant(x16.float(), forced = m.last_act_scales) cast once, and within the resolution
    of a once-rounded 16-bit output, (2^-8 | 2^-11) + 1e-5 of max |y64|, of the fp64 oracle with those scales."""
    hip = _hip()
    i = ('ls-1', 'gf-3').index(xq)
    clamp = {'kind': 'symmetric', 'alpha': (2, 1.3)[(i + len(shape)) % 2]}
    ws = ('ls-2', 'ls-1')[i]
    f, o = shape[-1], 70
    m = _module(xq, ws, f, o, clamp, seed=71 + i).eval().to(DEV)
    x = detgen.normal(f'qlinacthalf.free.{i}', shape, scale=1.3).to(DEV).to(DTYPES[dt])
    with torch.no_grad():
        y = m(x)
        with torch.autocast('cuda', dtype=x.dtype):
            ya = m(x)
    assert (counters['half'], counters['act'], counters['xnor'], counters['pack']) == (2, 0, 2, 1)
    assert ya.dtype == x.dtype and torch.equal(_bits(ya), _bits(y))
    scales = m.last_act_scales.clone()
    n, t, k = shape[0], x.numel() // (shape[0] * f), m.x_approximate.n_planes
    alpha = _rounded(clamp['alpha'], x.dtype)
    geom = hip.make_geom(n, t * f, 1, 1, o, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    planes = torch.zeros((k * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    out = torch.empty((k, n), device=DEV)
    counters['real']['act'](x.reshape(n, t * f).float(), geom, m.x_approximate.hip_scheme, k, 3, alpha, planes, out, scales)
    wbits, wsum, wscales = m._packed_weights(hip)
    ref = counters['real']['xnor'](planes, k, scales, t, wbits, wsum, wscales, m.bias.detach(), n * t, f, o).to(x.dtype)
    differ = (_bits(y) != _bits(ref.view(*shape[:-1], o))).sum().item()
    # the fp64 oracle: the reference's quantizers on the clamped 16-bit rows with the kernel's scales
    xc = x.cpu().float().clamp(-alpha, alpha).reshape(n, t * f, 1, 1)
    vs = [scales[q].cpu() for q in range(k)]
    xq64 = P.quantize_activation(xc.double(), xq, scales=[v.double() for v in vs])[1].reshape(n * t, f)
    wq = P.quantize_weight(m.weight.detach().cpu().view(o, f, 1, 1), ws, [b.cpu() for b in m.w_approximate.cached_scales()])
    y64 = F.linear(xq64, wq.view(o, f).double(), m.bias.detach().cpu().double()).view(*shape[:-1], o)
    err = ((y.cpu().double() - y64).abs().max() / y64.abs().max()).item()
    bound = (2.0 ** -8 if x.dtype == torch.bfloat16 else 2.0 ** -11) + BOUND
    print(f'{xq} {dt} {shape} alpha={alpha}: {differ} outputs differ from the kernels on x.float(); max err / max|y64| = {err:.3e} '
          f'(bound {bound:.3e})')
    assert differ == 0
    assert err <= bound


@pytest.mark.parametrize('dt', DTYPES)
def test_strided_inputs_are_copied_first(dt, counters):
    f, o = 128, 40
    m = _module('gf-3', 'ls-1', f, o, CLAMPS[1], seed=81).eval().to(DEV)
    h = detgen.normal('qlinacthalf.stride.h', (6, 5, f), scale=1.3).to(DEV).to(DTYPES[dt])
    wide = detgen.normal('qlinacthalf.stride.w', (4, 3, f + 7), scale=1.3).to(DEV).to(DTYPES[dt])
    for x in (h[:, 0], wide[..., :f], wide[..., 7:]):
        assert not x.is_contiguous()
        before = counters['half']
        with torch.no_grad():
            y = m(x)
            yc = m(x.contiguous())
        assert counters['half'] - before == 2 and counters['act'] == 0
        assert y.shape == (*x.shape[:-1], o) and y.dtype == x.dtype
        assert torch.equal(_bits(y), _bits(yc))


def test_sixteen_bit_binary_activation_paths_that_stay_on_torch(counters):
    """Train mode, an input that wants a gradient, 16-bit weights, free-running ls-2, an autocast of the other type: the torch
    formulation, neither quantizer kernel."""
    x = detgen.normal('qlinacthalf.torch.x', (5, 128), scale=1.2).to(DEV)
    bf, fp = torch.bfloat16, torch.float16
    cases = [
        (_module('ls-1', 'ls-1', 128, 20, CLAMPS[1], seed=91).to(DEV).train(), x.to(bf), bf, False),
        (_module('gf-3', 'ls-1', 128, 20, CLAMPS[1], seed=92).eval().to(DEV), x.to(bf).requires_grad_(True), bf, True),
        (_module('ls-1', 'ls-1', 128, 20, CLAMPS[1], seed=93).eval().to(DEV).bfloat16(), x.to(bf), None, False),
        (_module('ls-2', 'ls-1', 128, 20, CLAMPS[1], seed=94).eval().to(DEV), x.to(bf), bf, False),
        (_module('ls-1', 'ls-1', 128, 20, CLAMPS[1], seed=95).eval().to(DEV), x.to(fp), bf, False),
    ]
    for mod, xin, autocast, grad in cases:
        with torch.set_grad_enabled(grad), torch.autocast('cuda', dtype=autocast or bf, enabled=autocast is not None):
            assert not mod._wants_hip(xin)
            y = mod(xin)
            ref = mod._forward_torch(xin)
        assert torch.equal(y, ref)
    print(f'calls: lsq_linear_act_quant_half {counters["half"]}, lsq_act_quant {counters["act"]}')
    assert (counters['half'], counters['act']) == (0, 0)
