"""lsq_act_quant_half (liblsq_hip_conv_act_half.so) and QuantConv2d with ``act_half`` on bf16 / fp16 inputs on the GPU: the
planes against a CPU fp32 restatement of the chain packed into the convolution's layout and against lsq_act_quant on
x.float(); the scales against the fp64 mean of the fp32 magnitudes; the free-running v1 against lsq_act_quant,
lsq_linear_act_quant_solve_half and the exact oracle; halo and guard words; invariance to the batch, determinism, alignment;
zeros, -0.0, subnormals; refused calls; the module's dispatch, both routes, the counters and the paths that stay on torch.

Every test prints the figure it asserts on (pytest -s shows them)."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_act_half_cases as C
import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = C.DTYPES
LS1, LS2, LST, GF = 1, 2, 3, 4
E_NULL, E_SHAPE, E_SCHEME, E_UNSUPPORTED = -1, -2, -3, -6
# |v - v64| <= SCALE_BOUND * v64 against the fp64 mean of the fp32 magnitudes: derived, not measured -- the fp32 sum of 8
# non-negative terms carries at most 7 roundings of 2^-24, the final conversion to fp32 one more
SCALE_BOUND = 2.0 ** -21
GUARD = 5                         # words / floats / ints around planes, scales and status
SENTINEL_WORD, SENTINEL_SCALE, SENTINEL_STATUS = 0x5A5A5A5A5A5A5A5A, 12345.0, -77


def _hip():
    from quant import _hip
    return _hip


def _geom(gi, n):
    c, h, w, groups, pad = C.GEOMS[gi]
    return _hip().make_geom(n, c, h, w, C.OUT_CHANNELS, C.KERNEL, C.KERNEL, (1, 1), pad, (1, 1), groups)


def _prepared(gi, n, k, fill):
    """(buffer, planes view of k * words inside GUARD words): halo and guards hold the sentinel, the interior `fill`."""
    c, h, w, groups, (ph, pw) = C.GEOMS[gi]
    gt, hp, wp = C.plane_shape(gi, n)
    body = torch.full((k, n, gt, hp, wp), SENTINEL_WORD, dtype=torch.int64)
    body[..., ph:ph + h, pw:pw + w] = fill
    guard = torch.full((GUARD,), SENTINEL_WORD, dtype=torch.int64)
    buf = torch.cat([guard, body.view(-1), guard]).to(DEV)
    return buf, buf[GUARD:GUARD + body.numel()]


def _halo_intact(gi, planes):
    """planes [k, N, Gt, Hp, Wp] on the CPU: every halo word still holds the sentinel."""
    c, h, w, groups, (ph, pw) = C.GEOMS[gi]
    halo = torch.ones(planes.shape[-2:], dtype=torch.bool)
    halo[ph:ph + h, pw:pw + w] = False
    return bool((planes[..., halo] == SENTINEL_WORD).all())


def _interior(gi, planes):
    c, h, w, groups, (ph, pw) = C.GEOMS[gi]
    return planes[..., ph:ph + h, pw:pw + w]


def _quant(x, gi, scheme, k, alpha, skip=3, forced=None, fill=0):
    """The kernel on x [N, C, H, W] (on the GPU) with `alpha` already a value of x's type.  The planes' interior is pre-filled
    with `fill`, their halo with a sentinel; planes, scales and status lie inside guard words; halo and guards must come back
    untouched.  Returns (planes [k, N, Gt, Hp, Wp] int64, scales [k, N], status [N]) on the CPU."""
    hip = _hip()
    n = x.shape[0]
    pbuf, planes = _prepared(gi, n, k, fill)
    sbuf = torch.full((GUARD + k * n + GUARD,), SENTINEL_SCALE, device=DEV)
    tbuf = torch.full((GUARD + n + GUARD,), SENTINEL_STATUS, dtype=torch.int32, device=DEV)
    scales, status = sbuf[GUARD:GUARD + k * n].view(k, n), tbuf[GUARD:GUARD + n]
    hip.act_quant_half(x, _geom(gi, n), scheme, k, skip, alpha, planes, scales, forced, status)
    torch.cuda.synchronize()
    assert (pbuf[:GUARD] == SENTINEL_WORD).all() and (pbuf[GUARD + planes.numel():] == SENTINEL_WORD).all()
    assert (sbuf[:GUARD] == SENTINEL_SCALE).all() and (sbuf[GUARD + k * n:] == SENTINEL_SCALE).all()
    assert (tbuf[:GUARD] == SENTINEL_STATUS).all() and (tbuf[GUARD + n:] == SENTINEL_STATUS).all()
    out = planes.view(k, n, *C.plane_shape(gi, n)).cpu()
    assert _halo_intact(gi, out)
    return out, scales.cpu().clone(), status.cpu().clone()


def _act_quant_reference(x, gi, scheme, k, alpha, skip, forced, fill):
    """lsq_act_quant on x.float() into a buffer prepared the same way: (planes [k, N, Gt, Hp, Wp], scales [k, N]) on the CPU."""
    hip = _hip()
    n = x.shape[0]
    _, planes = _prepared(gi, n, k, fill)
    scales = torch.empty((k, n), device=DEV)
    hip.act_quant(x.float(), _geom(gi, n), scheme, k, skip, alpha, planes, scales, None if forced is None else forced.to(DEV).contiguous())
    torch.cuda.synchronize()
    return planes.view(k, n, *C.plane_shape(gi, n)).cpu(), scales.cpu()


def _check_scales(scales, mags, what):
    """Each v_q against the fp64 mean of the fp32 magnitudes built from the kernel's own earlier scales."""
    v64 = mags.double().flatten(2).mean(dim=2)
    rel = ((scales.double() - v64).abs() / v64.clamp_min(1e-300)).max().item()
    print(f'{what}: max |v - v64| / v64 = {rel / SCALE_BOUND:.3f} of the bound {SCALE_BOUND:.3e}')
    assert ((scales.double() - v64).abs() <= SCALE_BOUND * v64).all(), (what, rel)


def _expected_words(x, gi, alpha, scales):
    """(words [k, N, Gt, Hp, Wp] int64 with a zero halo, |res_q|) of the CPU chain + packer on x (CPU, 16-bit)."""
    groups, pad = C.GEOMS[gi][3:]
    bits, mags = C.chain(x.float(), alpha, scales)
    return torch.from_numpy(C.pack(bits.numpy(), groups, pad).view(np.int64)), mags


def _given(k, n, seed):
    """Per-sample scales of a decreasing chain."""
    base = detgen.uniform(f'convacthalf.v.{seed}', (1, n), 0.5, 1.1, seed=seed)
    return torch.cat([base * 0.55 ** q for q in range(k)]).contiguous()


# (name, LSQ_SCHEME_*, k, scales given)
CASES = [('ls-1', LS1, 1, False), ('gf-1', GF, 1, False), ('gf-3', GF, 3, False), ('gf-8', GF, 8, False),
         ('ls-2 given', LS2, 2, True), ('ls-T given', LST, 2, True), ('gf-3 given', GF, 3, True),
         ('ls-2 free', LS2, 2, False), ('ls-T free', LST, 2, False)]


@pytest.mark.parametrize('ci', range(len(CASES)))
@pytest.mark.parametrize('gi', range(len(C.GEOMS)))
@pytest.mark.parametrize('dt', DTYPES)
def test_planes_and_scales(dt, gi, ci):
    """Every geometry x scheme x type, the clamp bounds and skips in rotation, the interior pre-filled with zeros and with
    ones: halo and guards untouched; interior words equal the CPU chain + packer with the kernel's own scales; the whole
    buffer equals lsq_act_quant's on x.float() with those scales; given scales copied; computed scales within the derived
    bound of the fp64 mean; the free-running v1 equals lsq_act_quant's, lsq_linear_act_quant_solve_half's and the oracle's."""
    hip = _hip()
    name, scheme, k, given = CASES[ci]
    dtype, di = DTYPES[dt], list(DTYPES).index(dt)
    free_solve = scheme in (LS2, LST) and not given
    n = C.batch_size(gi)
    alpha = C.rounded(C.BOUNDS[(gi + ci + di) % 4], dtype)
    skip = C.SKIPS[(gi + ci // 2 + di) % 2]
    x16 = C.batch(gi, dt)
    x = x16.to(DEV)
    forced = None
    if given:
        forced = _given(k, n, seed=ci)
        if scheme == LST:
            forced = forced[[0, 0]].contiguous()
    what = f'{name} {dt} geometry {gi + 1} N={n} alpha={alpha} skip={skip}'
    planes, scales, status = _quant(x, gi, scheme, k, alpha, skip, None if forced is None else forced.to(DEV), fill=0)
    ones, scales1, status1 = _quant(x, gi, scheme, k, alpha, skip, None if forced is None else forced.to(DEV), fill=-1)
    assert torch.equal(planes, ones) and torch.equal(scales.view(torch.int32), scales1.view(torch.int32))
    assert torch.equal(status, status1)
    want, mags = _expected_words(x16, gi, alpha, scales)
    wrong = (_interior(gi, planes) != _interior(gi, want)).sum().item()
    ref, _ = _act_quant_reference(x, gi, scheme, k, alpha, skip, scales, fill=0)
    wrong_ref = (planes != ref).sum().item()
    print(f'{what}: {wrong} interior words differ from the CPU chain, {wrong_ref} words of the buffer from lsq_act_quant')
    assert wrong == 0 and wrong_ref == 0
    if given:
        assert torch.equal(scales.view(torch.int32), forced.view(torch.int32))
        assert (status == 1).all()
    elif not free_solve:
        _check_scales(scales, mags, what)
        assert (status == 1).all()
    else:
        ternary = scheme == LST
        m = x16[0].numel()
        v1 = scales[0].view(torch.int32)
        free, free_scales = _act_quant_reference(x, gi, scheme, 2, alpha, skip, None, fill=0)
        lin_planes = torch.zeros((2 * n * ((m + 63) // 64),), dtype=torch.int64, device=DEV)
        lin_scales = torch.empty((2, n), device=DEV)
        hip.linear_act_quant_solve_half(x.view(n, m), scheme, skip, alpha, lin_planes, lin_scales)
        xc = C.clamped32(x16.view(n, m), alpha)
        oracle, found = C.oracle_rows(xc, ternary, skip)
        differ = [(v1 != free_scales[0].view(torch.int32)).sum().item(),
                  (v1 != lin_scales[0].cpu().view(torch.int32)).sum().item(),
                  (v1 != torch.from_numpy(oracle).view(torch.int32)).sum().item()]
        wrong_free = (planes != free).sum().item()
        # status: the oracle's found, except that a sub-sample of zeros only is reported as a row without a candidate
        found = found & (np.abs(xc[:, ::skip]).max(axis=1) > 0)
        wrong_status = (status.bool() != torch.from_numpy(found)).sum().item()
        print(f'{what}: v1 differs in {differ} rows from lsq_act_quant / lsq_linear_act_quant_solve_half / the oracle; '
              f'{wrong_free} words differ from lsq_act_quant free-running; {wrong_status} status words wrong')
        assert differ == [0, 0, 0] and wrong_free == 0 and wrong_status == 0
        if ternary:
            assert torch.equal(scales[1].view(torch.int32), v1)
        else:
            _check_scales(scales[1:], mags[1:], what + ' v2')


BATCH_SCHEMES = (('ls-1', LS1, 1), ('gf-3', GF, 3), ('ls-2 free', LS2, 2), ('ls-T free', LST, 2))


@pytest.mark.parametrize('gi', (3, 7, 9))
@pytest.mark.parametrize('dt', DTYPES)
def test_a_samples_result_does_not_depend_on_the_batch(dt, gi):
    """Geometries 4, 8 and 10: the same sample alone and as sample 0, 2 and 4 of a batch of 5 gives the same scale bits and
    words; two runs give the same bits."""
    dtype = DTYPES[dt]
    batch = C.batch(gi, dt, 5).clone()
    sample = batch[1].clone()
    for r in (0, 2, 4):
        batch[r] = sample
    alpha = C.rounded(1.3, dtype)
    for name, scheme, k in BATCH_SCHEMES:
        p1, s1, t1 = _quant(sample[None].to(DEV), gi, scheme, k, alpha)
        pb, sb, tb = _quant(batch.to(DEV), gi, scheme, k, alpha)
        pb2, sb2, tb2 = _quant(batch.to(DEV), gi, scheme, k, alpha)
        differ = sum((sb[:, r].view(torch.int32) != s1[:, 0].view(torch.int32)).sum().item() + (pb[:, r] != p1[:, 0]).sum().item()
                     + int(tb[r] != t1[0]) for r in (0, 1, 2, 4))
        print(f'{name} {dt} geometry {gi + 1}: {differ} scale / plane / status words differ between the sample alone and in the batch')
        assert differ == 0
        assert torch.equal(pb, pb2) and torch.equal(sb.view(torch.int32), sb2.view(torch.int32)) and torch.equal(tb, tb2)


@pytest.mark.parametrize('gi', (2, 3, 7))
@pytest.mark.parametrize('dt', DTYPES)
def test_unaligned_inputs_give_the_same_bits(dt, gi):
    """Geometries 3, 4 and 8: x at an odd element offset (2-byte loads), and at an offset of 4 elements (8-byte alignment:
    geometry 4 leaves its 16-byte loads), against the aligned copy."""
    dtype = DTYPES[dt]
    alpha = C.rounded(1.3, dtype)
    x = C.batch(gi, dt).to(DEV)
    assert x.data_ptr() % 16 == 0
    for off in (1, 4):
        buf = torch.empty((x.numel() + off,), dtype=dtype, device=DEV)
        buf[off:] = x.view(-1)
        xu = buf[off:].view(x.shape)
        assert xu.data_ptr() % 16 == 2 * off and xu.is_contiguous()
        for name, scheme, k in BATCH_SCHEMES + (('ls-2 given', LS2, 2),):
            forced = _given(2, x.shape[0], 3).to(DEV) if name.endswith('given') else None
            pa, sa, ta = _quant(x, gi, scheme, k, alpha, 3, forced)
            pu, su, tu = _quant(xu, gi, scheme, k, alpha, 3, forced)
            differ = (pa != pu).sum().item() + (sa.view(torch.int32) != su.view(torch.int32)).sum().item() + (ta != tu).sum().item()
            print(f'{name} {dt} geometry {gi + 1} offset {off}: {differ} words differ between the aligned and the offset input')
            assert differ == 0


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize('gi', (4, 5))
@pytest.mark.parametrize('dt', DTYPES)
def test_zero_samples_and_negative_zero(dt, gi):
    """An all-zero sample and a sample of -0.0 (geometries 5 and 6: channels past C / groups in the last word): scale +0,
    every real channel's bit 1, the padding channels' bits 0, solve status 0."""
    c, h, w, groups, pad = C.GEOMS[gi]
    x = torch.zeros((2, c, h, w), dtype=DTYPES[dt])
    x[1] = -0.0
    assert (x[1].view(torch.int16) == -32768).all()
    want = torch.from_numpy(C.pack(np.ones((1, 2, c, h, w), dtype=bool), groups, pad).view(np.int64))
    for name, scheme, k in BATCH_SCHEMES:
        for fill in (0, -1):
            planes, scales, status = _quant(x.to(DEV), gi, scheme, k, 2.0, 3, None, fill)
            print(f'{name} {dt} geometry {gi + 1} fill={fill}: scales {scales.flatten().tolist()}, status {status.tolist()}, '
                  f'last word {planes[0, 1, -1, pad[0], pad[1]].item():#x}')
            assert (scales == 0).all() and not torch.signbit(scales).any()
            assert all(torch.equal(_interior(gi, planes[q:q + 1]), _interior(gi, want)) for q in range(k))
            assert (status == (0 if scheme in (LS2, LST) else 1)).all()


@pytest.mark.parametrize('gi', (2, 8))
@pytest.mark.parametrize('dt', DTYPES)
def test_constant_and_fully_clamped_samples(dt, gi):
    """The table solve where one key holds a whole sample (geometry 3: 2-byte loads, M = 3087; geometry 9: 16-byte loads,
    M = 2048), ls-2 / ls-T free-running, skip 1 and 3.  Samples of 0.75 without a clamp: every candidate lies in one slice,
    ls-2 finds v1 = c inside the run and ls-T its extra candidate c / 2.  Samples with |x| >= 2 under the bound 0.5: every
    element is counted on key(alpha), both signs.  v1 bit for bit and status against lsq_exact and against
    lsq_linear_act_quant_solve_half on the flat rows; the interior words against the CPU chain."""
    hip = _hip()
    c, h, w = C.GEOMS[gi][:3]
    m = c * h * w
    dtype = DTYPES[dt]
    big = detgen.normal(f'convacthalf.big.{gi}', (2, c, h, w), seed=gi, scale=1.0)
    big = (big + torch.where(big >= 0, 2.0, -2.0)).to(dtype)
    assert (big.float().abs() >= 2).all()
    for what, x16, alpha in (('constant', torch.full((2, c, h, w), 0.75, dtype=dtype), -1.0), ('clamped', big, 0.5)):
        for name, scheme in (('ls-2', LS2), ('ls-T', LST)):
            for skip in C.SKIPS:
                planes, scales, status = _quant(x16.to(DEV), gi, scheme, 2, alpha, skip)
                want_v1, found = C.oracle_rows(C.clamped32(x16.view(2, m), alpha), scheme == LST, skip)
                lin_planes = torch.zeros((2 * 2 * ((m + 63) // 64),), dtype=torch.int64, device=DEV)
                lin_scales = torch.empty((2, 2), device=DEV)
                hip.linear_act_quant_solve_half(x16.to(DEV).view(2, m), scheme, skip, alpha, lin_planes, lin_scales)
                words, _ = _expected_words(x16, gi, alpha, scales)
                print(f'{what} {name} {dt} geometry {gi + 1} skip={skip}: v1 {scales[0].tolist()} oracle {want_v1.tolist()} '
                      f'linear {lin_scales[0].tolist()} status {status.tolist()} found {found.tolist()}')
                assert torch.equal(scales[0].view(torch.int32), torch.from_numpy(want_v1).view(torch.int32))
                assert torch.equal(scales[0].view(torch.int32), lin_scales[0].cpu().view(torch.int32))
                assert torch.equal(status.bool(), torch.from_numpy(found))
                assert torch.equal(_interior(gi, planes), _interior(gi, words))
                if what == 'constant':
                    assert (scales[0] == (0.375 if scheme == LST else 0.75)).all()


@pytest.mark.parametrize('dt', DTYPES)
def test_negative_subnormals(dt):
    """64 negative subnormals -k * (smallest subnormal), k = 1 .. 64, as a sample (64, 1, 1): every bit 0 (a flushed value
    would be -0.0: bit 1), the scale within the bound of their fp64 mean (a flushed sample would give 0)."""
    hip = _hip()
    dtype = DTYPES[dt]
    tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133
    x = (-torch.arange(1, 65, dtype=torch.float64) * tiny).to(dtype).view(1, 64, 1, 1)
    assert torch.equal(x.double().flatten(), -torch.arange(1, 65, dtype=torch.float64) * tiny)
    assert (x.float().abs() < torch.finfo(dtype).tiny).all()
    geom = hip.make_geom(1, 64, 1, 1, 64, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    v64 = 32.5 * tiny
    for xin, scheme, k, alpha, word in ((x, LS1, 1, -1.0, 0), (-x, GF, 2, 2.0, -1)):
        planes = torch.full((k,), SENTINEL_WORD, dtype=torch.int64, device=DEV)
        scales = torch.empty((k, 1), device=DEV)
        hip.act_quant_half(xin.to(DEV), geom, scheme, k, 3, alpha, planes, scales)
        print(f'{dt} subnormals: plane word {planes[0].item():#x}, scale {scales[0].item()!r}, fp64 mean {v64!r}')
        assert planes[0].item() == word
        assert abs(scales[0].item() - v64) <= SCALE_BOUND * v64


def test_refused_calls_write_nothing():
    hip = _hip()
    gi, n = 2, 3
    x = C.batch(gi, 'bf16').to(DEV)
    code = hip.LINEAR_HALF_DTYPES
    fn = hip.conv_act_half_lib().lsq_act_quant_half
    bad_groups = hip.make_geom(n, 63, 7, 7, 64, 3, 3, (1, 1), (1, 1), (1, 1), 2)
    good = _geom(gi, n)
    # (geometry, dtype code, scheme, k, skip, scales given, expected)
    refusals = ((good, code[torch.float32], LS1, 1, 3, False, E_UNSUPPORTED), (good, code[torch.float32], GF, 3, 3, True, E_UNSUPPORTED),
                (good, code[torch.bfloat16], LS2, 1, 3, False, E_SCHEME), (good, code[torch.bfloat16], GF, 9, 3, False, E_SCHEME),
                (good, code[torch.bfloat16], LS1, 2, 3, True, E_SCHEME), (good, code[torch.bfloat16], LST, 2, 0, False, E_SHAPE),
                (bad_groups, code[torch.bfloat16], LS1, 1, 3, False, E_SHAPE), (None, code[torch.bfloat16], LS1, 1, 3, False, E_NULL))
    for geom, xdt, scheme, k, skip, given, expected in refusals:
        kk = min(max(k, 1), 8)
        pbuf, planes = _prepared(gi, n, kk, SENTINEL_WORD)
        scales = torch.full((kk, n), SENTINEL_SCALE, device=DEV)
        status = torch.full((n,), SENTINEL_STATUS, dtype=torch.int32, device=DEV)
        forced = _given(kk, n, 1).to(DEV) if given else None
        rc = fn(x.data_ptr(), xdt, None if geom is None else ctypes.byref(geom), scheme, k, skip, 2.0, hip.ptr(forced),
                planes.data_ptr(), scales.data_ptr(), status.data_ptr(), None)
        torch.cuda.synchronize()
        print(f'scheme={scheme} k={k} skip={skip} dtype={xdt}: code {rc}')
        assert rc == expected
        assert (pbuf == SENTINEL_WORD).all() and (scales == SENTINEL_SCALE).all() and (status == SENTINEL_STATUS).all()
    with pytest.raises(TypeError):
        hip.act_quant_half(x.float(), good, LS1, 1, 3, 2.0, torch.zeros((hip.act_plane_words(good),), dtype=torch.int64, device=DEV),
                           torch.zeros((1, n), device=DEV))


# ------------------------------------------------------------------------------------------------ QuantConv2d
CLAMPS = ({'kind': 'identity'}, {'kind': 'symmetric', 'alpha': 2})
BOUND = 1e-4      # the project's convolution bound: the fp32 kernels' own error against fp64, of max |y64|
XQS = ('ls-2', 'ls-T', 'gf-3', 'ls-1')
# (in channels, out channels, kernel, padding, stride, H = W, N)
LAYERS = ((64, 70, 3, 1, 1, 9, 5), (64, 70, 3, 1, 2, 9, 5), (65, 40, 1, 0, 1, 7, 5))


def _module(xq, ws, cin, cout, ksz, clamp, seed, bias=True, **kw):
    from quant.binary.binary_conv import QuantConv2d
    m = QuantConv2d(xq, ws, cin, cout, ksz, clamp, bias=bias, **kw)
    detgen.fill_module(m, seed=seed)
    with torch.no_grad():
        for buf, v in zip(m.w_approximate.cached_scales(), P.weight_scales(m.weight, ws)):
            buf.copy_(v)
    return m


@pytest.fixture
def counters(monkeypatch):
    hip = _hip()
    names = {'half': 'act_quant_half', 'act': 'act_quant', 'pack': 'pack_weight', 'xnor': 'xnor_conv2d'}
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


def _input(name, layer, dtype):
    cin, _, _, _, _, hw, n = layer
    return detgen.normal(name, (n, cin, hw, hw), scale=1.3).to(DEV).to(dtype)


@pytest.mark.parametrize('dt', DTYPES)
def test_default_module_stays_on_torch(dt, counters):
    m = _module('ls-1', 'ls-1', 64, 70, 3, CLAMPS[1], seed=51, padding=1).eval().to(DEV)
    x = _input('qconvacthalf.default', LAYERS[0], DTYPES[dt])
    with torch.no_grad(), torch.autocast('cuda', dtype=x.dtype):      # (fp32 weights: torch itself needs the autocast)
        assert not m._wants_hip(x)
        y, ref = m(x), m._forward_torch(x)
    print(f'default {dt}: lsq_act_quant_half {counters["half"]} calls, lsq_act_quant {counters["act"]} calls')
    assert torch.equal(y, ref) and y.dtype == x.dtype
    assert (counters['half'], counters['act']) == (0, 0)


@pytest.mark.parametrize('li', range(len(LAYERS)))
@pytest.mark.parametrize('xq', XQS)
@pytest.mark.parametrize('dt', DTYPES)
def test_given_scales_match_the_fp32_forward_bit_for_bit(dt, xq, li, counters):
    """Moving average 'eval_only', scales set by hand: the planes of x16 are those of x16.float() (the clamp bounds none / 2
    are values of both types), so m(x16) is the fp32 forward's result rounded once -- on both routes; one weight pack."""
    i = XQS.index(xq)
    layer = LAYERS[li]
    cin, cout, ksz, pad, stride = layer[:5]
    clamp = CLAMPS[(i + li) % 2]
    m = _module(xq, ('ls-1', 'ls-2', 'gf-3', 'ls-T')[i], cin, cout, ksz, clamp, seed=61 + i, bias=i % 2 == 0, padding=pad,
                stride=stride, moving_average_mode='eval_only').eval().to(DEV)
    m.act_half = True
    _set_average(m, i)
    x = _input(f'qconvacthalf.x.{i}', layer, DTYPES[dt])
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
    assert y.dtype == x.dtype and y.shape == y32.shape and y32.dtype == torch.float32
    differ = (_bits(y) != _bits(y32.to(x.dtype))).sum().item()
    differ_cast = (_bits(y) != _bits(y_cast)).sum().item()
    print(f'{xq} {dt} layer {layer} {clamp["kind"]}: {differ} outputs differ from the fp32 forward rounded once, {differ_cast} from '
          'the cast route')
    assert differ == 0 and differ_cast == 0
    assert torch.equal(scales, m.last_act_scales) and scales.shape == (m.x_approximate.n_planes, x.shape[0])


@pytest.mark.parametrize('li', range(len(LAYERS)))
@pytest.mark.parametrize('xq', ('ls-1', 'gf-3', 'ls-2'))
@pytest.mark.parametrize('dt', DTYPES)
def test_free_running_forward(dt, xq, li, counters):
    """Clamp 1.3: m(x16) is lsq_xnor_conv2d on lsq_act_quant(x16.float(), forced = m.last_act_scales) rounded once, the same
    bits under an autocast of the type, and within one rounding of the output type, (2^-8 | 2^-11) + 1e-4 of max |y64|, of
    the fp64 oracle with those scales."""
    hip = _hip()
    i = ('ls-1', 'gf-3', 'ls-2').index(xq)
    layer = LAYERS[li]
    cin, cout, ksz, pad, stride, hw, n = layer
    clamp = {'kind': 'symmetric', 'alpha': 1.3}
    ws = ('ls-2', 'ls-1', 'ls-T')[i]
    m = _module(xq, ws, cin, cout, ksz, clamp, seed=71 + i, padding=pad, stride=stride).eval().to(DEV)
    m.act_half = True
    x = _input(f'qconvacthalf.free.{i}', layer, DTYPES[dt])
    with torch.no_grad():
        y = m(x)
        with torch.autocast('cuda', dtype=x.dtype):
            ya = m(x)
    assert (counters['half'], counters['act'], counters['xnor'], counters['pack']) == (2, 0, 2, 1)
    assert ya.dtype == x.dtype and torch.equal(_bits(ya), _bits(y))
    scales = m.last_act_scales.clone()
    k = m.x_approximate.n_planes
    alpha = C.rounded(1.3, x.dtype)
    geom = hip.make_geom(n, cin, hw, hw, cout, ksz, ksz, (stride, stride), (pad, pad), (1, 1), 1)
    planes = torch.zeros((k * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    out = torch.empty((k, n), device=DEV)
    counters['real']['act'](x.float(), geom, m.x_approximate.hip_scheme, k, 3, alpha, planes, out, scales)
    wbits, wsum, wscales, _ = m._packed_weights(geom, hip)
    ho, wo = hip.out_hw(geom)
    ref = torch.empty((n, cout, ho, wo), device=DEV)
    counters['real']['xnor'](planes, k, scales, wbits, wsum, wscales, m.bias.detach(), geom, ref)
    differ = (_bits(y) != _bits(ref.to(x.dtype))).sum().item()
    # the fp64 oracle: the reference's quantizers on the clamped 16-bit samples with the kernel's scales
    xc = x.cpu().float().clamp(-alpha, alpha)
    vs = [scales[q].cpu() for q in range(k)]
    xq64 = P.quantize_activation(xc.double(), xq, scales=[v.double() for v in vs])[1]
    wq = P.quantize_weight(m.weight.detach().cpu(), ws, [b.cpu() for b in m.w_approximate.cached_scales()])
    y64 = F.conv2d(xq64, wq.double(), m.bias.detach().cpu().double(), stride, pad)
    err = ((y.cpu().double() - y64).abs().max() / y64.abs().max()).item()
    bound = (2.0 ** -8 if x.dtype == torch.bfloat16 else 2.0 ** -11) + BOUND
    print(f'{xq} {dt} layer {layer} alpha={alpha}: {differ} outputs differ from the kernels on x.float(); max err / max|y64| = '
          f'{err:.3e} (bound {bound:.3e})')
    assert differ == 0
    assert err <= bound


@pytest.mark.parametrize('dt', DTYPES)
def test_fused_forward_composes_on_a_sixteen_bit_input(dt, counters):
    """fused_forward with a batch norm in front, ReLU and a residual: the composition of the modules, the convolution inside
    it on the kernels -- lsq_act_quant_half once, no folded batch norm."""
    layer = LAYERS[0]
    dtype = DTYPES[dt]
    m = _module('ls-1', 'ls-1', 64, 70, 3, CLAMPS[1], seed=81, padding=1).eval().to(DEV)
    m.act_half = True
    bn = torch.nn.BatchNorm2d(64).eval().to(DEV)
    with torch.no_grad():
        bn.running_mean.copy_(detgen.normal('qconvacthalf.bn.m', (64,), scale=0.1))
        bn.running_var.copy_(detgen.uniform('qconvacthalf.bn.v', (64,), 0.5, 1.5))
    x = _input('qconvacthalf.fused', layer, dtype)
    res = detgen.normal('qconvacthalf.res', (5, 70, 9, 9), scale=1.0).to(DEV).to(dtype)
    with torch.no_grad():
        y = m.fused_forward(x, pre_bn=bn, relu=True, res_pre=res)
        assert (counters['half'], counters['act'], counters['xnor']) == (1, 0, 1)
        ref = torch.relu(m(bn(x)) + res)
    print(f'fused_forward {dt}: {(_bits(y) != _bits(ref)).sum().item()} outputs differ from the composition')
    assert y.dtype == dtype and torch.equal(_bits(y), _bits(ref))
    assert (counters['half'], counters['act']) == (2, 0)


@pytest.mark.parametrize('dt', DTYPES)
def test_channels_last_inputs_are_copied_first(dt, counters):
    m = _module('gf-3', 'ls-1', 64, 70, 3, CLAMPS[1], seed=82, padding=1).eval().to(DEV)
    m.act_half = True
    x = _input('qconvacthalf.cl', LAYERS[0], DTYPES[dt])
    xl = x.to(memory_format=torch.channels_last)
    assert not xl.is_contiguous()
    with torch.no_grad():
        y, yl = m(x), m(xl)
    print(f'channels-last {dt}: {(_bits(y) != _bits(yl)).sum().item()} outputs differ from the contiguous copy')
    assert counters['half'] == 2 and counters['act'] == 0
    assert torch.equal(_bits(y), _bits(yl))


def test_sixteen_bit_paths_that_stay_on_torch(counters):
    """Train mode, an input that wants a gradient, 16-bit weights, an autocast of the other type, fp activations, free-running
    ls-2 with act_half_solve off: the torch formulation, neither quantizer kernel -- with act_half set."""
    x = detgen.normal('qconvacthalf.torch.x', (3, 64, 6, 6), scale=1.2).to(DEV)
    bf, fp = torch.bfloat16, torch.float16

    def mod(xq, seed, **attrs):
        m = _module(xq, 'ls-1', 64, 20, 3, CLAMPS[1], seed=seed, padding=1).to(DEV)
        m.act_half = True
        m.__dict__.update(attrs)
        return m

    cases = [
        (mod('ls-1', 91).train(), x.to(bf), bf, False),
        (mod('gf-3', 92).eval(), x.to(bf).requires_grad_(True), bf, True),
        (mod('ls-1', 93).eval().bfloat16(), x.to(bf), None, False),
        (mod('ls-1', 94).eval(), x.to(fp), bf, False),
        (mod('fp', 95).eval(), x.to(bf), bf, False),
        (mod('ls-2', 96, act_half_solve=False).eval(), x.to(bf), bf, False),
    ]
    for m, xin, autocast, grad in cases:
        with torch.set_grad_enabled(grad), torch.autocast('cuda', dtype=autocast or bf, enabled=autocast is not None):
            assert not m._wants_hip(xin)
            y = m(xin)
            ref = m._forward_torch(xin)
        assert torch.equal(y, ref)
    print(f'calls: lsq_act_quant_half {counters["half"]}, lsq_act_quant {counters["act"]}')
    assert (counters['half'], counters['act']) == (0, 0)
