"""lsq_act_quant_bn_half (liblsq_hip_conv_act_bn_half.so) on the GPU, through the C ABI's Python wrapper, bf16 and fp16:
planes (interior words and untouched halo), scales and status bit for bit against lsq_act_quant_half on the materialised
tensor ``folded(x, scale, shift)``; the free-running v1 also against the exact oracle on that tensor; the identity set and
the call without arrays against lsq_act_quant_half on x; unaligned x; independence of the batch; refusals that write
nothing.  The accuracy of ``folded`` itself against fp64 runs on the CPU (no gpu mark).

Geometry numbers in the docstrings count from 1 as in conv_act_half_cases.GEOMS' comments; ``gi`` counts from 0.  Where a
request names "geometries a and b" the tests cover both readings of the numbers.

Every test prints the figure it asserts on (pytest -s shows them)."""

import ctypes

import pytest
import torch

import conv_act_bn_half_cases as B
import conv_act_half_cases as C

gpu = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = C.DTYPES
LS1, LS2, LST, GF = 1, 2, 3, 4
E_NULL, E_SCHEME, E_UNSUPPORTED = -1, -3, -6
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


def _quant(x, gi, scheme, k, alpha, skip=3, forced=None, fill=0, pre=None, null_pre=False):
    """One quantizer call on x [N, C, H, W] (on the GPU): lsq_act_quant_bn_half with ``pre`` = (scale, shift) on the GPU,
    the same entry point with both arrays NULL (``null_pre``), else lsq_act_quant_half.  The planes' interior is pre-filled
    with `fill`, their halo and the guard words around planes, scales and status with sentinels, which must come back
    untouched.  Returns the WHOLE plane buffer [k, N, Gt, Hp, Wp] int64 (halo included), scales [k, N], status [N] on the
    CPU."""
    hip = _hip()
    n = x.shape[0]
    pbuf, planes = _prepared(gi, n, k, fill)
    sbuf = torch.full((GUARD + k * n + GUARD,), SENTINEL_SCALE, device=DEV)
    tbuf = torch.full((GUARD + n + GUARD,), SENTINEL_STATUS, dtype=torch.int32, device=DEV)
    scales, status = sbuf[GUARD:GUARD + k * n].view(k, n), tbuf[GUARD:GUARD + n]
    if pre is not None:
        hip.act_quant_bn_half(x, _geom(gi, n), scheme, k, skip, alpha, planes, scales, forced, pre, status)
    elif null_pre:
        rc = hip.conv_act_bn_half_lib().lsq_act_quant_bn_half(
            x.data_ptr(), hip.LINEAR_HALF_DTYPES[x.dtype], ctypes.byref(_geom(gi, n)), scheme, k, skip, float(alpha), None, None,
            hip.ptr(forced), planes.data_ptr(), scales.data_ptr(), status.data_ptr(), hip.stream_ptr(x.device))
        assert rc == 0
    else:
        hip.act_quant_half(x, _geom(gi, n), scheme, k, skip, alpha, planes, scales, forced, status)
    torch.cuda.synchronize()
    assert (pbuf[:GUARD] == SENTINEL_WORD).all() and (pbuf[GUARD + planes.numel():] == SENTINEL_WORD).all()
    assert (sbuf[:GUARD] == SENTINEL_SCALE).all() and (sbuf[GUARD + k * n:] == SENTINEL_SCALE).all()
    assert (tbuf[:GUARD] == SENTINEL_STATUS).all() and (tbuf[GUARD + n:] == SENTINEL_STATUS).all()
    out = planes.view(k, n, *C.plane_shape(gi, n)).cpu()
    c, h, w, groups, (ph, pw) = C.GEOMS[gi]
    halo = torch.ones(out.shape[-2:], dtype=torch.bool)
    halo[ph:ph + h, pw:pw + w] = False
    assert bool((out[..., halo] == SENTINEL_WORD).all())
    return out, scales.cpu().clone(), status.cpu().clone()


def _differ(a, b):
    """Words of planes, scales (as bits) and status that differ between two results of _quant."""
    return ((a[0] != b[0]).sum().item() + (a[1].view(torch.int32) != b[1].view(torch.int32)).sum().item()
            + (a[2] != b[2]).sum().item())


def _given(k, n, seed):
    """Per-sample scales of a decreasing chain."""
    import detgen
    base = detgen.uniform(f'convactbnhalf.v.{seed}', (1, n), 0.5, 1.1, seed=seed)
    return torch.cat([base * 0.55 ** q for q in range(k)]).contiguous()


def _pre(gi, dt, which):
    return tuple(t.to(DEV) for t in B.params(gi, dt, which))


# (name, LSQ_SCHEME_*, k, skip, scales given)
SCHEMES = [('ls-1', LS1, 1, 3, False), ('gf-3', GF, 3, 3, False), ('ls-2 skip 1', LS2, 2, 1, False),
           ('ls-2 skip 3', LS2, 2, 3, False), ('ls-T', LST, 2, 3, False), ('ls-2 given', LS2, 2, 3, True),
           ('gf-3 given', GF, 3, 3, True)]
# the parameter sets of a geometry: 'mixed' everywhere; the edge and (fp16) overflow sets at geometries 4, 5 and 6
EDGE_GEOMS = (3, 4, 5)


def _sets(gi, dt):
    return ('mixed',) + ((('edges',) + (('overflow',) if dt == 'fp16' else ())) if gi in EDGE_GEOMS else ())


@gpu
@pytest.mark.parametrize('si', range(len(SCHEMES)))
@pytest.mark.parametrize('gi', range(len(C.GEOMS)))
@pytest.mark.parametrize('dt', DTYPES)
def test_composition(dt, gi, si):
    """Every geometry x scheme x type, the clamp bounds none / 2.0 / 0.5 each: planes (interior and halo), scales and status
    of lsq_act_quant_bn_half on x equal lsq_act_quant_half's on folded(x, scale, shift) bit for bit; for free-running
    ls-2 / ls-T v1 also equals the exact oracle on folded(...).  The overflow set (fp16: t holds +-inf) only under a clamp."""
    name, scheme, k, skip, given = SCHEMES[si]
    dtype = DTYPES[dt]
    n = C.batch_size(gi)
    x = C.batch(gi, dt).to(DEV)
    forced = _given(k, n, seed=si).to(DEV) if given else None
    for which in _sets(gi, dt):
        t16 = B.folded_batch(gi, dt, which)
        t = t16.to(DEV)
        pre = _pre(gi, dt, which)
        for bound in B.FOLD_BOUNDS:
            if which == 'overflow' and bound < 0:
                continue
            alpha = C.rounded(bound, dtype)
            got = _quant(x, gi, scheme, k, alpha, skip, forced, fill=-1, pre=pre)
            want = _quant(t, gi, scheme, k, alpha, skip, forced, fill=-1)
            differ = _differ(got, want)
            what = f'{name} {dt} geometry {gi + 1} N={n} set {which} alpha={alpha}'
            print(f'{what}: {differ} plane / scale / status words differ from lsq_act_quant_half on the folded tensor')
            assert differ == 0, what
            if scheme in (LS2, LST) and not given:
                m = t16[0].numel()
                xc = C.clamped32(t16.view(n, m), alpha)
                oracle, found = C.oracle_rows(xc, scheme == LST, skip)
                wrong = (got[1][0].view(torch.int32) != torch.from_numpy(oracle).view(torch.int32)).sum().item()
                print(f'{what}: v1 differs from the oracle on the folded tensor in {wrong} rows')
                assert wrong == 0, what


@gpu
@pytest.mark.parametrize('gi', (0, 3, 4, 7, 8))
@pytest.mark.parametrize('dt', DTYPES)
def test_identity_and_null_arrays(dt, gi):
    """scale 1, shift 0 and the call with both arrays NULL give the bits of lsq_act_quant_half on x (geometries 1, 4, 5, 8, 9)."""
    dtype = DTYPES[dt]
    n = C.batch_size(gi)
    x = C.batch(gi, dt).to(DEV)
    pre = _pre(gi, dt, 'identity')
    for name, scheme, k, skip, given in SCHEMES:
        forced = _given(k, n, seed=1).to(DEV) if given else None
        for bound in (-1, 0.5):
            alpha = C.rounded(bound, dtype)
            want = _quant(x, gi, scheme, k, alpha, skip, forced)
            differ = [_differ(_quant(x, gi, scheme, k, alpha, skip, forced, pre=pre), want),
                      _differ(_quant(x, gi, scheme, k, alpha, skip, forced, null_pre=True), want)]
            print(f'{name} {dt} geometry {gi + 1} alpha={alpha}: {differ} words differ (identity set, NULL arrays)')
            assert differ == [0, 0]


@gpu
@pytest.mark.parametrize('gi', (1, 2, 3, 6, 7))
@pytest.mark.parametrize('dt', DTYPES)
def test_unaligned_inputs_give_the_same_bits(dt, gi):
    """x at an offset of one element (2 bytes: every wide load is left) against the aligned copy (geometries 2, 3, 4, 7, 8)."""
    dtype = DTYPES[dt]
    alpha = C.rounded(2.0, dtype)
    x = C.batch(gi, dt).to(DEV)
    pre = _pre(gi, dt, 'mixed')
    assert x.data_ptr() % 16 == 0
    buf = torch.empty((x.numel() + 1,), dtype=dtype, device=DEV)
    buf[1:] = x.view(-1)
    xu = buf[1:].view(x.shape)
    assert xu.data_ptr() % 16 == 2 and xu.is_contiguous()
    for name, scheme, k, skip, given in SCHEMES:
        forced = _given(k, x.shape[0], 3).to(DEV) if given else None
        differ = _differ(_quant(x, gi, scheme, k, alpha, skip, forced, pre=pre), _quant(xu, gi, scheme, k, alpha, skip, forced, pre=pre))
        print(f'{name} {dt} geometry {gi + 1}: {differ} words differ between the aligned and the offset input')
        assert differ == 0


@gpu
@pytest.mark.parametrize('gi', (2, 3, 6, 7))
@pytest.mark.parametrize('dt', DTYPES)
def test_a_samples_result_does_not_depend_on_the_batch(dt, gi):
    """The same sample alone and as sample 0, 2 and 4 of a batch of 5 gives the same scale bits, words and status
    (geometries 3, 4, 7, 8)."""
    dtype = DTYPES[dt]
    batch = C.batch(gi, dt, 5).clone()
    sample = batch[1].clone()
    for r in (0, 2, 4):
        batch[r] = sample
    alpha = C.rounded(2.0, dtype)
    pre = _pre(gi, dt, 'mixed')
    for name, scheme, k, skip, given in SCHEMES:
        if given:
            continue
        p1, s1, t1 = _quant(sample[None].to(DEV), gi, scheme, k, alpha, skip, pre=pre)
        pb, sb, tb = _quant(batch.to(DEV), gi, scheme, k, alpha, skip, pre=pre)
        differ = sum((sb[:, r].view(torch.int32) != s1[:, 0].view(torch.int32)).sum().item() + (pb[:, r] != p1[:, 0]).sum().item()
                     + int(tb[r] != t1[0]) for r in (0, 1, 2, 4))
        print(f'{name} {dt} geometry {gi + 1}: {differ} scale / plane / status words differ between the sample alone and in the batch')
        assert differ == 0


@pytest.mark.parametrize('gi', range(len(C.GEOMS)))
@pytest.mark.parametrize('dt', DTYPES)
def test_the_folded_value_is_the_correctly_rounded_affine_map(dt, gi):
    """The mixed set on the CPU: |float(t) - (x s + b in fp64)| <= half an ulp of the type at |t| + 2^-22 (|x s| + |b|).
    The second term bounds the two fp32 roundings (2^-24 |x s| and 2^-24 |x s + b| <= 2^-24 (|x s| + |b|)) with a factor 2
    of margin; ulp(t) is the spacing of the type at |t| (the subnormal spacing below the smallest normal)."""
    dtype = DTYPES[dt]
    x = C.batch(gi, dt)
    s, b = B.params(gi, dt, 'mixed')
    t = B.folded_batch(gi, dt, 'mixed').double()
    xs = x.double() * s.double().view(1, -1, 1, 1)
    exact = xs + b.double().view(1, -1, 1, 1)
    mant = 8 if dtype == torch.bfloat16 else 11                    # significand bits, the hidden one included
    tiny = torch.finfo(dtype).tiny
    ulp = torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(tiny))) - (mant - 1))
    bound = 0.5 * ulp + 2.0 ** -22 * (xs.abs() + b.double().abs().view(1, -1, 1, 1))
    worst = ((t - exact).abs() / bound).max().item()
    print(f'{dt} geometry {gi + 1}: max |t - exact| / bound = {worst:.4f}')
    assert torch.isfinite(t).all() and worst <= 1.0


@gpu
def test_refused_calls_write_nothing():
    """One pre-array alone, a wrong dtype, a wrong k: the code, and planes, scales and status as they were."""
    hip = _hip()
    gi, n = 2, 3
    x = C.batch(gi, 'bf16').to(DEV)
    scale, shift = _pre(gi, 'bf16', 'mixed')
    code = hip.LINEAR_HALF_DTYPES
    fn = hip.conv_act_bn_half_lib().lsq_act_quant_bn_half
    good = _geom(gi, n)
    # (dtype code, scheme, k, pre_scale, pre_shift, expected)
    refusals = ((code[torch.bfloat16], LS1, 1, scale, None, E_NULL), (code[torch.bfloat16], LS2, 2, None, shift, E_NULL),
                (code[torch.float32], LS1, 1, scale, shift, E_UNSUPPORTED), (code[torch.float32], GF, 3, None, None, E_UNSUPPORTED),
                (code[torch.bfloat16], LS2, 1, scale, shift, E_SCHEME), (code[torch.float16], GF, 9, scale, shift, E_SCHEME),
                (code[torch.bfloat16], LS1, 2, None, None, E_SCHEME))
    for xdt, scheme, k, ps, pb, expected in refusals:
        kk = min(max(k, 1), 8)
        pbuf, planes = _prepared(gi, n, kk, SENTINEL_WORD)
        scales = torch.full((kk, n), SENTINEL_SCALE, device=DEV)
        status = torch.full((n,), SENTINEL_STATUS, dtype=torch.int32, device=DEV)
        rc = fn(x.data_ptr(), xdt, ctypes.byref(good), scheme, k, 3, 2.0, hip.ptr(ps), hip.ptr(pb), None, planes.data_ptr(),
                scales.data_ptr(), status.data_ptr(), None)
        torch.cuda.synchronize()
        print(f'scheme={scheme} k={k} dtype={xdt} pre=({ps is not None}, {pb is not None}): code {rc}')
        assert rc == expected
        assert (pbuf == SENTINEL_WORD).all() and (scales == SENTINEL_SCALE).all() and (status == SENTINEL_STATUS).all()
    with pytest.raises(TypeError):
        hip.act_quant_bn_half(x.float(), good, LS1, 1, 3, 2.0, torch.zeros((hip.act_plane_words(good),), dtype=torch.int64, device=DEV),
                              torch.zeros((1, n), device=DEV), None, (scale, shift))
