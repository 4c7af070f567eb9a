"""lsq_linear_act_quant_solve_half (liblsq_hip_linear_act_solve.so) and QuantLinear with free-running ls-2 / ls-T activations on
bf16 / fp16 inputs on the GPU: v1 bit for bit against the exact oracle and against lsq_solve_rows on x.float(); the planes
against a CPU fp32 restatement of the chain, lsq_linear_act_quant_half with the kernel's scales and lsq_act_quant on x.float()
free-running; v2 against the fp64 mean; zeros, -0.0, constant and fully clamped rows, subnormals; invariance to the batch,
determinism, alignment, pre-filled planes, guard words; the module's dispatch with ``act_half_solve`` on and off.

Every test prints the figure it asserts on (pytest -s shows them)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import act_solve_half_cases as C
import detgen
from oracle import ref_port as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = C.DTYPES
LS2, LST = 2, 3
SCHEME = {'ls-2': LS2, 'ls-T': LST}
# |v2 - v64| <= SCALE_BOUND * v64 against the fp64 mean of the fp32 magnitudes |res_1|: derived, not measured -- the fp32 sum
# of 8 non-negative terms carries at most 7 roundings of 2^-24, the final conversion to fp32 one more
SCALE_BOUND = 2.0 ** -21
GUARD = 5                         # words / floats / ints around planes, scales and status
SENTINEL_WORD, SENTINEL_SCALE, SENTINEL_STATUS = 0x5A5A5A5A5A5A5A5A, 12345.0, -77


def _hip():
    from quant import _hip
    return _hip


def _nw(L):
    return (L + 63) // 64


def _i32(t):
    return t.contiguous().view(torch.int32)


def _solve(x, scheme, skip, alpha, fill=SENTINEL_WORD):
    """The kernel on x [N, L] (on the GPU) with `alpha` already a value of x's type; planes pre-filled with `fill`; planes,
    scales and status inside guard words that must come back untouched.  Returns (planes [2, N, nw] int64, scales [2, N],
    status [N] int32) on the CPU."""
    hip = _hip()
    n, L = x.shape
    words = 2 * n * _nw(L)
    pbuf = torch.full((GUARD + words + GUARD,), fill, dtype=torch.int64, device=DEV)
    pbuf[:GUARD] = SENTINEL_WORD
    pbuf[GUARD + words:] = SENTINEL_WORD
    sbuf = torch.full((GUARD + 2 * n + GUARD,), SENTINEL_SCALE, device=DEV)
    tbuf = torch.full((GUARD + n + GUARD,), SENTINEL_STATUS, dtype=torch.int32, device=DEV)
    planes, scales, status = pbuf[GUARD:GUARD + words], sbuf[GUARD:GUARD + 2 * n].view(2, n), tbuf[GUARD:GUARD + n]
    hip.linear_act_quant_solve_half(x, scheme, skip, alpha, planes, scales, status)
    torch.cuda.synchronize()
    assert (pbuf[:GUARD] == SENTINEL_WORD).all() and (pbuf[GUARD + words:] == SENTINEL_WORD).all()
    assert (sbuf[:GUARD] == SENTINEL_SCALE).all() and (sbuf[GUARD + 2 * n:] == SENTINEL_SCALE).all()
    assert (tbuf[:GUARD] == SENTINEL_STATUS).all() and (tbuf[GUARD + n:] == SENTINEL_STATUS).all()
    return planes.view(2, n, _nw(L)).cpu(), scales.cpu().clone(), status.cpu().clone()


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


def _given_half(x, scheme, alpha, scales):
    """lsq_linear_act_quant_half on x with the given scales."""
    hip = _hip()
    n, L = x.shape
    planes = torch.full((2 * n * _nw(L),), SENTINEL_WORD, dtype=torch.int64, device=DEV)
    out = torch.empty((2, n), device=DEV)
    hip.linear_act_quant_half(x, scheme, 2, alpha, planes, out, scales.to(DEV).contiguous())
    torch.cuda.synchronize()
    return planes.view(2, n, _nw(L)).cpu()


def _free_act_quant(x, scheme, skip, alpha):
    """lsq_act_quant on x.float(), free-running: (planes [2, N, nw], scales [2, N]) on the CPU."""
    hip = _hip()
    n, L = x.shape
    geom = hip.make_geom(n, L, 1, 1, 1, 1, 1, (1, 1), (0, 0), (1, 1), 1)
    planes = torch.zeros((2 * hip.act_plane_words(geom),), dtype=torch.int64, device=DEV)
    out = torch.empty((2, n), device=DEV)
    hip.act_quant(x.float(), geom, scheme, 2, skip, alpha, planes, out)
    torch.cuda.synchronize()
    return planes.view(2, n, _nw(L)).cpu(), out.cpu()


_RUN = {}


def _run(li, dt, bound, skip, scheme):
    """The kernel on a case of act_solve_half_cases, once per case, shared by the tests below (nothing writes into it)."""
    key = (li, dt, bound, skip, scheme)
    if key not in _RUN:
        x = C.rows(li, dt).to(DEV)
        _RUN[key] = _solve(x, SCHEME[scheme], skip, C.rounded(bound, DTYPES[dt]))
    return _RUN[key]


def _combos():
    return [(b, skip, scheme) for b in C.BOUNDS for skip in C.SKIPS for scheme in C.SCHEMES]


# ------------------------------------------------------------------------------------------------ the solve
@pytest.mark.parametrize('li', range(len(C.LS)))
@pytest.mark.parametrize('dt', DTYPES)
def test_v1_is_the_exact_oracles_and_lsq_solve_rows(dt, li):
    """Every case: v1 bits equal oracle.lsq_exact on the clamped x.float() and lsq_solve_rows on x.float() with the same
    rounded bound; status says whether the oracle found a candidate."""
    hip = _hip()
    L = C.LS[li]
    x32 = C.rows(li, dt).to(DEV).float()
    for bound, skip, scheme in _combos():
        alpha = C.rounded(bound, DTYPES[dt])
        _, scales, status = _run(li, dt, bound, skip, scheme)
        want, found = C.oracle(li, dt, bound, skip, scheme)
        v12, _ = hip.solve_rows(x32, skip, scheme == 'ls-T', alpha)
        differ = (_i32(scales[0]) != torch.from_numpy(want.view(np.int32))).sum().item()
        differ_hip = (_i32(scales[0]) != _i32(v12[0].cpu())).sum().item()
        wrong_status = (status.bool() != torch.from_numpy(found)).sum().item()
        print(f'{scheme} {dt} L={L} alpha={alpha} skip={skip}: {differ} rows differ from lsq_exact, {differ_hip} from '
              f'lsq_solve_rows, {wrong_status} status words wrong ({int((~found).sum())} rows without a candidate)')
        assert differ == 0 and differ_hip == 0 and wrong_status == 0
        assert set(status.tolist()) <= {0, 1}


@pytest.mark.parametrize('li', range(len(C.LS)))
@pytest.mark.parametrize('dt', DTYPES)
def test_planes_and_v2(dt, li):
    """Every case: the planes equal the CPU chain with the kernel's scales, lsq_linear_act_quant_half given those scales and
    lsq_act_quant on x.float() free-running; ls-2: v2 within the derived bound of the fp64 mean of |res_1|; ls-T: v2 is v1."""
    L = C.LS[li]
    x = C.rows(li, dt).to(DEV)
    for bound, skip, scheme in _combos():
        alpha = C.rounded(bound, DTYPES[dt])
        planes, scales, _ = _run(li, dt, bound, skip, scheme)
        bits, mags = _chain(x.cpu().float(), alpha, scales)
        wrong = (planes != _pack(bits)).sum().item()
        wrong_half = (planes != _given_half(x, SCHEME[scheme], alpha, scales)).sum().item()
        wrong_act = (planes != _free_act_quant(x, SCHEME[scheme], skip, alpha)[0]).sum().item()
        print(f'{scheme} {dt} L={L} alpha={alpha} skip={skip}: {wrong} words differ from the CPU chain, {wrong_half} from '
              f'lsq_linear_act_quant_half, {wrong_act} from lsq_act_quant')
        assert wrong == 0 and wrong_half == 0 and wrong_act == 0
        if scheme == 'ls-T':
            assert torch.equal(_i32(scales[1]), _i32(scales[0]))
        else:
            v64 = mags[1].double().mean(dim=1)
            rel = ((scales[1].double() - v64).abs() / v64.clamp_min(1e-300)).max().item()
            print(f'    max |v2 - v64| / v64 = {rel:.3e} (bound {SCALE_BOUND:.3e})')
            assert ((scales[1].double() - v64).abs() <= SCALE_BOUND * v64).all()


# ------------------------------------------------------------------------------------------------ special rows
def _against_oracle(x, alpha, what):
    """x [n, L] (CPU, 16-bit) through both schemes and skips: v1 and status against lsq_exact, planes against the CPU chain.
    Returns {(scheme, skip): (planes, scales, oracle v1)}."""
    out = {}
    for scheme in C.SCHEMES:
        for skip in C.SKIPS:
            planes, scales, status = _solve(x.to(DEV), SCHEME[scheme], skip, alpha)
            want, found = C.oracle_rows(C.clamped32(x, alpha), scheme == 'ls-T', skip)
            print(f'{what} {scheme} skip={skip}: v1 {scales[0].tolist()} oracle {want.tolist()} v2 {scales[1].tolist()} '
                  f'status {status.tolist()}')
            assert torch.equal(_i32(scales[0]), torch.from_numpy(want.view(np.int32)))
            assert torch.equal(status.bool(), torch.from_numpy(found))
            bits, _ = _chain(x.float(), alpha, scales)
            assert torch.equal(planes, _pack(bits))
            out[(scheme, skip)] = (planes, scales, want)
    return out


@pytest.mark.parametrize('L', (65, 4104))
@pytest.mark.parametrize('dt', DTYPES)
def test_zero_rows_and_negative_zero(dt, L):
    """An all-zero row and a row of -0.0: v1 = v2 = +0, every bit 1 up to L and 0 past it."""
    x = torch.zeros((2, L), dtype=DTYPES[dt])
    x[1] = -0.0
    assert (x[1].view(torch.int16) == -32768).all()
    ones = _pack(torch.ones((2, 2, L), dtype=torch.bool))
    for (scheme, skip), (planes, scales, _) in _against_oracle(x, 2.0, f'zeros {dt} L={L}').items():
        assert (scales == 0).all() and not torch.signbit(scales).any()
        assert torch.equal(planes, ones)


@pytest.mark.parametrize('L', (65, 4104))
@pytest.mark.parametrize('dt', DTYPES)
def test_constant_and_fully_clamped_rows(dt, L):
    """A row of 0.75 (one key holds the whole row: ls-2 finds v1 = c inside the run, ls-T its extra candidate c / 2) and rows
    with |x| >= 2 under the bound 0.5 (every element on key(alpha), both signs): whatever lsq_exact says."""
    dtype = DTYPES[dt]
    const = torch.full((1, L), 0.75, dtype=dtype)
    res = _against_oracle(const, -1.0, f'constant {dt} L={L}')
    for skip in C.SKIPS:
        print(f'constant {dt} L={L} skip={skip}: ls-2 v1 {res[("ls-2", skip)][1][0].item()}, ls-T v1 {res[("ls-T", skip)][1][0].item()}')
        assert res[('ls-2', skip)][2][0] == np.float32(0.75) and res[('ls-T', skip)][2][0] == np.float32(0.375)
    big = detgen.normal(f'actsolvehalf.big.{L}', (3, L), seed=L, scale=1.0)
    big = (big + torch.where(big >= 0, 2.0, -2.0)).to(dtype)
    assert (big.float().abs() >= 2).all()
    _against_oracle(big, 0.5, f'clamped {dt} L={L}')


@pytest.mark.parametrize('dt', DTYPES)
def test_negative_subnormals(dt):
    """64 distinct negative subnormals -k * (smallest subnormal), k = 1 .. 64: the oracle's v1 (a flushed row would give 0),
    every bit of plane 0 is 0 (a flushed value would be -0.0: bit 1)."""
    dtype = DTYPES[dt]
    tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133
    x = (-torch.arange(1, 65, dtype=torch.float64) * tiny).to(dtype).view(1, 64)
    assert torch.equal(x.double(), -torch.arange(1, 65, dtype=torch.float64).view(1, 64) * tiny)
    for (scheme, skip), (planes, scales, want) in _against_oracle(x, -1.0, f'subnormals {dt}').items():
        assert want[0] > 0 and planes[0].item() == 0


# ------------------------------------------------------------------------------------------------ batch, alignment, fill
@pytest.mark.parametrize('L', (800, 4104, 70001))
@pytest.mark.parametrize('dt', DTYPES)
def test_a_rows_result_does_not_depend_on_the_batch(dt, L):
    """The same row alone and as rows 0 / 150 / 299 of a batch of 300 (rows 0 / 1 / 2 of 3 at 70001): the same scale bits and
    plane words; two runs: the same bits."""
    dtype = DTYPES[dt]
    n = 300 if L < 70001 else 3
    batch = detgen.normal(f'actsolvehalf.batch.{L}', (n, L), seed=L, scale=1.2).to(dtype).to(DEV)
    at = (0, n // 2, n - 1)
    row = batch[1 if n == 3 else 17].clone()
    for r in at:
        batch[r] = row
    alpha = C.rounded(1.3, dtype)
    for scheme in C.SCHEMES:
        p1, s1, t1 = _solve(row.view(1, L), SCHEME[scheme], 3, alpha)
        pb, sb, tb = _solve(batch, SCHEME[scheme], 3, alpha)
        pb2, sb2, tb2 = _solve(batch, SCHEME[scheme], 3, alpha)
        differ = sum((_i32(sb[:, r]) != _i32(s1[:, 0])).sum().item() + (pb[:, r] != p1[:, 0]).sum().item() + int(tb[r] != t1[0])
                     for r in at)
        print(f'{scheme} {dt} L={L}: {differ} scale / plane / status words differ between the row alone and in the batch')
        assert differ == 0
        assert torch.equal(pb, pb2) and torch.equal(_i32(sb), _i32(sb2)) and torch.equal(tb, tb2)


@pytest.mark.parametrize('dt', DTYPES)
def test_unaligned_rows_give_the_same_bits(dt):
    """x at an odd element offset with odd L (2-byte loads) against the aligned copy; and, with L % 8 == 0, the 2-byte loads
    of a misaligned x against the 16-byte loads of the aligned one."""
    dtype = DTYPES[dt]
    alpha = C.rounded(1.3, dtype)
    for n, L in ((7, 801), (3, 4105), (7, 800), (3, 4104)):
        x = detgen.normal(f'actsolvehalf.align.{L}', (n, L), seed=L, scale=1.2).to(dtype).to(DEV)
        assert x.data_ptr() % 16 == 0
        buf = torch.empty((n * L + 1,), dtype=dtype, device=DEV)
        buf[1:] = x.view(-1)
        xu = buf[1:].view(n, L)
        assert xu.data_ptr() % 16 == 2 and xu.is_contiguous()
        for scheme in C.SCHEMES:
            for skip in C.SKIPS:
                pa, sa, ta = _solve(x, SCHEME[scheme], skip, alpha)
                pu, su, tu = _solve(xu, SCHEME[scheme], skip, alpha)
                differ = (pa != pu).sum().item() + (_i32(sa) != _i32(su)).sum().item() + (ta != tu).sum().item()
                print(f'{scheme} {dt} N={n} L={L} skip={skip}: {differ} words differ between the aligned and the offset rows')
                assert differ == 0


@pytest.mark.parametrize('dt', DTYPES)
def test_prefilled_planes_come_out_with_zero_tails(dt):
    """planes pre-filled with all ones and with zeros come out equal: every word is written in full, the bits past L are 0."""
    dtype = DTYPES[dt]
    for L in (1, 63, 65, 4104 + 5):
        x = detgen.normal(f'actsolvehalf.fill.{L}', (7, L), seed=L, scale=1.2).to(dtype).to(DEV)
        for scheme in C.SCHEMES:
            ones, _, _ = _solve(x, SCHEME[scheme], 3, 2.0, fill=-1)
            zeros, _, _ = _solve(x, SCHEME[scheme], 3, 2.0, fill=0)
            assert torch.equal(ones, zeros)
            tail = ones[..., -1] >> (L % 64)            # (arithmetic shift: a set top bit would show as -1)
            print(f'{scheme} {dt} L={L}: tail bits {tail.abs().max().item()}')
            assert (tail == 0).all()


def test_status_is_optional_and_errors_write_nothing():
    hip = _hip()
    n, L = 7, 800
    x = C.rows(5, 'bf16').to(DEV)
    planes = torch.full((2 * n * _nw(L),), SENTINEL_WORD, dtype=torch.int64, device=DEV)
    scales = torch.full((2, n), SENTINEL_SCALE, device=DEV)
    code = hip.LINEAR_HALF_DTYPES
    lib = hip.linear_act_solve_lib()
    for kw in (dict(scheme=1), dict(scheme=4), dict(skip=0), dict(xdt=code[torch.float32])):
        a = dict(xdt=code[torch.bfloat16], scheme=LS2, skip=3)
        a.update(kw)
        rc = lib.lsq_linear_act_quant_solve_half(x.data_ptr(), a['xdt'], n, L, a['scheme'], a['skip'], 2.0, planes.data_ptr(),
                                                 scales.data_ptr(), None, None)
        torch.cuda.synchronize()
        print(f'{kw}: code {rc}')
        assert rc < 0
        assert (planes == SENTINEL_WORD).all() and (scales == SENTINEL_SCALE).all()
    hip.linear_act_quant_solve_half(x, LS2, 3, 2.0, planes, scales)            # no status
    torch.cuda.synchronize()
    want, _ = C.oracle(5, 'bf16', 2.0, 3, 'ls-2')
    assert torch.equal(_i32(scales[0].cpu()), torch.from_numpy(want.view(np.int32)))


# ------------------------------------------------------------------------------------------------ QuantLinear
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
    names = {'solve': 'linear_act_quant_solve_half', 'half': 'linear_act_quant_half', 'act': 'act_quant', 'pack': 'pack_weight',
             'xnor': 'linear_xnor'}
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


def _act_workspace(m):
    """The module's one activation workspace: (planes, scales)."""
    ws = [v for k, v in m._hip_cache.items() if isinstance(k, tuple) and k[0] == 'act']
    assert len(ws) == 1
    return ws[0]


@pytest.mark.parametrize('shape', [(9, 128), (4, 3, 128), (5, 100)])
@pytest.mark.parametrize('xq', C.SCHEMES)
@pytest.mark.parametrize('dt', DTYPES)
def test_module_forward_with_act_half_solve(dt, xq, shape, counters):
    """act_half_solve = True: one lsq_linear_act_quant_solve_half, no lsq_act_quant, one lsq_linear_xnor, one weight pack;
    v1 and the planes are the cast route's (act_half_kernel = False); y within the resolution of a once-rounded 16-bit output,
    (2^-8 | 2^-11) + 1e-5 of max |y64|, of the fp64 oracle with the kernel's scales; the same bits under an autocast of the
    input's type; with act_half_solve = False the module stays on torch."""
    i = C.SCHEMES.index(xq)
    clamp = {'kind': 'symmetric', 'alpha': (2, 1.3)[(i + len(shape)) % 2]}
    ws = ('ls-2', 'ls-1')[i]
    f, o = shape[-1], 70
    m = _module(xq, ws, f, o, clamp, seed=171 + i).eval().to(DEV)
    x = detgen.normal(f'qlinactsolve.x.{i}', shape, scale=1.3).to(DEV).to(DTYPES[dt])
    with torch.no_grad():
        with torch.autocast('cuda', dtype=x.dtype):                      # (torch's F.linear needs it: 16-bit x, fp32 weights)
            assert not m._wants_hip(x)                                   # off by default
            y_torch = m(x)
            assert torch.equal(y_torch, m._forward_torch(x))
        assert (counters['solve'], counters['half'], counters['act'], counters['xnor']) == (0, 0, 0, 0)
        m.act_half_solve = True
        assert m._wants_hip(x)
        y = m(x)
        assert (counters['solve'], counters['half'], counters['act'], counters['xnor'], counters['pack']) == (1, 0, 0, 1, 1)
        scales = m.last_act_scales.clone()
        planes = _act_workspace(m)[0].clone()
        with torch.autocast('cuda', dtype=x.dtype):
            ya = m(x)
        assert (counters['solve'], counters['act'], counters['xnor'], counters['pack']) == (2, 0, 2, 1)
        m.act_half_kernel = False
        y_cast = m(x)
        assert (counters['solve'], counters['half'], counters['act'], counters['xnor'], counters['pack']) == (2, 0, 1, 3, 1)
        scales_cast = m.last_act_scales.clone()
        planes_cast = _act_workspace(m)[0].clone()
    assert y.dtype == x.dtype and y.shape == (*shape[:-1], o)
    assert ya.dtype == x.dtype and torch.equal(_bits(ya), _bits(y))
    n, t, k = shape[0], x.numel() // (shape[0] * f), 2
    assert scales.shape == (k, n)
    differ_v1 = (_i32(scales[0]) != _i32(scales_cast[0])).sum().item()
    differ_planes = (planes != planes_cast).sum().item()
    alpha = C.rounded(clamp['alpha'], x.dtype)
    # the fp64 oracle: the reference's quantizers on the clamped 16-bit rows with the kernel's scales
    xc = x.cpu().float().clamp(-alpha, alpha).reshape(n, t * f, 1, 1)
    vs = [scales[q].cpu().double() for q in range(k)]
    xq64 = P.quantize_activation(xc.double(), xq, scales=vs)[1].reshape(n * t, f)
    wq = P.quantize_weight(m.weight.detach().cpu().view(o, f, 1, 1), ws, [b.cpu() for b in m.w_approximate.cached_scales()])
    y64 = F.linear(xq64, wq.view(o, f).double(), m.bias.detach().cpu().double()).view(*shape[:-1], o)
    err = ((y.cpu().double() - y64).abs().max() / y64.abs().max()).item()
    bound = (2.0 ** -8 if x.dtype == torch.bfloat16 else 2.0 ** -11) + BOUND
    print(f'{xq} {dt} {shape} alpha={alpha}: {differ_v1} v1 and {differ_planes} plane words differ from the cast route; '
          f'max err / max|y64| = {err:.3e} (bound {bound:.3e})')
    assert differ_v1 == 0 and differ_planes == 0
    assert err <= bound


def test_paths_that_stay_on_torch_with_act_half_solve(counters):
    """Train mode, an input that wants a gradient and an autocast of the other type stay on the torch formulation with the
    attribute on."""
    x = detgen.normal('qlinactsolve.torch.x', (5, 128), scale=1.2).to(DEV)
    bf, fp = torch.bfloat16, torch.float16
    clamp = {'kind': 'symmetric', 'alpha': 2}

    def mod(seed):
        m = _module('ls-2', 'ls-1', 128, 20, clamp, seed=seed).to(DEV)
        m.act_half_solve = True
        return m

    cases = [(mod(191).train(), x.to(bf), bf, False), (mod(192).eval(), x.to(bf).requires_grad_(True), bf, True),
             (mod(193).eval(), x.to(fp), bf, False)]
    for m, xin, autocast, grad in cases:
        with torch.set_grad_enabled(grad), torch.autocast('cuda', dtype=autocast):
            assert not m._wants_hip(xin)
            y = m(xin)
            ref = m._forward_torch(xin)
        assert torch.equal(y, ref)
    print(f'calls: lsq_linear_act_quant_solve_half {counters["solve"]}, lsq_act_quant {counters["act"]}')
    assert (counters['solve'], counters['half'], counters['act']) == (0, 0, 0)
