"""ctypes binding of the gfx950 C-ABI library (``include/lsq_hip.h``).

PyTorch is used only as the owner of device memory and streams: every call passes raw
device pointers (``tensor.data_ptr()``) and the current HIP stream.  There is no CPU or
eager fallback here: if the library is missing, or a call fails, an exception is raised.
"""

import collections
import contextlib
import ctypes
import functools
import warnings
import os
import threading
from typing import Optional, Sequence, Tuple

import torch

from . import _sublibs
from ._sublibs import ConvGeom, NextLs1, ConvDgradPlan  # noqa: F401  (the mirrors of the C structs: public names of this module)

_LIB_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lib')
# (LSQ_HIP_LIB: developer builds, e.g. -DLSQ_PHASE_CLOCKS)
_LIB_PATH = os.environ.get('LSQ_HIP_LIB') or os.path.join(_LIB_DIR, 'liblsq_hip.so')
_lock = threading.Lock()
_lib = None

ABI_VERSION = 12
SCHEME_LS1, SCHEME_LS2, SCHEME_LST, SCHEME_GF = 1, 2, 3, 4
MAX_PLANES = 8
MAX_XNOR_KERNEL = 8          # lsq_xnor_conv2d: KH, KW <= 8
MAX_SOLVER_KEYS = 1 << 22    # lsq_act_quant LS-2 / LS-T: sub-sampled keys per row
XNOR_MFMA_MAX_OUTPUTS = 1 << 30      # lsq_xnor_conv2d: at this many outputs the popcount kernel serves the call (same bits)
_xnor_limit_warned = set()


class LsqHipError(RuntimeError):
    """A C-ABI call returned a non-zero code."""


def library_path() -> str:
    return _LIB_PATH


def _load(path, make_dir, prototypes, version_symbol, version, soname):
    """Load one of the C-ABI libraries: ``path`` must exist (no fallback: a missing library is an error that says how to
    build it, ``make -C ml-quant_amd/<make_dir>``), its functions get the ``prototypes`` of quant/_sublibs.py, and
    ``version_symbol()`` must return ``version``.  Loads are serialized; the caller keeps the handle."""
    with _lock:
        if not os.path.exists(path):
            raise LsqHipError(
                f'{path} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                f'(or `make -C ml-quant_amd/{make_dir}`). The HIP path has no fallback.')
        handle = ctypes.CDLL(path)
        _sublibs.apply_prototypes(handle, prototypes)
        if getattr(handle, version_symbol)() != version:
            raise LsqHipError(f'{soname} ABI version mismatch')
        return handle


def lib():
    """Load (once) and return the C-ABI library; raises if it has not been built."""
    global _lib
    if _lib is None:
        prototypes = {**_sublibs.MAIN_PROTOTYPES['lsq_hip.h'], **_sublibs.MAIN_PROTOTYPES['lsq_hip_debug.h']}
        _lib = _load(_LIB_PATH, 'csrc', prototypes, 'lsq_abi_version', ABI_VERSION, 'liblsq_hip.so')
    return _lib


def available() -> bool:
    return os.path.exists(_LIB_PATH)


def source_fingerprint() -> str:
    """sha256 over the kernel sources (csrc/*.hip, *.h, Makefile; names and contents, sorted): counter profiles record
    it when they are captured and bench.py attaches their figures only while it still matches -- a profile of older
    kernels is reported as stale instead of silently priced against the current ones."""
    import hashlib
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'csrc')
    h = hashlib.sha256()
    for name in sorted(os.listdir(src)):
        if name.endswith(('.hip', '.h')) or name == 'Makefile':
            h.update(name.encode() + b'\0')
            with open(os.path.join(src, name), 'rb') as f:
                h.update(f.read())
    return h.hexdigest()


def check(code: int, what: str) -> None:
    if code != 0:
        msg = lib().lsq_error_string(code).decode()
        raise LsqHipError(f'{what} failed with code {code}: {msg}')


def stream_ptr(device=None) -> int:
    """HIP stream the kernels of ``device`` are launched on (torch's current stream of THAT device)."""
    if _raw_stream is not None:               # (no Stream object built per launch: this runs several times per layer)
        d = torch.device(device) if device is not None else None
        return _raw_stream(torch.cuda.current_device() if d is None or d.index is None else d.index)
    return torch.cuda.current_stream(device).cuda_stream


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


_SAME_DEVICE = contextlib.nullcontext()
_UNTIMED = contextlib.nullcontext()


def _on(t: torch.Tensor):
    """Device guard for a C-ABI call: the library never calls hipSetDevice, so the tensor's device is made
    current around the launch (a model on cuda:1 with cuda:0 current must not launch on cuda:0's stream)."""
    if t.device.index == torch.cuda.current_device():
        return _SAME_DEVICE                    # (the common case: entering torch.cuda.device costs microseconds per launch)
    return torch.cuda.device(t.device)


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def make_geom(n, c, h, w, o, kh, kw, stride, padding, dilation, groups) -> ConvGeom:
    key = (n, c, h, w, o, kh, kw, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1], groups)
    g = ConvGeom(*key)
    g._key = key                                   # (valid as long as nobody writes the fields afterwards: nothing here does)
    return g


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f'the HIP path computes in fp32, got {t.dtype}')
    return t if t.is_contiguous() else t.contiguous()


# ---- optional per-kernel timing with HIP events on the launch stream (bench.py's roofline leg)
_timing = None
_timing_only = None
_timing_paused = False


def enable_timing(on: bool = True, only: Optional[Sequence[str]] = None) -> None:
    """Bracket every C-ABI call (or only the entry points named in ``only``) with HIP events on the launch
    stream.  An event pair costs a few microseconds of stream time per call, so benchmarks instrument only
    the kernel they report on inside their timed region."""
    global _timing, _timing_only
    _timing = {} if on else None
    _timing_only = None if only is None else frozenset(only)


def pause_timing(paused: bool = True) -> None:
    """Keep the records but stop (resume) bracketing calls: a benchmark samples some of its timed steps."""
    global _timing_paused
    _timing_paused = bool(paused)


def drain_timing(by_tag: bool = False):
    """{kernel: (launches, total_ms, total_algorithmic_bytes, total_ops, total_survey_bytes)}; call after
    torch.cuda.synchronize().  ops = binary MACs (xnor conv) or bf16 FLOPs (sign-weight conv), 0 for the quantizer;
    survey bytes = SURVEY 8(d)'s count (input once + output once, no residual operands).  ``by_tag``: keys are
    (kernel, tag) with the tag the call site attached (the layer's input channels and height)."""
    out = {}
    for name, recs in (_timing or {}).items():
        groups = {}
        for s, e, b in recs:
            groups.setdefault((name, b[2]) if by_tag else name, []).append((s.elapsed_time(e), b[0], b[1], b[3]))
        for key, rows in groups.items():
            out[key] = (len(rows), sum(r[0] for r in rows), sum(r[1] for r in rows), sum(r[2] for r in rows),
                        sum(r[3] for r in rows))
        recs.clear()
    return out


class _Timed:
    def __init__(self, name, nbytes, ops=0, tag=None, survey_bytes=None):
        # nbytes: every operand the call must move once (residuals of a fused epilogue included);
        # survey_bytes: SURVEY 8(d)'s definition for the path kernels (input read once + output written once)
        self.name, self.nbytes = name, (nbytes, ops, tag, nbytes if survey_bytes is None else survey_bytes)

    def __enter__(self):
        self.on = _timing is not None and not _timing_paused and (_timing_only is None or self.name in _timing_only)
        if self.on:                       # (events record on the current stream of the current device: call inside _on)
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()

    def __exit__(self, *exc):
        if self.on:
            self.e.record()
            _timing.setdefault(self.name, []).append((self.s, self.e, self.nbytes))


_ws_caches = collections.defaultdict(dict)      # {cache name: {(device, stream): buffer}}: one cache per kernel family, none shared
_WS_CACHE_MAX = 16      # (device, stream) entries kept per cache: streams come and go (one per captured graph)


def _remember(cache: dict, key, buf):
    cache.pop(key, None)
    cache[key] = buf                          # (insertion order = age: the oldest entries go first)
    while len(cache) > _WS_CACHE_MAX:
        cache.pop(next(iter(cache)))


_ws_bytes_memo = {}


def _ws_bytes(fn: str, rows: int) -> int:
    key = (fn, rows)
    need = _ws_bytes_memo.get(key)
    if need is None:
        if len(_ws_bytes_memo) > 256:
            _ws_bytes_memo.clear()
        need = _ws_bytes_memo[key] = getattr(lib(), fn)(rows)
    return need


def _stream_buffer(name: str, need: int, device, zeroed: bool = False) -> torch.Tensor:
    """The uint8 buffer of at least ``need`` bytes that the cache ``name`` keeps for (device, its current stream), grown on
    demand (``zeroed``: a new one starts as zeros) -- kernels of one stream run in order, so sharing it between calls is safe."""
    cache = _ws_caches[name]
    device = torch.device(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (device.index, stream_ptr(device))
    buf = cache.get(key)
    if buf is None or buf.numel() < need:
        buf = (torch.zeros if zeroed else torch.empty)((need,), dtype=torch.uint8, device=device)
        _remember(cache, key, buf)
    return buf


def solver_workspace(rows: int, device) -> torch.Tensor:
    """Scratch for the LS2/LST solve (slot records passed from the sweep to the solve kernel); cached per
    (device, stream) and grown on demand."""
    return _stream_buffer('solver', _ws_bytes('lsq_solver_workspace_bytes', rows), device)


def sweep_workspace(rows: int, device) -> torch.Tensor:
    """Row workspace of the ls-1 / gf-k sweeps (partial sums + arrival counters of rows shared by several workgroups):
    any content (the arrival slots carry a per-launch epoch); cached per (device, stream) like the solver's."""
    return _stream_buffer('sweep', _ws_bytes('lsq_sweep_workspace_bytes', rows), device, zeroed=True)


def _ws_args(ws: Optional[torch.Tensor]):
    """The (pointer, bytes) arguments of an optional workspace."""
    return (None, 0) if ws is None else (ws.data_ptr(), ws.numel())


def act_quant(x: torch.Tensor, geom: ConvGeom, scheme: int, k: int, skip: int, alpha: float,
              planes: torch.Tensor, scales: torch.Tensor, forced: Optional[torch.Tensor] = None,
              pre: Optional[tuple] = None) -> None:
    """pre = (scale[C], shift[C]) folds an eval-mode batch norm into the read."""
    x = _f32c(x)
    ws = None
    if forced is None:
        ws = solver_workspace(geom.N, x.device) if scheme in (SCHEME_LS2, SCHEME_LST) else sweep_workspace(geom.N, x.device)
    m = geom.C * geom.H * geom.W
    # (accounting -- x read once + k bit planes written -- only when a benchmark asked for it: the record costs microseconds)
    with _on(x), (_Timed('lsq_act_quant', geom.N * (4 * m + k * m // 8), 0, f'C{geom.C}_H{geom.H}') if _timing is not None else _UNTIMED):
        check(lib().lsq_act_quant(x.data_ptr(), ctypes.byref(geom), scheme, k, skip, float(alpha),
                                  None if pre is None else pre[0].data_ptr(), None if pre is None else pre[1].data_ptr(),
                                  ptr(forced), planes.data_ptr(), scales.data_ptr(), *_ws_args(ws), stream_ptr(x.device)),
              'lsq_act_quant')


def solve_rows(rows: torch.Tensor, skip: int, ternary: bool, alpha: float = -1.0):
    """Returns (v12 [2,R] fp32, status [R] int32)."""
    rows = _f32c(rows)
    r, m = rows.shape
    v12 = torch.empty((2, r), dtype=torch.float32, device=rows.device)
    status = torch.empty((r,), dtype=torch.int32, device=rows.device)
    ws = solver_workspace(r, rows.device)
    with _on(rows):
        check(lib().lsq_solve_rows(rows.data_ptr(), r, m, skip, int(ternary), float(alpha), v12.data_ptr(),
                                   status.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr(rows.device)), 'lsq_solve_rows')
    return v12, status


def pack_weight(w: torch.Tensor, geom: ConvGeom, scales: torch.Tensor):
    """scales [k, O] -> (wbits int64 [k * words], wsum int32 [k, O, taps])."""
    w = _f32c(w)
    scales = _f32c(scales)
    k = scales.shape[0]
    words = lib().lsq_weight_plane_words(ctypes.byref(geom))
    wbits = torch.empty((k * words,), dtype=torch.int64, device=w.device)
    wsum = torch.empty((k, geom.O, geom.KH * geom.KW), dtype=torch.int32, device=w.device)
    with _on(w):
        check(lib().lsq_pack_weight(w.data_ptr(), ctypes.byref(geom), k, scales.data_ptr(), wbits.data_ptr(),
                                    wsum.data_ptr(), stream_ptr(w.device)), 'lsq_pack_weight')
    return wbits, wsum


def act_plane_words(geom: ConvGeom) -> int:
    return lib().lsq_act_plane_words(ctypes.byref(geom))


def out_hw(geom: ConvGeom):
    ho = (geom.H + 2 * geom.pad_h - geom.dil_h * (geom.KH - 1) - 1) // geom.stride_h + 1
    wo = (geom.W + 2 * geom.pad_w - geom.dil_w * (geom.KW - 1) - 1) // geom.stride_w + 1
    return ho, wo


ACT_NONE, ACT_RELU, ACT_PRELU, ACT_PRELU_CHANNEL = 0, 1, 2, 3


def _act(relu: bool, prelu: Optional[torch.Tensor], out_channels: int):
    """(LSQ_ACT_* code, slope pointer) of the fused epilogue: ``prelu`` is an nn.PReLU weight (1 or O slopes)."""
    if prelu is None:
        return (ACT_RELU if relu else ACT_NONE), None
    if relu:
        raise LsqHipError('relu and prelu are exclusive')
    w = _f32c(prelu.detach())
    if w.numel() not in (1, out_channels):
        raise LsqHipError(f'PReLU with {w.numel()} slopes on {out_channels} channels')
    return (ACT_PRELU if w.numel() == 1 else ACT_PRELU_CHANNEL), w


def xnor_conv2d(planes: torch.Tensor, kx: int, xscales: torch.Tensor, wbits: torch.Tensor, wsum: torch.Tensor,
                wscales: torch.Tensor, bias: Optional[torch.Tensor], geom: ConvGeom, y: torch.Tensor,
                relu: bool = False, res_pre: Optional[torch.Tensor] = None,
                res_post: Optional[torch.Tensor] = None, prelu: Optional[torch.Tensor] = None) -> None:
    """y = act(conv + bias + res_pre) + res_post, act = ReLU (``relu``), PReLU (``prelu`` = its weight) or identity
    (the fused block epilogue is optional)."""
    act, slope = _act(relu, prelu, geom.O)
    m = geom.C * geom.H * geom.W
    macs = y.numel() * (geom.C // geom.groups) * geom.KH * geom.KW * kx * wscales.shape[0]
    nres = (res_pre is not None) + (res_post is not None)
    if y.numel() >= XNOR_MFMA_MAX_OUTPUTS and (geom.KH, geom.KW, geom.groups, geom.dil_h, geom.dil_w) == (3, 3, 1, 1, 1) \
            and geom.C in (64, 128, 256, 512) and geom.O % 32 == 0 and 'outputs' not in _xnor_limit_warned:
        # (csrc/lsq_xnor_mfma.hip indexes its output with 32 bits: a call this large is served by the popcount kernel -- same
        #  bits, about half the speed.  Said once, not silently.)
        _xnor_limit_warned.add('outputs')
        warnings.warn(f'lsq_xnor_conv2d: {y.numel()} outputs (2^30 or more): this call runs on the popcount kernel instead of the '
                      'fp4 matrix-core kernel (same result, about half the speed); split the batch to stay below 2^30 outputs')
    # algorithmic bytes: planes read + fp32 output written + every residual operand of the fused epilogue read
    with _on(y), (_Timed('lsq_xnor_conv2d', geom.N * kx * m // 8 + 4 * y.numel() * (1 + nres), macs, f'C{geom.C}_H{geom.H}_s{geom.stride_h}',
                         geom.N * kx * m // 8 + 4 * y.numel()) if _timing is not None else _UNTIMED):
        check(lib().lsq_xnor_conv2d(planes.data_ptr(), kx, xscales.data_ptr(), wbits.data_ptr(), wsum.data_ptr(),
                                    wscales.shape[0], wscales.data_ptr(), ptr(bias), ctypes.byref(geom), act, ptr(slope),
                                    ptr(res_pre), ptr(res_post), y.data_ptr(), stream_ptr(y.device)), 'lsq_xnor_conv2d')


E_UNSUPPORTED = -6


#: (projection input channels, out-channels) for which the fused launch measured faster on MI355X than lsq_pointwise_conv +
#: lsq_xnor_conv2d (profiles/proj_fused.json); every other shape keeps the two launches
PROJ_FUSED_SHAPES = frozenset({(64, 128), (128, 256), (256, 512)})


def proj_fused_wins(cp: int, o: int) -> bool:
    return (cp, o) in PROJ_FUSED_SHAPES


def xnor_conv2d_proj(planes: torch.Tensor, kx: int, xscales: torch.Tensor, wbits: torch.Tensor, wsum: torch.Tensor,
                     wscales: torch.Tensor, bias: Optional[torch.Tensor], geom: ConvGeom, y: torch.Tensor, proj: tuple,
                     relu: bool = False, res_pre: Optional[torch.Tensor] = None, res_post: Optional[torch.Tensor] = None,
                     prelu: Optional[torch.Tensor] = None) -> bool:
    """lsq_xnor_conv2d with the projection shortcut ``proj = (x, w [O, Cp], bias or None, stride, post)`` computed in the
    epilogue's residual registers (include/lsq_hip_conv_proj.h): ``post`` False = it plays ``res_pre``, True = ``res_post``.
    Returns False -- nothing launched, nothing written -- where the library refuses the call as unsupported (the caller runs
    ``pointwise_conv`` + ``xnor_conv2d``: same bits)."""
    px, pw, pb, stride, post = proj
    px, pw = _f32c(px), _f32c(pw)
    pb = None if pb is None else _f32c(pb)
    act, slope = _act(relu, prelu, geom.O)
    m = geom.C * geom.H * geom.W
    cp = px.shape[1]
    nres = (res_pre is not None) + (res_post is not None)
    macs = y.numel() * (geom.C // geom.groups) * geom.KH * geom.KW * kx * wscales.shape[0]
    pd = _sublibs.Proj(px.data_ptr(), pw.data_ptr(), ptr(pb), cp, px.shape[2], px.shape[3], int(stride), int(bool(post)))
    lib()                                           # (liblsq_hip_conv_proj.so links liblsq_hip.so: the same loaded object)
    # bytes: the convolution's own plus the projection's gathered input (one 4-byte value per output pixel and input channel);
    # ops stay the binary MACs, so the line's matrix-core fraction keeps its meaning
    with _on(y), (_Timed('lsq_xnor_conv2d', geom.N * kx * m // 8 + 4 * y.numel() * (1 + nres) + 4 * (y.numel() // geom.O) * cp,
                         macs, f'C{geom.C}_H{geom.H}_s{geom.stride_h}', geom.N * kx * m // 8 + 4 * y.numel())
                  if _timing is not None else _UNTIMED):
        code = conv_proj_lib().lsq_xnor_conv2d_proj(planes.data_ptr(), kx, xscales.data_ptr(), wbits.data_ptr(), wsum.data_ptr(),
                                                    wscales.shape[0], wscales.data_ptr(), ptr(bias), ctypes.byref(geom), act,
                                                    ptr(slope), ptr(res_pre), ptr(res_post), ctypes.byref(pd), y.data_ptr(),
                                                    stream_ptr(y.device))
    if code == E_UNSUPPORTED:
        return False
    check(code, 'lsq_xnor_conv2d_proj')
    return True


def xnor_conv2d_chain(planes: torch.Tensor, xscales: Optional[torch.Tensor], x_units: Optional[torch.Tensor], x_alpha: float,
                      wbits: torch.Tensor, wsum: torch.Tensor, wscales: torch.Tensor, bias: Optional[torch.Tensor],
                      geom: ConvGeom, y: torch.Tensor, relu: bool = False, res_pre: Optional[torch.Tensor] = None,
                      res_post: Optional[torch.Tensor] = None, prelu: Optional[torch.Tensor] = None,
                      nxt: Optional[NextLs1] = None) -> bool:
    """lsq_xnor_conv2d for a CHAIN of 1-bit layers: the activation scale from the row sums ``x_units`` a previous call's
    epilogue left (or ``xscales`` [1, N]), and / or the next layer's quantizer in this call's epilogue (``nxt``).  Returns
    False -- nothing launched -- when the geometry is outside the integer-MFMA kernel (the caller takes the unchained
    calls: same bits)."""
    act, slope = _act(relu, prelu, geom.O)
    m = geom.C * geom.H * geom.W
    nres = (res_pre is not None) + (res_post is not None)
    macs = y.numel() * geom.C * geom.KH * geom.KW * wscales.shape[0]
    extra = 0 if nxt is None else y.numel() // 8
    with _on(y), (_Timed('lsq_xnor_conv2d', geom.N * m // 8 + 4 * y.numel() * (1 + nres) + extra, macs,
                         f'C{geom.C}_H{geom.H}_s{geom.stride_h}', geom.N * m // 8 + 4 * y.numel()) if _timing is not None else _UNTIMED):
        code = lib().lsq_xnor_conv2d_chain(planes.data_ptr(), ptr(xscales), ptr(x_units), float(x_alpha), wbits.data_ptr(),
                                           wsum.data_ptr(), wscales.shape[0], wscales.data_ptr(), ptr(bias), ctypes.byref(geom),
                                           act, ptr(slope), ptr(res_pre), ptr(res_post),
                                           None if nxt is None else ctypes.byref(nxt), y.data_ptr(), stream_ptr(y.device))
    if code == E_UNSUPPORTED:
        return False
    check(code, 'lsq_xnor_conv2d_chain')
    return True


def signw_prepare_weight(wbits: torch.Tensor, planes: int, geom: ConvGeom) -> Optional[torch.Tensor]:
    """The bf16 operand image of lsq_signw_conv2d's 3x3 fast path for the sign planes ``wbits`` (once per eval
    session, next to pack_weight); None when the geometry has no fast path."""
    nbytes = lib().lsq_signw_weight_bytes(ctypes.byref(geom), planes)
    if nbytes <= 0:
        return None
    out = torch.empty((nbytes,), dtype=torch.uint8, device=wbits.device)
    with _on(wbits):
        check(lib().lsq_signw_prepare_weight(wbits.data_ptr(), planes, ctypes.byref(geom), out.data_ptr(),
                                             stream_ptr(wbits.device)), 'lsq_signw_prepare_weight')
    return out


def signw_conv2d(x: torch.Tensor, alpha: float, wbits: torch.Tensor, wscales: torch.Tensor,
                 bias: Optional[torch.Tensor], geom: ConvGeom, y: torch.Tensor, pre: Optional[tuple] = None,
                 relu: bool = False, res_pre: Optional[torch.Tensor] = None,
                 res_post: Optional[torch.Tensor] = None, prelu: Optional[torch.Tensor] = None,
                 wprep: Optional[torch.Tensor] = None) -> None:
    """``wprep``: signw_prepare_weight(wbits, ...) of the same weights and geometry (same result, 3x3 fast path)."""
    x = _f32c(x)
    if wprep is not None:              # (the image depends on channels, out-channels, taps and planes only: any batch / image size)
        want = lib().lsq_signw_weight_bytes(ctypes.byref(geom), wscales.shape[0])
        if wprep.dtype != torch.uint8 or wprep.numel() != want or wprep.device != x.device:
            raise ValueError(f'wprep: expected {want} bytes of signw_prepare_weight output on {x.device} for this geometry, '
                             f'got {wprep.numel()} x {wprep.dtype} on {wprep.device}')
    act, slope = _act(relu, prelu, geom.O)
    flops = 2 * 2 * y.numel() * (geom.C // geom.groups) * geom.KH * geom.KW * wscales.shape[0]   # hi + lo passes
    nres = (res_pre is not None) + (res_post is not None)
    with _on(x), _Timed('lsq_signw_conv2d', 4 * x.numel() + 4 * y.numel() * (1 + nres), flops, f'C{geom.C}_H{geom.H}_s{geom.stride_h}',
                         4 * x.numel() + 4 * y.numel()):     # fp32 input read + fp32 output written (+ residuals read)
        check(lib().lsq_signw_conv2d(x.data_ptr(), float(alpha), None if pre is None else pre[0].data_ptr(),
                                     None if pre is None else pre[1].data_ptr(), wbits.data_ptr(), ptr(wprep), wscales.shape[0],
                                     wscales.data_ptr(), ptr(bias), ctypes.byref(geom), act, ptr(slope), ptr(res_pre),
                                     ptr(res_post), y.data_ptr(), stream_ptr(x.device)), 'lsq_signw_conv2d')


def pool_bias_relu_nhwc(x: torch.Tensor, kernel: int, stride: int, pad: int, bias: Optional[torch.Tensor],
                        relu: bool) -> torch.Tensor:
    """``relu(max_pool2d(x) + bias)`` of a channels-last fp32 tensor ``x`` (logical shape [N, C, H, W]) as
    one kernel that writes a contiguous NCHW tensor."""
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last):
        raise LsqHipError('pool_bias_relu_nhwc needs a channels-last fp32 4-d tensor')
    n, c, h, w = x.shape
    ho, wo = (h + 2 * pad - kernel) // stride + 1, (w + 2 * pad - kernel) // stride + 1
    y = torch.empty((n, c, ho, wo), dtype=torch.float32, device=x.device)
    with _on(x), _Timed('lsq_pool_bias_relu_nhwc', 4 * x.numel() + 4 * y.numel(), 0):
        check(lib().lsq_pool_bias_relu_nhwc(x.data_ptr(), n, c, h, w, kernel, stride, pad,
                                            ptr(None if bias is None else _f32c(bias)), int(relu), y.data_ptr(),
                                            stream_ptr(x.device)), 'lsq_pool_bias_relu_nhwc')
    return y


_stem_guard = {}


def _stem_guard_state(device):
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _stem_guard.get(idx)
    if st is None:
        st = _stem_guard[idx] = {'flag': torch.zeros((1,), dtype=torch.int32, device=torch.device('cuda', idx)),
                                 'host': torch.zeros((1,), dtype=torch.int32).pin_memory(), 'event': None, 'tripped': False,
                                 'calls': 0}
    return st


def stem_overflow_tripped(device) -> bool:
    """True once a FINISHED stem_conv_pool(split=22) call on ``device`` has reported an operand outside the fp16 split's
    domain (|value| >= 65504 or NaN).  Never blocks: the kernel raises a STICKY device flag; its copy to pinned host
    memory rides on the launch stream after the first call and then after every 16th (a copy is a launch of its own:
    4 us per forward if made every time) and is looked at only when its event has completed -- so the report arrives
    up to 16 calls after the offending one (whose output holds inf / nan).  Callers switch to split 3 (any finite
    input) then."""
    st = _stem_guard_state(device)
    ev = st['event']
    if ev is not None and ev.query():
        st['event'] = None
        if int(st['host'][0]) != 0:
            st['tripped'] = True
    return st['tripped']


def stem_overflow_check(device) -> bool:
    """Blocking form of :func:`stem_overflow_tripped`: waits for the device and reads the flag itself -- for the end of an
    evaluation loop and in front of a graph capture, where a report that is 16 calls late would be too late."""
    st = _stem_guard_state(device)
    torch.cuda.synchronize(device)
    st['event'] = None
    if int(st['flag'].item()) != 0:
        st['tripped'] = True
    return st['tripped']


def stem_overflow_flag_raised(device) -> bool:
    """True while the DEVICE flag is up, i.e. a call since the last ``stem_overflow_reset`` saw an out-of-domain operand
    (``stem_overflow_check`` also reports a trip that was dealt with earlier).  Waits for the device."""
    st = _stem_guard_state(device)
    torch.cuda.synchronize(device)
    st['event'] = None
    raised = int(st['flag'].item()) != 0
    st['tripped'] = st['tripped'] or raised
    return raised


def stem_overflow_reset(device, keep_tripped: bool = False) -> None:
    """Forget an earlier report (after the caller has dealt with it); waits for the device.  ``keep_tripped``: lower the
    device flag but keep the host-side memory of it, so that callers stay on the bf16 split (``evaluate`` repeats a pass)."""
    torch.cuda.synchronize(device)
    st = _stem_guard_state(device)
    st['event'], st['tripped'], st['calls'] = None, bool(keep_tripped and st['tripped']), 0
    st['flag'].zero_()
    st['host'].zero_()


def stem_conv_pool(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, split: int = 3) -> torch.Tensor:
    """``max_pool2d(relu(conv2d(x, w, stride=2, padding=3) + bias), 3, 2, 1)`` for a 7x7 convolution 3 -> 64
    channels (batch norm already folded into ``w`` / ``bias``) as ONE kernel, NCHW fp32 in and out.  ``split``: how the
    fp32 operands are fed to the 16-bit matrix cores -- 3: three bf16 terms, six MFMA passes, fp32-class accuracy, any
    finite input; 2: two bf16 terms, three passes, ~2^-17 per product; 22: fp16 leading term + scaled fp16 remainder,
    three passes, fp32-class accuracy (2^-23 per product), operands below 65504 in magnitude (larger ones become
    inf / nan in the output, and the call reports them: ``stem_overflow_tripped``)."""
    x, w, bias = _f32c(x), _f32c(w), _f32c(bias)
    n, c, h, wd = x.shape
    if c != 3 or tuple(w.shape) != (64, 3, 7, 7) or wd % 2 or h < 8 or wd < 8 or x.data_ptr() % 8:
        raise LsqHipError('stem_conv_pool: 7x7 stride-2 convolution from 3 to 64 channels, even width, at least 8 x 8, 8-byte aligned')
    hc, wc = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    hp, wp = (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
    y = torch.empty((n, 64, hp, wp), dtype=torch.float32, device=x.device)
    flops = 2 * (6 if split == 3 else 3) * n * 64 * hc * wc * 147      # 16-bit MFMA passes issued
    # (no guard while a HIP graph is being captured: the event / pinned-copy bookkeeping is host state of ONE call;
    #  the warm-up forwards in front of a capture run with it)
    guard = _stem_guard_state(x.device) if split == 22 and not torch.cuda.is_current_stream_capturing() else None
    if guard is not None:
        stem_overflow_tripped(x.device)                                   # (collect a finished report before the flag is reused)
    with _on(x), _Timed('lsq_stem_conv_pool', 4 * x.numel() + 4 * y.numel(), flops):
        check(lib().lsq_stem_conv_pool(x.data_ptr(), n, h, wd, w.data_ptr(), bias.data_ptr(), int(split), y.data_ptr(),
                                       None if guard is None else guard['flag'].data_ptr(), stream_ptr(x.device)),
              'lsq_stem_conv_pool')
        if guard is not None:
            guard['calls'] += 1
        if guard is not None and guard['event'] is None and guard['calls'] % 16 == 1:
            guard['host'].copy_(guard['flag'], non_blocking=True)
            guard['event'] = torch.cuda.Event()
            guard['event'].record()
    return y


def pointwise_conv(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int) -> torch.Tensor:
    """``conv2d(x, w[:, :, None, None], bias, stride)`` for a 1x1 kernel (the projection shortcut, batch norm
    already folded), NCHW fp32, exact fp32 on the matrix cores; C and O multiples of 64."""
    x, w = _f32c(x), _f32c(w)
    n, c, h, wd = x.shape
    o = w.shape[0]
    y = torch.empty((n, o, (h - 1) // stride + 1, (wd - 1) // stride + 1), dtype=torch.float32, device=x.device)
    with _on(x), _Timed('lsq_pointwise_conv', 4 * (y.numel() // o) * c + 4 * y.numel(), 2 * y.numel() * c):
        check(lib().lsq_pointwise_conv(x.data_ptr(), n, c, h, wd, w.data_ptr(), ptr(None if bias is None else _f32c(bias)), o,
                                       int(stride), y.data_ptr(), stream_ptr(x.device)), 'lsq_pointwise_conv')
    return y


def quant_values(x: torch.Tensor, scales: Optional[torch.Tensor], alpha: float) -> torch.Tensor:
    """x_q = sum_i v_i b_i of the quantizer chain for rows x[r] (dim 0) and plane scales [k, rows] (None: the clamp
    alone) -- what the reference's quantizer_* functions return, on the device in one pass."""
    x = _f32c(x)
    rows, m = x.shape[0], x.numel() // max(x.shape[0], 1)
    k = 0 if scales is None else scales.shape[0]
    sc = None if scales is None else _f32c(scales)
    out = torch.empty_like(x)
    with _on(x), _Timed('lsq_quant_values', 8 * x.numel(), 0):
        check(lib().lsq_quant_values(x.data_ptr(), rows, m, k, ptr(sc), float(alpha), out.data_ptr(), stream_ptr(x.device)),
              'lsq_quant_values')
    return out


def ste_backward(x: torch.Tensor, grad_q: torch.Tensor, scales: Optional[torch.Tensor], alpha: float) -> torch.Tensor:
    """Gradient with respect to ``x`` of <grad_q, quantizer(clamp(x))> through the straight-through estimator
    (quant/binary/ste.py:51-66) and the clamp; rows = dim 0, plane scales [k, rows] (None: the clamp alone)."""
    x, grad_q = _f32c(x), _f32c(grad_q)
    if grad_q.shape != x.shape:
        raise ValueError(f'gradient of shape {tuple(grad_q.shape)} for an input of shape {tuple(x.shape)}')
    rows, m = x.shape[0], x.numel() // max(x.shape[0], 1)
    k = 0 if scales is None else scales.shape[0]
    sc = None if scales is None else _f32c(scales)
    out = torch.empty_like(x)
    with _on(x), _Timed('lsq_ste_backward', 12 * x.numel(), 0):
        check(lib().lsq_ste_backward(x.data_ptr(), grad_q.data_ptr(), rows, m, k, ptr(sc), float(alpha), out.data_ptr(),
                                     stream_ptr(x.device)), 'lsq_ste_backward')
    return out


# ---- the libraries beside liblsq_hip.so, one shared object per kernel family, each loaded on first use.  They are the entries
# of quant/_sublibs.py.  A new family is: an entry there (its prototypes are held against the header by
# tests/test_sublib_table_host.py), csrc/<dir>/Makefile that includes csrc/sublib.mk, include/lsq_hip_<dir>.h, and one line
# of public names below; __graft_entry__.build() makes and checks every entry of the table.
def _sublib_path(name: str) -> str:
    return os.path.join(_LIB_DIR, _sublibs.soname(_sublibs.BY_DIR[name]))


class _Handles(dict):
    """{dir of the entry: its loaded library}; a miss loads the library, which raises if it has not been built (no fallback,
    as ``lib()``)."""

    def __missing__(self, name):
        s = _sublibs.BY_DIR[name]
        handle = self[name] = _load(_sublib_path(name), 'csrc/' + name, s.prototypes, s.version_symbol, s.version,
                                    _sublibs.soname(s))
        return handle


_handles = _Handles()


def _sublib(name: str):
    """(loader, library_path, ABI version) of the entry ``name``: ``loader()`` is ``_handles[name]`` and no more, so that a
    warm call costs one dict lookup -- no lock, no Python frame."""
    return functools.partial(_handles.__getitem__, name), functools.partial(_sublib_path, name), _sublibs.BY_DIR[name].version


train_lib, train_library_path, TRAIN_ABI_VERSION = _sublib('train')
linear_lib, linear_library_path, LINEAR_ABI_VERSION = _sublib('linear')
linear_fp_lib, linear_fp_library_path, LINEAR_FP_ABI_VERSION = _sublib('linear_fp')
linear_train_lib, linear_train_library_path, LINEAR_TRAIN_ABI_VERSION = _sublib('linear_train')
linear_train_half_lib, linear_train_half_library_path, LINEAR_TRAIN_HALF_ABI_VERSION = _sublib('linear_train_half')
linear_wgrad_lib, linear_wgrad_library_path, LINEAR_WGRAD_ABI_VERSION = _sublib('linear_wgrad')
linear_half_lib, linear_half_library_path, LINEAR_HALF_ABI_VERSION = _sublib('linear_half')
linear_act_half_lib, linear_act_half_library_path, LINEAR_ACT_HALF_ABI_VERSION = _sublib('linear_act_half')
linear_act_solve_lib, linear_act_solve_library_path, LINEAR_ACT_SOLVE_ABI_VERSION = _sublib('linear_act_solve')
conv_act_half_lib, conv_act_half_library_path, CONV_ACT_HALF_ABI_VERSION = _sublib('conv_act_half')
conv_half_lib, conv_half_library_path, CONV_HALF_ABI_VERSION = _sublib('conv_half')
conv_train_lib, conv_train_library_path, CONV_TRAIN_ABI_VERSION = _sublib('conv_train')
conv_train_half_lib, conv_train_half_library_path, CONV_TRAIN_HALF_ABI_VERSION = _sublib('conv_train_half')
conv_proj_lib, conv_proj_library_path, CONV_PROJ_ABI_VERSION = _sublib('conv_proj')
conv_xnor_half_lib, conv_xnor_half_library_path, CONV_XNOR_HALF_ABI_VERSION = _sublib('conv_xnor_half')
train_half_lib, train_half_library_path, TRAIN_HALF_ABI_VERSION = _sublib('train_half')
linear_wgrad_half_lib, linear_wgrad_half_library_path, LINEAR_WGRAD_HALF_ABI_VERSION = _sublib('linear_wgrad_half')
conv_act_bn_half_lib, conv_act_bn_half_library_path, CONV_ACT_BN_HALF_ABI_VERSION = _sublib('conv_act_bn_half')
conv_proj_half_lib, conv_proj_half_library_path, CONV_PROJ_HALF_ABI_VERSION = _sublib('conv_proj_half')
conv_fused_half_lib, conv_fused_half_library_path, CONV_FUSED_HALF_ABI_VERSION = _sublib('conv_fused_half')
bn_train_lib, bn_train_library_path, BN_TRAIN_ABI_VERSION = _sublib('bn_train')

LINEAR_MAX_FEATURES = 1 << 22       # lsq_linear_xnor: F < 2^22 (exact fp32 integers)
LINEAR_MAX_OUTPUTS = 1 << 21        # lsq_linear_xnor: O < 2^21
LINEAR_WGRAD_MAX_SAMPLES = 65535    # lsq_linear_signx_wgrad: N <= 65535 (the limit of lsq_quant_values)
LINEAR_HALF_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}     # LSQ_DTYPE_*
CONV_DGRAD_HALF_MAX_SAMPLES = 65535    # lsq_signw_conv2d_dgrad_half with x: N <= 65535 (the limit of lsq_ste_backward)
LINEAR_DGRAD_HALF_MAX_SAMPLES = 65535  # lsq_linear_signw_dgrad_half with x: M / T <= 65535 (the same limit)


# ---- the training library (include/lsq_hip_train.h)
def wgrad(planes: torch.Tensor, kx: int, xscales: torch.Tensor, gy: torch.Tensor, geom: ConvGeom) -> torch.Tensor:
    """grad_wq [O, C, KH, KW] = conv2d_weight(x_q, grad_y) with x_q = sum_p xscales[p][n] (2 bit_p - 1) read from the
    activation planes ``planes`` (lsq_train_wgrad), on the current stream.  The split-K slabs live in a workspace cached
    per (device, stream) like the solver's (any content; kernels of one stream run in order)."""
    gy, xscales = _f32c(gy), _f32c(xscales)
    if planes.dtype != torch.int64 or not planes.is_contiguous():
        raise TypeError('activation planes are a contiguous int64 tensor')
    tl = train_lib()
    need = int(tl.lsq_train_wgrad_workspace_bytes(ctypes.byref(geom), int(kx)))
    ws = _stream_buffer('wgrad', need, gy.device) if need else None
    out = torch.empty((geom.O, geom.C, geom.KH, geom.KW), dtype=torch.float32, device=gy.device)
    ho, wo = out_hw(geom)
    with _on(gy), _Timed('lsq_train_wgrad', 4 * gy.numel() + 8 * kx * act_plane_words(geom) + 4 * out.numel(),
                         2 * geom.N * ho * wo * geom.O * geom.C * geom.KH * geom.KW):
        check(tl.lsq_train_wgrad(planes.data_ptr(), int(kx), xscales.data_ptr(), gy.data_ptr(), ctypes.byref(geom),
                                 out.data_ptr(), *_ws_args(ws), stream_ptr(gy.device)), 'lsq_train_wgrad')
    return out


# ---- the host-side operand checks of the entry points below (``what`` names one), in one order; the first that fails raises
def _check_half(what: str, name: str, t: torch.Tensor) -> None:
    """TypeError unless the 16-bit operand ``t`` is bf16 or fp16: the first check of every 16-bit entry point."""
    if t.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f'{what}: {name} must be a bfloat16 or float16 tensor, got {t.dtype}')


def _check_dtypes(what: str, fp32: dict, int64: Optional[dict] = None, int32: Optional[dict] = None) -> list:
    """TypeError for an operand of ``fp32`` / ``int64`` / ``int32`` = {name: tensor} of another dtype; returns the tensors."""
    groups = ((torch.float32, fp32), (torch.int64, int64 or {}), (torch.int32, int32 or {}))
    for dtype, named in groups:
        wrong = [name for name, t in named.items() if t.dtype != dtype]
        if wrong:
            raise TypeError(f'{what}: {", ".join(wrong)} must be {dtype} tensors')
    return [t for _, named in groups for t in named.values()]


def _check_placement(what: str, tensors: Sequence[torch.Tensor], problem=None) -> None:
    """ValueError ``'<what>: ...'`` for operands that are not ``contiguous``; then with the text ``problem()`` returns (the
    caller's own checks of sizes and of what must match, None: nothing to say); last -- so that every check above can be
    reached with CPU tensors, no library loaded -- for operands not all on the same ``cuda device``."""
    if any(not t.is_contiguous() for t in tensors):
        raise ValueError(f'{what}: operands must be contiguous')
    text = None if problem is None else problem()
    if text is not None:
        raise ValueError(f'{what}: {text}')
    dev = tensors[0].device
    if dev.type != 'cuda' or any(t.device != dev for t in tensors):
        raise ValueError(f'{what}: every operand on the same cuda device')


def _check_operands(what: str, fp32: dict, int64: Optional[dict] = None, int32: Optional[dict] = None,
                    half: Sequence[torch.Tensor] = (), problem=None) -> None:
    """``_check_dtypes``, then ``_check_placement`` of those operands and of ``half`` (the 16-bit ones: ``_check_half`` is the
    caller's, in front).  An entry point with a dtype check of its own in between calls the two itself."""
    _check_placement(what, [*half, *_check_dtypes(what, fp32, int64, int32)], problem)


def _check_linear(what: str, dims: dict, fp32: dict, int64: Optional[dict] = None, int32: Optional[dict] = None,
                  bad: bool = False, wplanes: Optional[tuple] = None, mismatch=None,
                  bias: Optional[torch.Tensor] = None) -> None:
    """``_check_operands`` (``bias`` is one of ``fp32``) with the linear entry points' own checks between contiguity and device:
      * ``bad sizes``: an entry of ``dims`` = {name: size} that is not positive, or ``bad`` (the caller's element counts
        against the dims);
      * operands that ``do not match``: ``wplanes`` = (wbits, wscales, F, O), the sign planes / scales [kw, O] lsq_pack_weight
        took and wrote for (O, F, 1, 1); then ``mismatch()``, the caller's own (what does not match, or None);
      * a ``bias`` of other than ``dims['O']`` elements."""
    if bias is not None:
        fp32 = dict(fp32, bias=bias)

    def problem():
        if bad or min(dims.values()) <= 0:
            return ('bad sizes ' + ' '.join(f'{name}={v}' for name, v in dims.items()) + ' for '
                    + ', '.join(f'{name} of {t.numel()}' for name, t in fp32.items()) + ' elements')
        if wplanes is not None:
            wbits, wscales, F, O = wplanes
            if wscales.dim() != 2 or wscales.shape[1] != O \
                    or wbits.numel() != wscales.shape[0] * ((F + 63) // 64) * ((O + 15) // 16 * 16):
                return 'weight planes / scales do not match (kw, F, O)'
        subject = None if mismatch is None else mismatch()
        if subject is not None:
            return f'{subject} do not match'
        if bias is not None and bias.numel() != dims['O']:
            return 'bias must have O elements'

    _check_operands(what, fp32, int64, int32, problem=problem)


def _geom_matches_gy(geom: ConvGeom, gy: torch.Tensor) -> bool:
    """Whether the forward geometry is a valid one and ``gy`` has the shape of its output."""
    return (min(geom.N, geom.C, geom.H, geom.W, geom.O, geom.KH, geom.KW, geom.groups, geom.stride_h, geom.stride_w,
                geom.dil_h, geom.dil_w) >= 1 and min(geom.pad_h, geom.pad_w) >= 0 and geom.C % geom.groups == 0
            and geom.O % geom.groups == 0 and tuple(gy.shape) == (geom.N, geom.O) + tuple(out_hw(geom)))


def _signw_plane_words(geom: ConvGeom) -> int:
    """int64 words of one sign-weight plane of ``geom``: KH * KW * ceil(C/g / 64) * g * ceil16(O/g)."""
    return geom.KH * geom.KW * ((geom.C // geom.groups + 63) // 64) * geom.groups * ((geom.O // geom.groups + 15) // 16 * 16)


# ---- the linear-layer library (include/lsq_hip_linear.h)
def linear_xnor(planes: torch.Tensor, kx: int, xscales: torch.Tensor, rows_per_scale: int, wbits: torch.Tensor,
                wsum: torch.Tensor, wscales: torch.Tensor, bias: Optional[torch.Tensor], M: int, F: int, O: int) -> torch.Tensor:
    """y [M, O] = F.linear(x_q, w_q, bias) from sign planes (lsq_linear_xnor): ``planes`` / ``xscales`` [kx, M / rows_per_scale]
    are what lsq_act_quant wrote for (N, rows_per_scale * F, 1, 1), ``wbits`` / ``wsum`` / ``wscales`` [kw, O] what
    lsq_pack_weight took and wrote for (O, F, 1, 1).  Bit for bit the 1x1 lsq_xnor_conv2d over (M, F, 1, 1)."""
    M, F, O, kx, t = int(M), int(F), int(O), int(kx), int(rows_per_scale)
    # (scales and a bias of another layout are copied, as the convolution's are)
    xscales, wscales, bias = _f32c(xscales), _f32c(wscales), None if bias is None else _f32c(bias)
    nw, dev = (F + 63) // 64, planes.device
    _check_linear('lsq_linear_xnor', {'M': M, 'F': F, 'O': O, 'kx': kx, 'rows_per_scale': t},
                  {'xscales': xscales, 'wscales': wscales}, {'planes': planes, 'wbits': wbits}, {'wsum': wsum},
                  bad=t > 0 and M % t != 0, wplanes=(wbits, wscales, F, O), bias=bias,
                  mismatch=lambda: ('activation planes / scales and (kx, M, F)'
                                    if planes.numel() < kx * M * nw or xscales.numel() != kx * (M // t) else
                                    'weight sums and (kw, O)' if wsum.numel() != wscales.shape[0] * O else None))
    kw = wscales.shape[0]
    y = torch.empty((M, O), dtype=torch.float32, device=dev)
    with _on(y), _Timed('lsq_linear_xnor', M * kx * nw * 8 + 4 * M * O, M * O * F * kx * kw):
        check(linear_lib().lsq_linear_xnor(planes.data_ptr(), kx, xscales.data_ptr(), t, wbits.data_ptr(), wsum.data_ptr(),
                                           kw, wscales.data_ptr(), ptr(bias), M, F, O, y.data_ptr(), stream_ptr(dev)),
              'lsq_linear_xnor')
    return y


# ---- the fp-activation linear-layer library (include/lsq_hip_linear_fp.h)
def linear_signw(x: torch.Tensor, alpha: float, wbits: torch.Tensor, wscales: torch.Tensor, bias: Optional[torch.Tensor],
                 M: int, F: int, O: int) -> torch.Tensor:
    """y [M, O] = F.linear(clamp(x), w_q, bias) for fp32 rows ``x`` [M, F] (any 4-byte-aligned data pointer) and the sign
    planes ``wbits`` / scales ``wscales`` [kw, O] lsq_pack_weight took and wrote for (O, F, 1, 1) (lsq_linear_signw);
    ``alpha`` is the symmetric clamp bound, negative for none."""
    M, F, O = int(M), int(F), int(O)
    _check_linear('lsq_linear_signw', {'M': M, 'F': F, 'O': O}, {'x': x, 'wscales': wscales}, {'wbits': wbits},
                  bad=x.numel() != M * F, wplanes=(wbits, wscales, F, O), bias=bias)
    kw, nw, opad, dev = wscales.shape[0], (F + 63) // 64, (O + 15) // 16 * 16, x.device
    y = torch.empty((M, O), dtype=torch.float32, device=dev)
    launches = (kw + 1) // 2                         # (y is read back by every launch after the first)
    with _on(y), _Timed('lsq_linear_signw', 4 * M * F * launches + 8 * kw * nw * opad + 4 * M * O * (2 * launches - 1),
                        2 * 2 * M * F * O * kw):       # bf16 FLOPs: the hi and the lo pass of every plane
        check(linear_fp_lib().lsq_linear_signw(x.data_ptr(), float(alpha), wbits.data_ptr(), kw, wscales.data_ptr(),
                                               ptr(bias), M, F, O, y.data_ptr(), stream_ptr(dev)), 'lsq_linear_signw')
    return y


# ---- the linear-layer training library (include/lsq_hip_linear_train.h)
def linear_signw_dgrad(gy: torch.Tensor, wbits: torch.Tensor, wscales: torch.Tensor, M: int, F: int, O: int) -> torch.Tensor:
    """gx [M, F] = gy @ w_q for fp32 gradient rows ``gy`` [M, O] (any 4-byte-aligned data pointer) and the sign planes
    ``wbits`` / scales ``wscales`` [kw, O] lsq_pack_weight took and wrote for (O, F, 1, 1) -- the forward's own operands
    (lsq_linear_signw_dgrad).  The transposed plane image lives in a workspace cached per (device, stream) like the
    solver's (rewritten by every call; kernels of one stream run in order)."""
    M, F, O = int(M), int(F), int(O)
    _check_linear('lsq_linear_signw_dgrad', {'M': M, 'F': F, 'O': O}, {'gy': gy, 'wscales': wscales}, {'wbits': wbits},
                  bad=gy.numel() != M * O, wplanes=(wbits, wscales, F, O))
    kw, nw, opad, dev = wscales.shape[0], (F + 63) // 64, (O + 15) // 16 * 16, gy.device
    tl = linear_train_lib()
    need = int(tl.lsq_linear_signw_dgrad_workspace_bytes(kw, F, O))
    ws = _stream_buffer('linear_dgrad', need, dev) if need else None
    gx = torch.empty((M, F), dtype=torch.float32, device=dev)
    with _on(gx), _Timed('lsq_linear_signw_dgrad', 4 * M * O * kw + 8 * kw * nw * opad + 2 * need + 4 * M * F,
                         2 * 2 * M * F * O * kw):       # bf16 FLOPs: the hi and the lo pass of every plane
        check(tl.lsq_linear_signw_dgrad(gy.data_ptr(), wbits.data_ptr(), kw, wscales.data_ptr(), M, F, O, gx.data_ptr(),
                                        *_ws_args(ws), stream_ptr(dev)), 'lsq_linear_signw_dgrad')
    return gx


# ---- the linear layer's 16-bit training library (include/lsq_hip_linear_train_half.h)
def linear_signw_dgrad_half(gy: torch.Tensor, wbits: torch.Tensor, wscales: torch.Tensor, M: int, F: int, O: int,
                            x: Optional[torch.Tensor] = None, xscales: Optional[torch.Tensor] = None, alpha: float = -1.0,
                            T: int = 1, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """grad_x [M, F] of the 16-bit train step in one launch (lsq_linear_signw_dgrad_half): gy @ w_q for the bf16 / fp16
    gradient rows ``gy`` [M, O] (any 2-byte-aligned data pointer) and the forward's own sign planes ``wbits`` / fp32 scales
    ``wscales`` [kw, O]; with ``x`` (the step's input [M, F] of gy's type, sample n owning rows n T .. n T + T - 1) the
    result then goes through the straight-through estimator of the activation quantizer -- ``xscales`` [kx, M / T] fp32, None
    for fp activations -- and the clamp ``alpha``, the bound ALREADY ROUNDED into the type (negative: none).  ``out_dtype``:
    gy.dtype (the default) or torch.float32; the 16-bit result is the fp32 one rounded once.  With ``x`` there are at most
    65535 samples (the limit of lsq_ste_backward).  The transposed plane image lives in the workspace of
    ``linear_signw_dgrad`` (the same size; cached per (device, stream), rewritten by every call; kernels of one stream run in
    order)."""
    what = 'lsq_linear_signw_dgrad_half'
    M, F, O, T = int(M), int(F), int(O), int(T)
    _check_half(what, 'gy', gy)
    out_dtype = gy.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, gy.dtype):
        raise TypeError(f'{what}: out_dtype must be torch.float32 or {gy.dtype}, got {out_dtype}')
    if x is not None and x.dtype != gy.dtype:
        raise TypeError(f'{what}: x must be of gy\'s type {gy.dtype}, got {x.dtype}')
    if xscales is not None and x is None:
        raise ValueError(f'{what}: xscales without x')
    dims = {'M': M, 'F': F, 'O': O} if x is None else {'M': M, 'F': F, 'O': O, 'T': T}

    def mismatch():
        if xscales is not None and (xscales.dim() != 2 or not 1 <= xscales.shape[0] <= MAX_PLANES
                                    or xscales.shape[1] != M // T):
            return 'activation scales and (kx, M / T)'
        if not 1 <= wscales.shape[0] <= MAX_PLANES:
            return f'{wscales.shape[0]} weight planes and 1 .. {MAX_PLANES}'
        if x is not None and M // T > LINEAR_DGRAD_HALF_MAX_SAMPLES:
            return f'{M // T} samples and the limit of {LINEAR_DGRAD_HALF_MAX_SAMPLES} with x'

    _check_linear(what, dims, {'wscales': wscales} if xscales is None else {'wscales': wscales, 'xscales': xscales},
                  {'wbits': wbits}, bad=gy.numel() != M * O or (x is not None and (x.numel() != M * F or (T > 0 and M % T != 0))),
                  wplanes=(wbits, wscales, F, O), mismatch=mismatch)
    dev = wscales.device
    halves = [gy] if x is None else [gy, x]
    if any(not t.is_contiguous() for t in halves):
        raise ValueError(f'{what}: operands must be contiguous')
    if any(t.device != dev for t in halves):
        raise ValueError(f'{what}: every operand on the same cuda device')
    kw, nw, opad = wscales.shape[0], (F + 63) // 64, (O + 15) // 16 * 16
    tl = linear_train_half_lib()
    need = int(tl.lsq_linear_signw_dgrad_half_workspace_bytes(kw, F, O))
    ws = _stream_buffer('linear_dgrad', need, dev) if need else None
    gx = torch.empty((M, F), dtype=out_dtype, device=dev)
    kx = 0 if xscales is None else xscales.shape[0]
    nbytes = 2 * M * O * kw + 8 * kw * nw * opad + 2 * need + gx.element_size() * M * F + (0 if x is None else 2 * M * F)
    with _on(gx), (_Timed(what, nbytes, 2 * 2 * M * F * O * kw) if _timing is not None else _UNTIMED):      # (hi and lo pass)
        check(tl.lsq_linear_signw_dgrad_half(gy.data_ptr(), LINEAR_HALF_DTYPES[gy.dtype], wbits.data_ptr(), kw,
                                             wscales.data_ptr(), M, F, O, ptr(x), T, kx, ptr(xscales), float(alpha),
                                             gx.data_ptr(), LINEAR_HALF_DTYPES[out_dtype], *_ws_args(ws), stream_ptr(dev)), what)
    return gx


# ---- the linear layer's weight-gradient library (include/lsq_hip_linear_wgrad.h)
def linear_signx_wgrad(gy: torch.Tensor, x: torch.Tensor, xscales: torch.Tensor, alpha: float, N: int, T: int, F: int,
                       O: int) -> torch.Tensor:
    """gwq [O, F] = gy^T @ x_q for fp32 gradient rows ``gy`` [N * T, O] (any 4-byte-aligned data pointer), the layer's input
    ``x`` [N * T, F] before the clamp and the per-(plane, sample) scales ``xscales`` [kx, N] of its quantizer
    (lsq_linear_signx_wgrad): x_q is never written, its signs go into a bit image in a workspace cached per (device, stream)
    like the solver's (rewritten by every call; kernels of one stream run in order)."""
    N, T, F, O = int(N), int(T), int(F), int(O)
    M = N * T
    _check_linear('lsq_linear_signx_wgrad', {'N': N, 'T': T, 'F': F, 'O': O}, {'gy': gy, 'x': x, 'xscales': xscales},
                  bad=gy.numel() != M * O or x.numel() != M * F,
                  mismatch=lambda: 'activation scales and (kx, N)' if xscales.dim() != 2 or xscales.shape[1] != N else None)
    kx, dev = xscales.shape[0], gy.device
    wl = linear_wgrad_lib()
    need = int(wl.lsq_linear_signx_wgrad_workspace_bytes(kx, N, T, F, O))
    ws = _stream_buffer('linear_wgrad', need, dev) if need else None
    gwq = torch.empty((O, F), dtype=torch.float32, device=dev)
    with _on(gwq), _Timed('lsq_linear_signx_wgrad', 4 * M * O + 4 * M * F + 4 * kx * N + 2 * need + 4 * O * F,
                          2 * 2 * M * F * O * kx):       # bf16 FLOPs: the hi and the lo pass of every plane
        check(wl.lsq_linear_signx_wgrad(gy.data_ptr(), x.data_ptr(), kx, xscales.data_ptr(), float(alpha), N, T, F, O,
                                        gwq.data_ptr(), *_ws_args(ws), stream_ptr(dev)), 'lsq_linear_signx_wgrad')
    return gwq


# ---- the linear layer's 16-bit weight-gradient library (include/lsq_hip_linear_wgrad_half.h)
def linear_signx_wgrad_half(gy: torch.Tensor, x: torch.Tensor, xscales: torch.Tensor, alpha: float, N: int, T: int, F: int,
                            O: int, weight: Optional[torch.Tensor] = None,
                            wscales: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[O, F] fp32 in one call (lsq_linear_signx_wgrad_half): gy^T @ x_q for the bf16 / fp16 gradient rows ``gy`` [N * T, O]
    and the layer's input ``x`` [N * T, F] of the same type before the clamp (any 2-byte-aligned data pointers), with the
    per-(plane, sample) scales ``xscales`` [kx, N] fp32 and the clamp ``alpha``, the bound ALREADY ROUNDED into the type
    (negative: none) -- bit for bit ``linear_signx_wgrad(gy.float(), x.float(), ...)``; with ``weight`` [O, F] fp32 and
    ``wscales`` [kw, O] fp32 the product goes through the straight-through estimator of the weight quantizer in the kernel's
    epilogue -- bit for bit ``ste_backward(weight, that, wscales, -1.0)``, the step's grad_w.  The sign image lives in the
    workspace of ``linear_signx_wgrad`` (the same size; cached per (device, stream), rewritten by every call; kernels of one
    stream run in order)."""
    what = 'lsq_linear_signx_wgrad_half'
    N, T, F, O = int(N), int(T), int(F), int(O)
    M = N * T
    _check_half(what, 'gy', gy)
    if x.dtype != gy.dtype:
        raise TypeError(f'{what}: x must be of gy\'s type {gy.dtype}, got {x.dtype}')
    if (weight is None) != (wscales is None):
        raise ValueError(f'{what}: weight and wscales go together')
    fp32 = {'xscales': xscales} if weight is None else {'xscales': xscales, 'weight': weight, 'wscales': wscales}

    def mismatch():
        if xscales.dim() != 2 or xscales.shape[1] != N:
            return 'activation scales and (kx, N)'
        if weight is not None and (wscales.dim() != 2 or wscales.shape[1] != O or not 1 <= wscales.shape[0] <= MAX_PLANES):
            return f'weight scales and (1 .. {MAX_PLANES}, O)'

    def problem():
        if min(N, T, F, O) <= 0 or gy.numel() != M * O or x.numel() != M * F or (weight is not None and weight.numel() != O * F):
            return (f'bad sizes N={N} T={T} F={F} O={O} for gy of {gy.numel()}, x of {x.numel()}'
                    + ('' if weight is None else f', weight of {weight.numel()}') + ' elements')
        subject = mismatch()
        return None if subject is None else f'{subject} do not match'

    _check_operands(what, fp32, half=(gy, x), problem=problem)
    kx, dev = xscales.shape[0], gy.device
    kw = 0 if weight is None else wscales.shape[0]
    wl = linear_wgrad_half_lib()
    need = int(wl.lsq_linear_signx_wgrad_half_workspace_bytes(kx, N, T, F, O))
    ws = _stream_buffer('linear_wgrad', need, dev) if need else None
    out = torch.empty((O, F), dtype=torch.float32, device=dev)
    nbytes = 2 * M * O + 2 * M * F + 4 * kx * N + 2 * need + 4 * O * F + (0 if weight is None else 4 * O * F + 4 * kw * O)
    with _on(out), (_Timed(what, nbytes, 2 * 2 * M * F * O * kx) if _timing is not None else _UNTIMED):     # (hi and lo pass)
        check(wl.lsq_linear_signx_wgrad_half(gy.data_ptr(), x.data_ptr(), LINEAR_HALF_DTYPES[gy.dtype], kx, xscales.data_ptr(),
                                             float(alpha), N, T, F, O, ptr(weight), kw, ptr(wscales), out.data_ptr(),
                                             *_ws_args(ws), stream_ptr(dev)), what)
    return out


# ---- the 16-bit-activation linear-layer library (include/lsq_hip_linear_half.h)
def linear_signw_half(x: torch.Tensor, alpha: float, wbits: torch.Tensor, wscales: torch.Tensor, bias: Optional[torch.Tensor],
                      M: int, F: int, O: int, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """y [M, O] = F.linear(x.clamp(-alpha, alpha), w_q, bias) for bf16 / fp16 rows ``x`` [M, F] (any 2-byte-aligned data
    pointer) and the sign planes ``wbits`` / fp32 scales ``wscales`` [kw, O] lsq_pack_weight took and wrote for (O, F, 1, 1)
    (lsq_linear_signw_half); ``alpha`` is the symmetric clamp bound (rounded into x's type, as Tensor.clamp rounds it),
    negative for none.  ``out_dtype``: x.dtype (the default) or torch.float32; the 16-bit result is the fp32 one rounded
    once.  The fp32 running sum of a 16-bit result of more than two planes lives in a workspace cached per
    (device, stream) like the solver's (rewritten by every call; kernels of one stream run in order)."""
    M, F, O = int(M), int(F), int(O)
    out_dtype = x.dtype if out_dtype is None else out_dtype
    _check_half('lsq_linear_signw_half', 'x', x)
    if out_dtype not in (torch.float32, x.dtype):
        raise TypeError(f'lsq_linear_signw_half: out_dtype must be torch.float32 or {x.dtype}, got {out_dtype}')
    _check_linear('lsq_linear_signw_half', {'M': M, 'F': F, 'O': O}, {'wscales': wscales}, {'wbits': wbits},
                  bad=x.numel() != M * F, wplanes=(wbits, wscales, F, O), bias=bias)
    dev = wscales.device
    if not x.is_contiguous():
        raise ValueError('lsq_linear_signw_half: operands must be contiguous')
    if x.device != dev:
        raise ValueError('lsq_linear_signw_half: every operand on the same cuda device')
    kw, nw, opad = wscales.shape[0], (F + 63) // 64, (O + 15) // 16 * 16
    hl = linear_half_lib()
    xdt, ydt = LINEAR_HALF_DTYPES[x.dtype], LINEAR_HALF_DTYPES[out_dtype]
    need = int(hl.lsq_linear_signw_half_workspace_bytes(M, O, kw, ydt))
    ws = _stream_buffer('linear_half', need, dev) if need else None
    y = torch.empty((M, O), dtype=out_dtype, device=dev)
    launches = (kw + 1) // 2                         # (the fp32 sum is read back by every launch after the first)
    with _on(y), _Timed('lsq_linear_signw_half', 2 * M * F * launches + 8 * kw * nw * opad + 8 * M * O * (launches - 1)
                        + y.element_size() * M * O, 2 * M * F * O * kw):      # 16-bit FLOPs: one pass per plane
        check(hl.lsq_linear_signw_half(x.data_ptr(), xdt, float(alpha), wbits.data_ptr(), kw, wscales.data_ptr(), ptr(bias),
                                       M, F, O, y.data_ptr(), ydt, *_ws_args(ws), stream_ptr(dev)), 'lsq_linear_signw_half')
    return y


# ---- the 16-bit activation quantizer library (include/lsq_hip_linear_act_half.h)
def linear_act_quant_half(x: torch.Tensor, scheme: int, k: int, alpha: float, planes: torch.Tensor, scales: torch.Tensor,
                          forced: Optional[torch.Tensor] = None) -> None:
    """Sign planes and scales of the bf16 / fp16 rows ``x`` [N, L] (any 2-byte-aligned data pointer) into ``planes`` (int64,
    at least k * N * ceil(L / 64) words: what lsq_act_quant writes for (N, L, 1, 1), every word written in full) and
    ``scales`` [k, N] fp32 (lsq_linear_act_quant_half).  ``alpha`` is the symmetric clamp bound ALREADY ROUNDED into x's type
    (as Tensor.clamp rounds it), negative for none; ``forced`` [k, N] fp32: scales to use instead of computing them --
    required for ls-2 / ls-T, whose free-running solve is lsq_act_quant's."""
    scheme, k = int(scheme), int(k)
    _check_half('lsq_linear_act_quant_half', 'x', x)
    fp32 = {'scales': scales} if forced is None else {'scales': scales, 'forced': forced}

    def problem():
        if x.dim() != 2 or x.numel() == 0 or k < 1:
            return f'bad sizes k={k} for x of shape {tuple(x.shape)}'
        N, L = x.shape
        if planes.numel() < k * N * ((L + 63) // 64) or any(tuple(t.shape) != (k, N) for t in fp32.values()):
            return 'activation planes / scales and (k, N, L) do not match'
        if scheme in (SCHEME_LS2, SCHEME_LST) and forced is None:
            return 'ls-2 / ls-T need forced scales (their solve reads fp32 rows: lsq_act_quant)'

    _check_operands('lsq_linear_act_quant_half', fp32, {'planes': planes}, half=[x], problem=problem)
    (N, L), dev = x.shape, x.device
    passes = 1 if forced is not None else k
    with _on(x), (_Timed('lsq_linear_act_quant_half', N * (2 * L * passes + k * ((L + 63) // 64) * 8), 0)
                  if _timing is not None else _UNTIMED):
        check(linear_act_half_lib().lsq_linear_act_quant_half(
            x.data_ptr(), LINEAR_HALF_DTYPES[x.dtype], N, L, scheme, k, float(alpha), ptr(forced), planes.data_ptr(),
            scales.data_ptr(), stream_ptr(dev)), 'lsq_linear_act_quant_half')


# ---- the 16-bit free-running ls-2 / ls-T quantizer library (include/lsq_hip_linear_act_solve.h)
def linear_act_quant_solve_half(x: torch.Tensor, scheme: int, skip: int, alpha: float, planes: torch.Tensor,
                                scales: torch.Tensor, status: Optional[torch.Tensor] = None) -> None:
    """Free-running ls-2 / ls-T on the bf16 / fp16 rows ``x`` [N, L] (any 2-byte-aligned data pointer): the optimal v1 of the
    sub-sample ``row[::skip]``, v2 and both sign planes into ``planes`` (int64, at least 2 * N * ceil(L / 64) words: what
    lsq_act_quant writes for (N, L, 1, 1), every word written in full), ``scales`` [2, N] fp32 and, where given, ``status`` [N]
    int32 (1 = the row had a candidate) (lsq_linear_act_quant_solve_half).  ``alpha`` is the symmetric clamp bound ALREADY
    ROUNDED into x's type (as Tensor.clamp rounds it), negative for none."""
    scheme, skip = int(scheme), int(skip)
    what = 'lsq_linear_act_quant_solve_half'
    if x.dtype not in (torch.bfloat16, torch.float16):        # (a ValueError, unlike _check_half's)
        raise ValueError(f'{what}: x must be a bfloat16 or float16 tensor, got {x.dtype}')
    if scheme not in (SCHEME_LS2, SCHEME_LST):
        raise ValueError(f'{what}: the scheme must be ls-2 or ls-T, got {scheme}')

    def problem():
        if x.dim() != 2 or x.numel() == 0 or skip < 1:
            return f'bad sizes skip={skip} for x of shape {tuple(x.shape)}'
        N, L = x.shape
        if (planes.numel() < 2 * N * ((L + 63) // 64) or tuple(scales.shape) != (2, N)
                or (status is not None and tuple(status.shape) != (N,))):
            return 'activation planes / scales / status and (N, L) do not match'

    _check_operands(what, {'scales': scales}, {'planes': planes}, {} if status is None else {'status': status}, half=[x],
                    problem=problem)
    (N, L), dev = x.shape, x.device
    with _on(x), (_Timed(what, N * (2 * L * 2 + 2 * ((L + 63) // 64) * 8), 0) if _timing is not None else _UNTIMED):
        check(linear_act_solve_lib().lsq_linear_act_quant_solve_half(
            x.data_ptr(), LINEAR_HALF_DTYPES[x.dtype], N, L, scheme, skip, float(alpha), planes.data_ptr(), scales.data_ptr(),
            ptr(status), stream_ptr(dev)), what)


# ---- the 16-bit activation quantizer of QuantConv2d (include/lsq_hip_conv_act_half.h)
def act_quant_half(x: torch.Tensor, geom: ConvGeom, scheme: int, k: int, skip: int, alpha: float, planes: torch.Tensor,
                   scales: torch.Tensor, forced: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> None:
    """Sign planes and scales of the bf16 / fp16 batch ``x`` [N, C, H, W] (contiguous, any 2-byte-aligned data pointer) of
    ``geom`` into ``planes`` (int64, at least k * act_plane_words(geom) words in lsq_act_quant's layout, halo zeroed by the
    caller, every interior word written in full), ``scales`` [k, N] fp32 and, where given, ``status`` [N] int32
    (lsq_act_quant_half).  ``alpha`` is the symmetric clamp bound ALREADY ROUNDED into x's type (as Tensor.clamp rounds it),
    negative for none; ``forced`` [k, N] fp32: scales to use instead of computing them; ``skip``: the sub-sampling stride of
    the free-running ls-2 / ls-T solve."""
    scheme, k, skip = int(scheme), int(k), int(skip)
    what = 'lsq_act_quant_half'
    _check_half(what, 'x', x)
    fp32 = {'scales': scales} if forced is None else {'scales': scales, 'forced': forced}

    def problem():
        if x.dim() != 4 or x.numel() == 0 or k < 1 or skip < 1:
            return f'bad sizes k={k}, skip={skip} for x of shape {tuple(x.shape)}'
        N, C, H, W = x.shape
        if (geom.N, geom.C, geom.H, geom.W) != (N, C, H, W) or geom.groups < 1 or C % geom.groups or min(geom.pad_h, geom.pad_w) < 0:
            return f'the geometry and x of shape {tuple(x.shape)} do not match'
        words = N * geom.groups * ((C // geom.groups + 63) // 64) * (H + 2 * geom.pad_h) * (W + 2 * geom.pad_w)
        if (planes.numel() < k * words or any(tuple(t.shape) != (k, N) for t in fp32.values())
                or (status is not None and tuple(status.shape) != (N,))):
            return 'activation planes / scales / status and (k, geometry) do not match'

    _check_operands(what, fp32, {'planes': planes}, {} if status is None else {'status': status}, half=[x], problem=problem)
    (N, C, H, W), dev = x.shape, x.device
    m = C * H * W
    passes = 1 if forced is not None and k <= 2 else (2 if scheme in (SCHEME_LS2, SCHEME_LST) and forced is None else k)
    with _on(x), (_Timed(what, N * (2 * m * passes + k * m // 8), 0, f'C{C}_H{H}') if _timing is not None else _UNTIMED):
        check(conv_act_half_lib().lsq_act_quant_half(
            x.data_ptr(), LINEAR_HALF_DTYPES[x.dtype], ctypes.byref(geom), scheme, k, skip, float(alpha), ptr(forced),
            planes.data_ptr(), scales.data_ptr(), ptr(status), stream_ptr(dev)), what)


# ---- the same quantizer with the eval batch norm in front of it folded into the read (include/lsq_hip_conv_act_bn_half.h)
def act_quant_bn_half(x: torch.Tensor, geom: ConvGeom, scheme: int, k: int, skip: int, alpha: float, planes: torch.Tensor,
                      scales: torch.Tensor, forced: Optional[torch.Tensor], pre: Tuple[torch.Tensor, torch.Tensor],
                      status: Optional[torch.Tensor] = None) -> None:
    """``act_quant_half`` on ``t = (x.float() * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).to(x.dtype)`` without ``t``
    in memory (lsq_act_quant_bn_half): ``pre = (scale, shift)``, fp32 contiguous tensors of C elements on x's device, the
    folded batch norm; every other argument is ``act_quant_half``'s.  Planes, scales and status are bit for bit what
    ``act_quant_half`` writes for ``t``."""
    scheme, k, skip = int(scheme), int(k), int(skip)
    what = 'lsq_act_quant_bn_half'
    _check_half(what, 'x', x)
    pre_scale, pre_shift = pre
    fp32 = {'scales': scales, 'pre_scale': pre_scale, 'pre_shift': pre_shift}
    if forced is not None:
        fp32['forced'] = forced

    def problem():
        if x.dim() != 4 or x.numel() == 0 or k < 1 or skip < 1:
            return f'bad sizes k={k}, skip={skip} for x of shape {tuple(x.shape)}'
        N, C, H, W = x.shape
        if (geom.N, geom.C, geom.H, geom.W) != (N, C, H, W) or geom.groups < 1 or C % geom.groups or min(geom.pad_h, geom.pad_w) < 0:
            return f'the geometry and x of shape {tuple(x.shape)} do not match'
        if pre_scale.numel() != C or pre_shift.numel() != C:
            return f'pre_scale / pre_shift and the {C} channels of x do not match'
        words = N * geom.groups * ((C // geom.groups + 63) // 64) * (H + 2 * geom.pad_h) * (W + 2 * geom.pad_w)
        if (planes.numel() < k * words or tuple(scales.shape) != (k, N) or (forced is not None and tuple(forced.shape) != (k, N))
                or (status is not None and tuple(status.shape) != (N,))):
            return 'activation planes / scales / status and (k, geometry) do not match'

    _check_operands(what, fp32, {'planes': planes}, {} if status is None else {'status': status}, half=[x], problem=problem)
    (N, C, H, W), dev = x.shape, x.device
    m = C * H * W
    passes = 1 if forced is not None and k <= 2 else (2 if scheme in (SCHEME_LS2, SCHEME_LST) and forced is None else k)
    with _on(x), (_Timed(what, N * (2 * m * passes + k * m // 8), 0, f'C{C}_H{H}') if _timing is not None else _UNTIMED):
        check(conv_act_bn_half_lib().lsq_act_quant_bn_half(
            x.data_ptr(), LINEAR_HALF_DTYPES[x.dtype], ctypes.byref(geom), scheme, k, skip, float(alpha), pre_scale.data_ptr(),
            pre_shift.data_ptr(), ptr(forced), planes.data_ptr(), scales.data_ptr(), ptr(status), stream_ptr(dev)), what)


# ---- the 16-bit-activation x sign-weight convolution (include/lsq_hip_conv_half.h)
def signw_conv2d_half_supported(geom: ConvGeom) -> bool:
    """Whether lsq_signw_conv2d_half computes ``geom`` (lsq_signw_conv2d_half_plan, host code: no device call): False for a
    geometry past the library's 32-bit index limits or with an empty output."""
    return conv_half_lib().lsq_signw_conv2d_half_plan(ctypes.byref(geom)) >= 0


def signw_conv2d_half(x: torch.Tensor, alpha: float, wbits: torch.Tensor, wscales: torch.Tensor, bias: Optional[torch.Tensor],
                      geom: ConvGeom, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """y [N, O, Ho, Wo] = F.conv2d(x.clamp(-alpha, alpha), w_q, bias, ...) for the bf16 / fp16 batch ``x`` [N, C, H, W] of
    ``geom`` (contiguous, any 2-byte-aligned data pointer) and the sign planes ``wbits`` / fp32 scales ``wscales`` [kw, O]
    lsq_pack_weight took and wrote for ``geom`` (lsq_signw_conv2d_half); ``alpha`` is the symmetric clamp bound ALREADY
    ROUNDED into x's type (as Tensor.clamp rounds it), negative for none.  ``out_dtype``: x.dtype (the default) or
    torch.float32; the 16-bit result is the fp32 one rounded once.  The fp32 running sum of a 16-bit result of more than one
    plane lives in a workspace cached per (device, stream) like the solver's (rewritten by every call; kernels of one stream
    run in order)."""
    what = 'lsq_signw_conv2d_half'
    out_dtype = x.dtype if out_dtype is None else out_dtype
    _check_half(what, 'x', x)
    if out_dtype not in (torch.float32, x.dtype):
        raise TypeError(f'{what}: out_dtype must be torch.float32 or {x.dtype}, got {out_dtype}')
    fp32 = _check_dtypes(what, {'wscales': wscales} if bias is None else {'wscales': wscales, 'bias': bias})
    if wbits.dtype != torch.int64:
        raise TypeError(f'{what}: wbits must be a torch.int64 tensor')

    def problem():
        if x.dim() != 4 or x.numel() == 0 or wscales.dim() != 2 or wscales.shape[0] < 1:
            return f'bad sizes: x of shape {tuple(x.shape)}, wscales of shape {tuple(wscales.shape)}'
        if (geom.N, geom.C, geom.H, geom.W) != tuple(x.shape) or min(geom.O, geom.KH, geom.KW, geom.groups) < 1 \
                or geom.C % geom.groups or geom.O % geom.groups:
            return f'the geometry and x of shape {tuple(x.shape)} do not match'
        if wscales.shape[1] != geom.O or wbits.numel() < wscales.shape[0] * _signw_plane_words(geom) \
                or (bias is not None and tuple(bias.shape) != (geom.O,)):
            return 'weight planes / scales / bias and (kw, geometry) do not match'

    _check_placement(what, [x, wbits, *fp32], problem)
    (N, C, H, W), kw, O, dev = x.shape, wscales.shape[0], geom.O, x.device
    ho, wo = out_hw(geom)
    if ho < 1 or wo < 1:
        raise ValueError(f'{what}: the geometry has an empty output')
    hl = conv_half_lib()
    xdt, ydt = LINEAR_HALF_DTYPES[x.dtype], LINEAR_HALF_DTYPES[out_dtype]
    need = int(hl.lsq_signw_conv2d_half_workspace_bytes(ctypes.byref(geom), kw, ydt))
    ws = _stream_buffer('conv_half', need, dev) if need else None
    y = torch.empty((N, O, ho, wo), dtype=out_dtype, device=dev)
    nbytes = 2 * x.numel() + 8 * y.numel() * (kw - 1) + y.element_size() * y.numel()    # (the fp32 sum is read back per plane)
    with _on(y), (_Timed(what, nbytes, 2 * y.numel() * (C // geom.groups) * geom.KH * geom.KW * kw,
                         f'C{C}_H{H}_s{geom.stride_h}') if _timing is not None else _UNTIMED):
        check(hl.lsq_signw_conv2d_half(x.data_ptr(), xdt, float(alpha), wbits.data_ptr(), kw, wscales.data_ptr(), ptr(bias),
                                       ctypes.byref(geom), y.data_ptr(), ydt, *_ws_args(ws), stream_ptr(dev)), what)
    return y


# ---- the same convolution with the folded batch norm in its read and the block epilogue in the launch
# (include/lsq_hip_conv_fused_half.h)
def signw_conv2d_fused_half(x: torch.Tensor, alpha: float, wbits: torch.Tensor, wscales: torch.Tensor,
                            bias: Optional[torch.Tensor], geom: ConvGeom, pre: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                            relu: bool = False, res_pre: Optional[torch.Tensor] = None, res_post: Optional[torch.Tensor] = None,
                            prelu: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """y [N, O, Ho, Wo] = act(conv(t.clamp(-alpha, alpha), w_q) + bias + res_pre) + res_post in one launch per weight plane
    (lsq_signw_conv2d_fused_half): the operands of ``signw_conv2d_half`` and
      * ``pre = (scale, shift)``, fp32 contiguous tensors of C elements, the folded batch norm:
        ``t = (x.float() * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).to(x.dtype)``, never in memory; ``None``: t = x;
      * ``relu`` / ``prelu`` (an nn.PReLU weight of 1 or O fp32 slopes), exclusive;
      * ``res_pre`` / ``res_post``: tensors of x's type and y's shape, read as they are.
    The result has the values of ``signw_conv2d_half(t, ..., out_dtype=torch.float32)`` followed by the epilogue in fp32,
    rounded once into ``out_dtype`` (x.dtype, the default, or torch.float32).  The fp32 running sum of a 16-bit result of more
    than one plane lives in a workspace cached per (device, stream), as ``signw_conv2d_half``'s does."""
    what = 'lsq_signw_conv2d_fused_half'
    out_dtype = x.dtype if out_dtype is None else out_dtype
    _check_half(what, 'x', x)
    if out_dtype not in (torch.float32, x.dtype):
        raise TypeError(f'{what}: out_dtype must be torch.float32 or {x.dtype}, got {out_dtype}')
    res = {name: t for name, t in (('res_pre', res_pre), ('res_post', res_post)) if t is not None}
    wrong = [name for name, t in res.items() if t.dtype != x.dtype]
    if wrong:
        raise TypeError(f'{what}: {", ".join(wrong)} must be {x.dtype} tensors')
    named = {'wscales': wscales}
    if bias is not None:
        named['bias'] = bias
    if pre is not None:
        named['pre_scale'], named['pre_shift'] = pre
    if prelu is not None:
        named['prelu'] = prelu
    fp32 = _check_dtypes(what, named)
    if wbits.dtype != torch.int64:
        raise TypeError(f'{what}: wbits must be a torch.int64 tensor')
    ho, wo = out_hw(geom)
    shape = (geom.N, geom.O, ho, wo)

    def problem():
        if x.dim() != 4 or x.numel() == 0 or wscales.dim() != 2 or wscales.shape[0] < 1:
            return f'bad sizes: x of shape {tuple(x.shape)}, wscales of shape {tuple(wscales.shape)}'
        if (geom.N, geom.C, geom.H, geom.W) != tuple(x.shape) or min(geom.O, geom.KH, geom.KW, geom.groups) < 1 \
                or geom.C % geom.groups or geom.O % geom.groups:
            return f'the geometry and x of shape {tuple(x.shape)} do not match'
        if wscales.shape[1] != geom.O or wbits.numel() < wscales.shape[0] * _signw_plane_words(geom) \
                or (bias is not None and tuple(bias.shape) != (geom.O,)):
            return 'weight planes / scales / bias and (kw, geometry) do not match'
        if pre is not None and (pre[0].numel() != geom.C or pre[1].numel() != geom.C):
            return f'pre_scale / pre_shift and the {geom.C} channels of x do not match'
        if prelu is not None and (relu or prelu.numel() not in (1, geom.O)):
            return f'prelu of {prelu.numel()} slopes on {geom.O} channels' + (' together with relu' if relu else '')
        for name, t in res.items():
            if tuple(t.shape) != shape:
                return f'{name} of shape {tuple(t.shape)} must have the shape of y, {shape}'

    _check_placement(what, [x, wbits, *res.values(), *fp32], problem)
    if ho < 1 or wo < 1:
        raise ValueError(f'{what}: the geometry has an empty output')
    act, slope = _act(relu, None if prelu is None else prelu.detach(), geom.O)
    (N, C, H, W), kw, dev = x.shape, wscales.shape[0], x.device
    fl = conv_fused_half_lib()
    xdt, ydt = LINEAR_HALF_DTYPES[x.dtype], LINEAR_HALF_DTYPES[out_dtype]
    need = int(fl.lsq_signw_conv2d_fused_half_workspace_bytes(ctypes.byref(geom), kw, ydt))
    ws = _stream_buffer('conv_fused_half', need, dev) if need else None
    y = torch.empty(shape, dtype=out_dtype, device=dev)
    # algorithmic bytes: x read per plane + the fp32 sum written and read back per plane before the last + every 16-bit
    # residual read + y written
    nbytes = 2 * x.numel() * kw + 8 * y.numel() * (kw - 1) + 2 * y.numel() * len(res) + y.element_size() * y.numel()
    with _on(y), (_Timed(what, nbytes, 2 * y.numel() * (C // geom.groups) * geom.KH * geom.KW * kw,
                         f'C{C}_H{H}_s{geom.stride_h}') if _timing is not None else _UNTIMED):
        check(fl.lsq_signw_conv2d_fused_half(
            x.data_ptr(), xdt, float(alpha), None if pre is None else pre[0].data_ptr(), None if pre is None else pre[1].data_ptr(),
            wbits.data_ptr(), kw, wscales.data_ptr(), ptr(bias), ctypes.byref(geom), act, ptr(slope), ptr(res_pre), ptr(res_post),
            y.data_ptr(), ydt, *_ws_args(ws), stream_ptr(dev)), what)
    return y


# ---- the XNOR convolution with a 16-bit epilogue (include/lsq_hip_conv_xnor_half.h)
def xnor_conv2d_half(planes: torch.Tensor, k: int, xscales: torch.Tensor, wbits: torch.Tensor, wsum: torch.Tensor,
                     wscales: torch.Tensor, bias: Optional[torch.Tensor], geom: ConvGeom, dtype: torch.dtype,
                     relu: bool = False, res_pre: Optional[torch.Tensor] = None, res_post: Optional[torch.Tensor] = None,
                     prelu: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [N, O, Ho, Wo] of ``dtype`` (bf16 / fp16) = act(conv + bias + res_pre) + res_post from the operands of
    ``xnor_conv2d`` (lsq_xnor_conv2d_half): the residuals are tensors of ``dtype`` and y's shape, read as they are; the fp32
    result is rounded once -- bit for bit ``xnor_conv2d`` on ``res.float()`` followed by ``.to(dtype)``.  The fp32 running sum
    of a call of more than one launch (kw * ceil(k / 2) > 1) lives in a workspace cached per (device, stream) like the
    solver's (rewritten by every call; kernels of one stream run in order)."""
    what = 'lsq_xnor_conv2d_half'
    k = int(k)
    if dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f'{what}: dtype must be torch.bfloat16 or torch.float16, got {dtype}')
    res = {name: t for name, t in (('res_pre', res_pre), ('res_post', res_post)) if t is not None}
    wrong = [name for name, t in res.items() if t.dtype != dtype]
    if wrong:
        raise TypeError(f'{what}: {", ".join(wrong)} must be {dtype} tensors')
    fp32 = {'xscales': xscales, 'wscales': wscales}
    if bias is not None:
        fp32['bias'] = bias
    if prelu is not None:
        fp32['prelu'] = prelu
    ho, wo = out_hw(geom)
    shape = (geom.N, geom.O, ho, wo)

    def problem():
        if k < 1 or wscales.dim() != 2 or wscales.shape[0] < 1 or min(shape) < 1:
            return f'bad sizes: k={k}, wscales of shape {tuple(wscales.shape)}, output {shape}'
        if tuple(xscales.shape) != (k, geom.N) or planes.numel() < k * geom.N * geom.groups * (
                (geom.C // max(geom.groups, 1) + 63) // 64) * (geom.H + 2 * geom.pad_h) * (geom.W + 2 * geom.pad_w):
            return 'activation planes / scales and (k, geometry) do not match'
        if wscales.shape[1] != geom.O or wbits.numel() < wscales.shape[0] * _signw_plane_words(geom) \
                or tuple(wsum.shape) != (wscales.shape[0], geom.O, geom.KH * geom.KW) \
                or (bias is not None and tuple(bias.shape) != (geom.O,)):
            return 'weight planes / sums / scales / bias and (kw, geometry) do not match'
        if prelu is not None and (relu or prelu.numel() not in (1, geom.O)):
            return f'prelu of {prelu.numel()} slopes on {geom.O} channels' + (' together with relu' if relu else '')
        for name, t in res.items():
            if tuple(t.shape) != shape:
                return f'{name} of shape {tuple(t.shape)} must have the shape of y, {shape}'

    _check_operands(what, fp32, {'planes': planes, 'wbits': wbits}, {'wsum': wsum}, half=list(res.values()), problem=problem)
    act, slope = _act(relu, None if prelu is None else prelu.detach(), geom.O)
    dev, kw = planes.device, wscales.shape[0]
    hl = conv_xnor_half_lib()
    lib()                                           # (liblsq_hip_conv_xnor_half.so links liblsq_hip.so: the same loaded object)
    need = int(hl.lsq_xnor_conv2d_half_workspace_bytes(ctypes.byref(geom), k, kw))
    ws = _stream_buffer('conv_xnor_half', need, dev) if need else None
    y = torch.empty(shape, dtype=dtype, device=dev)
    m = geom.C * geom.H * geom.W
    launches = kw * ((k + 1) // 2)
    macs = y.numel() * (geom.C // geom.groups) * geom.KH * geom.KW * k * kw
    # algorithmic bytes: planes read + 16-bit output written + every 16-bit residual read (+ the fp32 sum, written and read
    # back once per launch before the last)
    nbytes = geom.N * k * m // 8 + 2 * y.numel() * (1 + len(res)) + 8 * y.numel() * (launches - 1)
    with _on(y), (_Timed(what, nbytes, macs, f'C{geom.C}_H{geom.H}_s{geom.stride_h}') if _timing is not None else _UNTIMED):
        check(hl.lsq_xnor_conv2d_half(planes.data_ptr(), k, xscales.data_ptr(), wbits.data_ptr(), wsum.data_ptr(), kw,
                                      wscales.data_ptr(), ptr(bias), ctypes.byref(geom), act, ptr(slope), ptr(res_pre),
                                      ptr(res_post), LINEAR_HALF_DTYPES[dtype], y.data_ptr(), *_ws_args(ws), stream_ptr(dev)),
              what)
    return y


# ---- the projection shortcut on 16-bit tensors (include/lsq_hip_conv_proj_half.h)
def pointwise_conv_half(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int) -> torch.Tensor:
    """``pointwise_conv`` on a bf16 / fp16 ``x`` [N, C, H, W] (lsq_pointwise_conv_half): fp32 ``w`` [O, C] and ``bias``, fp32
    arithmetic, the result rounded once into ``x``'s type -- bit for bit ``pointwise_conv(x.float(), ...).to(x.dtype)``.  ``x``
    may be a contiguous view that starts anywhere in its storage (2-byte alignment)."""
    what = 'lsq_pointwise_conv_half'
    _check_half(what, 'x', x)
    fp32 = {'w': w} if bias is None else {'w': w, 'bias': bias}
    stride = int(stride)

    def problem():
        if x.dim() != 4 or w.dim() != 2 or min(*x.shape, *w.shape, stride) < 1:
            return f'bad sizes: x of shape {tuple(x.shape)}, w of shape {tuple(w.shape)}, stride {stride}'
        if w.shape[1] != x.shape[1] or (bias is not None and tuple(bias.shape) != (w.shape[0],)):
            return 'w [O, C] / bias [O] and x [N, C, H, W] do not match'

    _check_operands(what, fp32, half=[x], problem=problem)
    n, c, h, wd = x.shape
    o = w.shape[0]
    y = torch.empty((n, o, (h - 1) // stride + 1, (wd - 1) // stride + 1), dtype=x.dtype, device=x.device)
    hl = conv_proj_half_lib()
    lib()                                           # (liblsq_hip_conv_proj_half.so links liblsq_hip.so: the same loaded object)
    with _on(x), (_Timed(what, 2 * (y.numel() // o) * c + 2 * y.numel(), 2 * y.numel() * c) if _timing is not None else _UNTIMED):
        check(hl.lsq_pointwise_conv_half(x.data_ptr(), LINEAR_HALF_DTYPES[x.dtype], n, c, h, wd, w.data_ptr(), ptr(bias), o,
                                         stride, y.data_ptr(), stream_ptr(x.device)), what)
    return y


def xnor_conv2d_proj_half(planes: torch.Tensor, k: int, xscales: torch.Tensor, wbits: torch.Tensor, wsum: torch.Tensor,
                          wscales: torch.Tensor, bias: Optional[torch.Tensor], geom: ConvGeom, proj: tuple, dtype: torch.dtype,
                          relu: bool = False, res_pre: Optional[torch.Tensor] = None, res_post: Optional[torch.Tensor] = None,
                          prelu: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None):
    """``xnor_conv2d_half`` with the projection shortcut ``proj = (x of dtype, w [O, Cp] fp32, bias fp32 or None, stride, post)``
    computed in the epilogue's residual registers (lsq_xnor_conv2d_proj_half): ``post`` False = it plays ``res_pre``, True =
    ``res_post``; the other slot may hold a tensor of ``dtype``.  Returns ``(True, y)``, y [N, O, Ho, Wo] of ``dtype`` -- bit for
    bit ``xnor_conv2d_proj`` on the widened operands followed by ``.to(dtype)``, one rounding --, or ``(False, None)`` --
    nothing launched -- where the library refuses the call as unsupported.  The caller then runs ``pointwise_conv_half`` +
    ``xnor_conv2d_half``, which round the shortcut to ``dtype`` first: not the same bits (include/lsq_hip_conv_proj_half.h).
    ``y``: a contiguous tensor of ``dtype`` and the output's shape to write instead of a new one (2-byte alignment)."""
    what = 'lsq_xnor_conv2d_proj_half'
    k = int(k)
    if dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f'{what}: dtype must be torch.bfloat16 or torch.float16, got {dtype}')
    px, pw, pb, stride, post = proj
    half = {name: t for name, t in (('proj x', px), ('res_pre', res_pre), ('res_post', res_post), ('y', y)) if t is not None}
    wrong = [name for name, t in half.items() if not isinstance(t, torch.Tensor) or t.dtype != dtype]
    if wrong:
        raise TypeError(f'{what}: {", ".join(wrong)} must be {dtype} tensors')
    fp32 = {'xscales': xscales, 'wscales': wscales, 'proj w': pw}
    for name, t in (('bias', bias), ('prelu', prelu), ('proj bias', pb)):
        if t is not None:
            fp32[name] = t
    ho, wo = out_hw(geom)
    shape = (geom.N, geom.O, ho, wo)

    def problem():
        if k < 1 or wscales.dim() != 2 or wscales.shape[0] < 1 or min(shape) < 1 or px.dim() != 4 or pw.dim() != 2:
            return f'bad sizes: k={k}, wscales of shape {tuple(wscales.shape)}, output {shape}, proj x of shape {tuple(px.shape)}'
        if tuple(xscales.shape) != (k, geom.N) or planes.numel() < k * geom.N * geom.groups * (
                (geom.C // max(geom.groups, 1) + 63) // 64) * (geom.H + 2 * geom.pad_h) * (geom.W + 2 * geom.pad_w):
            return 'activation planes / scales and (k, geometry) do not match'
        if wscales.shape[1] != geom.O or wbits.numel() < wscales.shape[0] * _signw_plane_words(geom) \
                or tuple(wsum.shape) != (wscales.shape[0], geom.O, geom.KH * geom.KW) \
                or (bias is not None and tuple(bias.shape) != (geom.O,)):
            return 'weight planes / sums / scales / bias and (kw, geometry) do not match'
        if px.shape[0] != geom.N or tuple(pw.shape) != (geom.O, px.shape[1]) or (pb is not None and tuple(pb.shape) != (geom.O,)):
            return 'proj x [N, Cp, H, W], w [O, Cp] and bias [O] do not match the geometry'
        if prelu is not None and (relu or prelu.numel() not in (1, geom.O)):
            return f'prelu of {prelu.numel()} slopes on {geom.O} channels' + (' together with relu' if relu else '')
        for name, t in half.items():
            if name != 'proj x' and tuple(t.shape) != shape:
                return f'{name} of shape {tuple(t.shape)} must have the shape of y, {shape}'

    _check_operands(what, fp32, {'planes': planes, 'wbits': wbits}, {'wsum': wsum}, half=list(half.values()), problem=problem)
    act, slope = _act(relu, None if prelu is None else prelu.detach(), geom.O)
    dev, kw, cp = planes.device, wscales.shape[0], px.shape[1]
    pd = _sublibs.ProjHalf(px.data_ptr(), pw.data_ptr(), ptr(pb), cp, px.shape[2], px.shape[3], int(stride), int(bool(post)))
    hl = conv_proj_half_lib()
    lib()                                           # (liblsq_hip_conv_proj_half.so links liblsq_hip.so: the same loaded object)
    if y is None:
        y = torch.empty(shape, dtype=dtype, device=dev)
    m = geom.C * geom.H * geom.W
    nres = (res_pre is not None) + (res_post is not None)
    macs = y.numel() * (geom.C // geom.groups) * geom.KH * geom.KW * k * kw
    # algorithmic bytes: planes read + 16-bit output written + every 16-bit residual tensor read + the projection's gathered
    # input (one 2-byte value per output pixel and input channel)
    nbytes = geom.N * k * m // 8 + 2 * y.numel() * (1 + nres) + 2 * (y.numel() // geom.O) * cp
    with _on(y), (_Timed(what, nbytes, macs, f'C{geom.C}_H{geom.H}_s{geom.stride_h}') if _timing is not None else _UNTIMED):
        code = hl.lsq_xnor_conv2d_proj_half(planes.data_ptr(), k, xscales.data_ptr(), wbits.data_ptr(), wsum.data_ptr(), kw,
                                            wscales.data_ptr(), ptr(bias), ctypes.byref(geom), act, ptr(slope), ptr(res_pre),
                                            ptr(res_post), ctypes.byref(pd), LINEAR_HALF_DTYPES[dtype], y.data_ptr(),
                                            stream_ptr(dev))
    if code == E_UNSUPPORTED:
        return False, None
    check(code, what)
    return True, y


# ---- the convolution layer's training library (include/lsq_hip_conv_train.h)
def signw_conv2d_dgrad_plan(geom: ConvGeom) -> Optional[ConvDgradPlan]:
    """The plan of lsq_signw_conv2d_dgrad for the forward geometry ``geom`` (host code: no device call), None where the
    call would refuse it."""
    plan = ConvDgradPlan()
    return plan if conv_train_lib().lsq_signw_conv2d_dgrad_plan(ctypes.byref(geom), ctypes.byref(plan)) == 0 else None


def signw_conv2d_dgrad_supported(geom: ConvGeom) -> bool:
    """Whether lsq_signw_conv2d_dgrad computes the forward geometry ``geom``: False past the library's 32-bit index and grid
    limits or with an empty output."""
    return signw_conv2d_dgrad_plan(geom) is not None


def signw_conv2d_dgrad(gy: torch.Tensor, wbits: torch.Tensor, wscales: torch.Tensor, geom: ConvGeom) -> torch.Tensor:
    """grad_xq [N, C, H, W] = conv2d_input(w_q, gy) for the fp32 output gradient ``gy`` [N, O, Ho, Wo] of the FORWARD geometry
    ``geom`` and the sign planes ``wbits`` / scales ``wscales`` [kw, O] lsq_pack_weight took and wrote for ``geom`` -- the
    forward's own operands (lsq_signw_conv2d_dgrad).  The transposed plane image lives in a workspace cached per
    (device, stream) like the solver's (rewritten by every call; kernels of one stream run in order)."""
    what = 'lsq_signw_conv2d_dgrad'
    _check_dtypes(what, {'gy': gy, 'wscales': wscales})
    if wbits.dtype != torch.int64:
        raise TypeError(f'{what}: wbits must be a torch.int64 tensor')

    def problem():
        if gy.dim() != 4 or gy.numel() == 0 or wscales.dim() != 2 or not 1 <= wscales.shape[0] <= MAX_PLANES:
            return f'bad sizes: gy of shape {tuple(gy.shape)}, wscales of shape {tuple(wscales.shape)}'
        if not _geom_matches_gy(geom, gy):
            return f'the geometry and gy of shape {tuple(gy.shape)} do not match'
        if wscales.shape[1] != geom.O or wbits.numel() != wscales.shape[0] * _signw_plane_words(geom):
            return 'weight planes / scales and (kw, geometry) do not match'

    _check_placement(what, [gy, wbits, wscales], problem)
    kw, C, words, dev = wscales.shape[0], geom.C, _signw_plane_words(geom), gy.device
    tl = conv_train_lib()
    need = int(tl.lsq_signw_conv2d_dgrad_workspace_bytes(ctypes.byref(geom), kw))
    ws = _stream_buffer('conv_dgrad', need, dev) if need else None
    gx = torch.empty((geom.N, C, geom.H, geom.W), dtype=torch.float32, device=dev)
    with _on(gx), (_Timed(what, 4 * gy.numel() + 8 * kw * words + 2 * need + 4 * gx.numel(),
                          2 * 2 * gy.numel() * (C // geom.groups) * geom.KH * geom.KW * kw,       # (hi and lo pass)
                          f'C{C}_H{geom.H}_s{geom.stride_h}') if _timing is not None else _UNTIMED):
        check(tl.lsq_signw_conv2d_dgrad(gy.data_ptr(), wbits.data_ptr(), kw, wscales.data_ptr(), ctypes.byref(geom),
                                        gx.data_ptr(), *_ws_args(ws), stream_ptr(dev)), what)
    return gx


# ---- the convolution layer's 16-bit training library (include/lsq_hip_conv_train_half.h)
def signw_conv2d_dgrad_half_plan(geom: ConvGeom) -> Optional[ConvDgradPlan]:
    """The plan of lsq_signw_conv2d_dgrad_half for the forward geometry ``geom`` (host code: no device call), None where the
    call would refuse it: for every geometry what ``signw_conv2d_dgrad_plan`` returns."""
    plan = ConvDgradPlan()
    return plan if conv_train_half_lib().lsq_signw_conv2d_dgrad_half_plan(ctypes.byref(geom), ctypes.byref(plan)) == 0 else None


def signw_conv2d_dgrad_half_supported(geom: ConvGeom) -> bool:
    """Whether lsq_signw_conv2d_dgrad_half computes the forward geometry ``geom``: False past the library's 32-bit index and
    grid limits or with an empty output."""
    return signw_conv2d_dgrad_half_plan(geom) is not None


def signw_conv2d_dgrad_half(gy: torch.Tensor, wbits: torch.Tensor, wscales: torch.Tensor, geom: ConvGeom,
                            x: Optional[torch.Tensor] = None, xscales: Optional[torch.Tensor] = None, alpha: float = -1.0,
                            out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """grad_x [N, C, H, W] of the 16-bit train step in one launch (lsq_signw_conv2d_dgrad_half): conv2d_input(w_q, gy) for the
    bf16 / fp16 output gradient ``gy`` [N, O, Ho, Wo] of the FORWARD geometry ``geom`` (contiguous, any 2-byte-aligned data
    pointer) and the forward's own sign planes ``wbits`` / fp32 scales ``wscales`` [kw, O]; with ``x`` (the step's input
    [N, C, H, W] of gy's type) the result then goes through the straight-through estimator of the activation quantizer --
    ``xscales`` [kx, N] fp32, None for fp activations -- and the clamp ``alpha``, the bound ALREADY ROUNDED into the type
    (negative: none).  ``out_dtype``: gy.dtype (the default) or torch.float32; the 16-bit result is the fp32 one rounded
    once.  With ``x`` the batch is at most 65535 samples (the limit of lsq_ste_backward).  The transposed plane image lives
    in a workspace cached per (device, stream) like the solver's (rewritten by every call; kernels of one stream run in
    order)."""
    what = 'lsq_signw_conv2d_dgrad_half'
    _check_half(what, 'gy', gy)
    out_dtype = gy.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, gy.dtype):
        raise TypeError(f'{what}: out_dtype must be torch.float32 or {gy.dtype}, got {out_dtype}')
    if x is not None and x.dtype != gy.dtype:
        raise TypeError(f'{what}: x must be of gy\'s type {gy.dtype}, got {x.dtype}')
    fp32 = _check_dtypes(what, {'wscales': wscales} if xscales is None else {'wscales': wscales, 'xscales': xscales})
    if wbits.dtype != torch.int64:
        raise TypeError(f'{what}: wbits must be a torch.int64 tensor')
    if xscales is not None and x is None:
        raise ValueError(f'{what}: xscales without x')

    def problem():
        if gy.dim() != 4 or gy.numel() == 0 or wscales.dim() != 2 or not 1 <= wscales.shape[0] <= MAX_PLANES:
            return f'bad sizes: gy of shape {tuple(gy.shape)}, wscales of shape {tuple(wscales.shape)}'
        if xscales is not None and (xscales.dim() != 2 or not 1 <= xscales.shape[0] <= MAX_PLANES):
            return f'bad sizes: xscales of shape {tuple(xscales.shape)}'
        if not _geom_matches_gy(geom, gy):
            return f'the geometry and gy of shape {tuple(gy.shape)} do not match'
        if wscales.shape[1] != geom.O or wbits.numel() != wscales.shape[0] * _signw_plane_words(geom):
            return 'weight planes / scales and (kw, geometry) do not match'
        if x is not None and tuple(x.shape) != (geom.N, geom.C, geom.H, geom.W):
            return f'the geometry and x of shape {tuple(x.shape)} do not match'
        if xscales is not None and xscales.shape[1] != geom.N:
            return 'activation scales and (kx, geometry) do not match'
        if x is not None and geom.N > CONV_DGRAD_HALF_MAX_SAMPLES:
            return f'at most {CONV_DGRAD_HALF_MAX_SAMPLES} samples with x, got {geom.N}'

    _check_placement(what, [gy, wbits, *fp32] + ([] if x is None else [x]), problem)
    kw, C, words, dev = wscales.shape[0], geom.C, _signw_plane_words(geom), gy.device
    tl = conv_train_half_lib()
    need = int(tl.lsq_signw_conv2d_dgrad_half_workspace_bytes(ctypes.byref(geom), kw))
    ws = _stream_buffer('conv_dgrad_half', need, dev) if need else None
    gx = torch.empty((geom.N, C, geom.H, geom.W), dtype=out_dtype, device=dev)
    kx = 0 if xscales is None else xscales.shape[0]
    nbytes = 2 * gy.numel() + 8 * kw * words + 2 * need + gx.element_size() * gx.numel() + (0 if x is None else 2 * x.numel())
    with _on(gx), (_Timed(what, nbytes, 2 * 2 * gy.numel() * (C // geom.groups) * geom.KH * geom.KW * kw,       # (hi and lo pass)
                          f'C{C}_H{geom.H}_s{geom.stride_h}') if _timing is not None else _UNTIMED):
        check(tl.lsq_signw_conv2d_dgrad_half(gy.data_ptr(), LINEAR_HALF_DTYPES[gy.dtype], wbits.data_ptr(), kw,
                                             wscales.data_ptr(), ctypes.byref(geom), ptr(x), kx, ptr(xscales), float(alpha),
                                             gx.data_ptr(), LINEAR_HALF_DTYPES[out_dtype], *_ws_args(ws), stream_ptr(dev)), what)
    return gx


# ---- the convolution's 16-bit weight / bias gradient (include/lsq_hip_train_half.h)
def wgrad_half(planes: torch.Tensor, kx: int, xscales: torch.Tensor, gy: torch.Tensor, geom: ConvGeom, bias: bool = False):
    """(grad_wq [O, C, KH, KW] fp32, grad_b [O] fp32 or None) of the 16-bit train step in one call (lsq_train_wgrad_half):
    ``wgrad`` for the bf16 / fp16 output gradient ``gy`` [N, O, Ho, Wo] read as it is (contiguous, any 2-byte-aligned data
    pointer) -- x_q = sum_p xscales[p][n] (2 bit_p - 1) from the activation planes ``planes`` of ``geom`` and the fp32 scales
    ``xscales`` [kx, N] -- and with ``bias`` the sum of gy over (n, ho, wo) from the same pass.  The split-K partial sums live
    in a workspace cached per (device, stream) like the solver's (any content; kernels of one stream run in order)."""
    what = 'lsq_train_wgrad_half'
    kx = int(kx)
    _check_half(what, 'gy', gy)
    _check_dtypes(what, {'xscales': xscales}, {'planes': planes})

    def problem():
        if gy.dim() != 4 or gy.numel() == 0 or not 1 <= kx <= MAX_PLANES:
            return f'bad sizes: gy of shape {tuple(gy.shape)}, kx={kx}'
        if not _geom_matches_gy(geom, gy):
            return f'the geometry and gy of shape {tuple(gy.shape)} do not match'
        if tuple(xscales.shape) != (kx, geom.N) or planes.numel() < kx * geom.N * geom.groups * (
                (geom.C // geom.groups + 63) // 64) * (geom.H + 2 * geom.pad_h) * (geom.W + 2 * geom.pad_w):
            return 'activation planes / scales and (kx, geometry) do not match'

    _check_placement(what, [gy, xscales, planes], problem)
    dev = gy.device
    tl = train_half_lib()
    need = int(tl.lsq_train_wgrad_half_workspace_bytes(ctypes.byref(geom), kx, int(bool(bias))))
    ws = _stream_buffer('wgrad_half', need, dev) if need else None
    gwq = torch.empty((geom.O, geom.C, geom.KH, geom.KW), dtype=torch.float32, device=dev)
    gb = torch.empty((geom.O,), dtype=torch.float32, device=dev) if bias else None
    with _on(gy), (_Timed(what, 2 * gy.numel() + 8 * kx * act_plane_words(geom) + 4 * gwq.numel() + (4 * geom.O if bias else 0),
                          2 * gy.numel() * geom.C * geom.KH * geom.KW, f'C{geom.C}_H{geom.H}_s{geom.stride_h}')
                   if _timing is not None else _UNTIMED):
        check(tl.lsq_train_wgrad_half(planes.data_ptr(), kx, xscales.data_ptr(), gy.data_ptr(), LINEAR_HALF_DTYPES[gy.dtype],
                                      ctypes.byref(geom), gwq.data_ptr(), ptr(gb), *_ws_args(ws), stream_ptr(dev)), what)
    return gwq, gb


# ---- the train-mode batch norm in front of a quantized convolution (include/lsq_hip_bn_train.h)
BN_TRAIN_MAX = 65535          # lsq_bn_train_*: N, C <= 65535


def _check_bn(what: str, x: torch.Tensor, vectors: dict, like: Optional[dict] = None, scales: Optional[torch.Tensor] = None,
              k: int = 0) -> tuple:
    """The operand checks of the bn_train entry points: fp32, contiguous, a 4-d ``x`` within the limits, ``vectors`` of C elements
    (None entries are optional operands left out), ``like`` of x's shape, plane scales [k, N]; returns (N, C, H, W)."""
    vectors = {name: t for name, t in vectors.items() if t is not None}
    fp32 = dict({'x': x}, **vectors, **(like or {}), **({} if scales is None else {'xscales': scales}))

    def problem():
        if x.dim() != 4 or x.numel() == 0 or not 0 <= k <= MAX_PLANES:
            return f'bad sizes: x of shape {tuple(x.shape)}, k={k}'
        if x.shape[0] > BN_TRAIN_MAX or x.shape[1] > BN_TRAIN_MAX:
            return f'N, C <= {BN_TRAIN_MAX}: x of shape {tuple(x.shape)}'
        wrong = [name for name, t in vectors.items() if t.numel() != x.shape[1]]
        if wrong:
            return f'{", ".join(wrong)} must have C = {x.shape[1]} elements'
        wrong = [name for name, t in (like or {}).items() if t.shape != x.shape]
        if wrong:
            return f'{", ".join(wrong)} must have the shape of x'
        if (k > 0) != (scales is not None) or (scales is not None and tuple(scales.shape) != (k, x.shape[0])):
            return 'plane scales must be [k, N]'

    _check_operands(what, fp32, problem=problem)
    return tuple(x.shape)


def bn_train_slabs(n: int, c: int, h: int, w: int) -> int:
    """Slabs of samples per channel in the two reductions of this library for x [n, c, h, w] (from the workspace size: one
    fp64 pair per channel and slab)."""
    return int(bn_train_lib().lsq_bn_train_workspace_bytes(n, c, h, w)) // (16 * c)


def bn_train_stats(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float,
                   momentum: Optional[float], running_mean: Optional[torch.Tensor] = None,
                   running_var: Optional[torch.Tensor] = None, batch_count: int = 1):
    """(mean, var, invstd, scale, shift), each [C] fp32, of the train-mode batch norm of x [N, C, H, W] (lsq_bn_train_stats): the
    batch mean and biased variance, 1 / sqrt(var + eps), scale = gamma invstd and shift = beta - mean scale.  ``running_mean`` /
    ``running_var`` are updated in place as nn.BatchNorm2d does (``momentum`` None: the cumulative average over ``batch_count``
    batches, this one included).  x is read once; the per-slab partial sums live in a workspace cached per (device, stream)."""
    what = 'lsq_bn_train_stats'
    n, c, h, w = _check_bn(what, x, {'gamma': gamma, 'beta': beta, 'running_mean': running_mean, 'running_var': running_var})
    if (running_mean is None) != (running_var is None):
        raise ValueError(f'{what}: running_mean and running_var come together')
    if n * h * w < 2:
        raise ValueError(f'{what}: expected more than 1 value per channel, got x of shape {tuple(x.shape)}')
    bl = bn_train_lib()
    out = torch.empty((5, c), dtype=torch.float32, device=x.device)
    ws = _stream_buffer('bn_train', int(bl.lsq_bn_train_workspace_bytes(n, c, h, w)), x.device)
    with _on(x), (_Timed(what, 4 * x.numel(), 0, f'C{c}_H{h}') if _timing is not None else _UNTIMED):
        check(bl.lsq_bn_train_stats(x.data_ptr(), n, c, h, w, ptr(gamma), ptr(beta), float(eps),
                                    -1.0 if momentum is None else float(momentum), int(batch_count), ptr(running_mean),
                                    ptr(running_var), *(out[i].data_ptr() for i in range(5)), *_ws_args(ws),
                                    stream_ptr(x.device)), what)
    return out[0], out[1], out[2], out[3], out[4]


def bn_apply(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """y = fmaf(x, scale[c], shift[c]) (lsq_bn_apply): the tensor the quantizers see behind ``pre=(scale, shift)``."""
    what = 'lsq_bn_apply'
    n, c, h, w = _check_bn(what, x, {'scale': scale, 'shift': shift})
    y = torch.empty_like(x)
    with _on(x), (_Timed(what, 8 * x.numel(), 0, f'C{c}_H{h}') if _timing is not None else _UNTIMED):
        check(bn_train_lib().lsq_bn_apply(x.data_ptr(), n, c, h, w, scale.data_ptr(), shift.data_ptr(), y.data_ptr(),
                                          stream_ptr(x.device)), what)
    return y


def quant_values_bn(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, scales: Optional[torch.Tensor],
                    alpha: float) -> torch.Tensor:
    """``quant_values(bn_apply(x, scale, shift), scales, alpha)`` in one pass, bit for bit (lsq_quant_values_bn)."""
    what = 'lsq_quant_values_bn'
    k = 0 if scales is None else int(scales.shape[0])
    n, c, h, w = _check_bn(what, x, {'scale': scale, 'shift': shift}, scales=scales, k=k)
    out = torch.empty_like(x)
    with _on(x), (_Timed(what, 8 * x.numel(), 0, f'C{c}_H{h}') if _timing is not None else _UNTIMED):
        check(bn_train_lib().lsq_quant_values_bn(x.data_ptr(), n, c, h, w, scale.data_ptr(), shift.data_ptr(), k, ptr(scales),
                                                 float(alpha), out.data_ptr(), stream_ptr(x.device)), what)
    return out


def bn_ste_backward(x: torch.Tensor, grad_q: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, mean: torch.Tensor,
                    invstd: torch.Tensor, scales: Optional[torch.Tensor], alpha: float):
    """(grad_x, grad_gamma, grad_beta) of quantizer(bn(x)) for the gradient ``grad_q`` with respect to the quantizer's value
    (lsq_bn_ste_backward): g = ``ste_backward(bn_apply(x), grad_q, scales, alpha)`` recomputed in both passes and never stored,
    grad_beta = sum g, grad_gamma = sum g x^ and grad_x = scale (g - grad_beta / m - x^ grad_gamma / m)."""
    what = 'lsq_bn_ste_backward'
    k = 0 if scales is None else int(scales.shape[0])
    n, c, h, w = _check_bn(what, x, {'scale': scale, 'shift': shift, 'mean': mean, 'invstd': invstd}, {'grad_q': grad_q},
                           scales, k)
    bl = bn_train_lib()
    gx = torch.empty_like(x)
    gvec = torch.empty((2, c), dtype=torch.float32, device=x.device)
    ws = _stream_buffer('bn_ste_backward', int(bl.lsq_bn_ste_backward_workspace_bytes(n, c, h, w)), x.device)
    with _on(x), (_Timed(what, 20 * x.numel(), 0, f'C{c}_H{h}') if _timing is not None else _UNTIMED):
        check(bl.lsq_bn_ste_backward(x.data_ptr(), grad_q.data_ptr(), n, c, h, w, scale.data_ptr(), shift.data_ptr(),
                                     mean.data_ptr(), invstd.data_ptr(), k, ptr(scales), float(alpha), gx.data_ptr(),
                                     gvec[0].data_ptr(), gvec[1].data_ptr(), *_ws_args(ws), stream_ptr(x.device)), what)
    return gx, gvec[0], gvec[1]


def xnor_impl(mode) -> int:
    """Test / profiling hook (include/lsq_hip_debug.h): 1 / True = every XNOR convolution through the popcount kernel, 0 / False
    = the dispatcher picks the matrix-core kernel where it applies (fp4 operands on the scaled MFMA, the default), 2 = the
    same with the int8 matrix-core kernel of rounds 2-5 (identical results).  Returns the old value."""
    return lib().lsq_debug_xnor_impl(int(mode))


@contextlib.contextmanager
def solver_trace(rows: int, device):
    """Test hook (include/lsq_hip_debug.h): inside the block every LS-2 / LS-T solve stores the sorted position of the
    candidate it chose, one int32 per row, into the yielded tensor (read it after a synchronize)."""
    buf = torch.full((rows,), -2, dtype=torch.int32, device=device)
    lib().lsq_debug_solver_trace(buf.data_ptr())
    try:
        yield buf
    finally:
        torch.cuda.synchronize(device)
        lib().lsq_debug_solver_trace(None)


@contextlib.contextmanager
def debug_switches(xnor_popcount: Optional[bool] = None, force_streaming: Optional[bool] = None,
                   fused_mode: Optional[int] = None):
    """Set the library's test hooks (include/lsq_hip_debug.h) for the duration of a ``with`` block and restore the
    previous values afterwards, whatever happens inside.  Process-wide: meant for single-threaded tests and scripts."""
    handle = lib()
    old = {}
    try:
        if xnor_popcount is not None:
            old['lsq_debug_xnor_impl'] = handle.lsq_debug_xnor_impl(int(xnor_popcount))
        if force_streaming is not None:
            old['lsq_debug_force_streaming'] = handle.lsq_debug_force_streaming(int(bool(force_streaming)))
        if fused_mode is not None:
            old['lsq_debug_fused_mode'] = handle.lsq_debug_fused_mode(int(fused_mode))
        yield
    finally:
        for name, value in old.items():
            getattr(handle, name)(value)
