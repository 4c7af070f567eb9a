"""The C-ABI libraries as data: one table that ``quant._hip`` loads them from, ``__graft_entry__`` builds them from and
tests/test_sublib_table_host.py holds against the headers under ``include/``.  Imports ctypes and nothing heavier, so it can
be read before anything is built.

A prototype is ``symbol: (restype, [argtypes])``.  A wrong one is not an exception but a kernel reading the wrong pointer,
which is why every entry is checked against its header's declaration (symbols, parameter counts, parameter kinds)."""

import collections
import ctypes

vp, i32, i64, f32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t


class ConvGeom(ctypes.Structure):
    """Mirror of ``lsq_conv_geom``."""

    _fields_ = [(n, ctypes.c_int32) for n in (
        'N', 'C', 'H', 'W', 'O', 'KH', 'KW', 'stride_h', 'stride_w',
        'pad_h', 'pad_w', 'dil_h', 'dil_w', 'groups')]

    def key(self):
        k = self.__dict__.get('_key')             # (make_geom leaves the tuple it was built from: 14 ctypes field reads otherwise)
        return k if k is not None else tuple(getattr(self, n) for n, _ in self._fields_)


class NextLs1(ctypes.Structure):
    """Mirror of ``lsq_next_ls1``: where a chained convolution leaves the next layer's 1-bit input."""

    _fields_ = [('planes', ctypes.c_void_p), ('sum_units', ctypes.c_void_p), ('pre_scale', ctypes.c_void_p),
                ('pre_shift', ctypes.c_void_p), ('clamp_alpha', ctypes.c_float), ('pad_h', ctypes.c_int32),
                ('pad_w', ctypes.c_int32)]


class ConvDgradPlan(ctypes.Structure):
    """Mirror of ``lsq_conv_dgrad_plan``."""

    _fields_ = [(name, ctypes.c_int32) for name in ('kernel', 'classes', 'dead_classes', 'tap_steps')]


class Proj(ctypes.Structure):
    """Mirror of ``lsq_proj``: the projection shortcut lsq_xnor_conv2d_proj computes in its epilogue's residual registers."""

    _fields_ = [('x', ctypes.c_void_p), ('w', ctypes.c_void_p), ('bias', ctypes.c_void_p), ('C', ctypes.c_int32),
                ('H', ctypes.c_int32), ('W', ctypes.c_int32), ('stride', ctypes.c_int32), ('post', ctypes.c_int32)]


class ProjHalf(ctypes.Structure):
    """Mirror of ``lsq_proj_half``: ``lsq_proj`` with ``x`` of the call's 16-bit type (lsq_xnor_conv2d_proj_half)."""

    _fields_ = Proj._fields_


gp = ctypes.POINTER(ConvGeom)

# ---- liblsq_hip.so: {header: prototypes}; quant._hip.lib() applies both (ABI_VERSION and the LSQ_HIP_LIB override live there)
MAIN_PROTOTYPES = {
    'lsq_hip.h': {
        'lsq_abi_version': (i32, []),
        'lsq_error_string': (ctypes.c_char_p, [i32]),
        'lsq_act_plane_words': (i64, [gp]),
        'lsq_weight_plane_words': (i64, [gp]),
        'lsq_act_quant': (i32, [vp, gp, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp, sz, vp]),
        'lsq_solver_workspace_bytes': (i64, [i64]),
        'lsq_sweep_workspace_bytes': (i64, [i64]),
        'lsq_solve_rows': (i32, [vp, i64, i64, i32, i32, f32, vp, vp, vp, sz, vp]),
        'lsq_pack_weight': (i32, [vp, gp, i32, vp, vp, vp, vp]),
        'lsq_xnor_conv2d': (i32, [vp, i32, vp, vp, vp, i32, vp, vp, gp, i32, vp, vp, vp, vp, vp]),
        'lsq_signw_conv2d': (i32, [vp, f32, vp, vp, vp, vp, i32, vp, vp, gp, i32, vp, vp, vp, vp, vp]),
        'lsq_signw_weight_bytes': (i64, [gp, i32]),
        'lsq_signw_prepare_weight': (i32, [vp, i32, gp, vp, vp]),
        'lsq_pool_bias_relu_nhwc': (i32, [vp, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, vp]),
        'lsq_pointwise_conv': (i32, [vp, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp]),
        'lsq_xnor_conv2d_chain': (i32, [vp, vp, vp, f32, vp, vp, i32, vp, vp, gp, i32, vp, vp, vp, ctypes.POINTER(NextLs1),
                                        vp, vp]),
        'lsq_quant_values': (i32, [vp, i64, i64, i32, vp, f32, vp, vp]),
        'lsq_ste_backward': (i32, [vp, vp, i64, i64, i32, vp, f32, vp, vp]),
        'lsq_stem_conv_pool': (i32, [vp, i32, i32, i32, vp, vp, i32, vp, vp, vp]),
    },
    'lsq_hip_debug.h': {
        'lsq_debug_xnor_impl': (i32, [i32]),
        'lsq_debug_force_streaming': (i32, [i32]),
        'lsq_debug_fused_mode': (i32, [i32]),
        'lsq_debug_solver_trace': (i32, [vp]),
    },
}

# ---- the libraries beside it: csrc/<dir>/Makefile (which includes csrc/sublib.mk) builds lib/liblsq_hip_<dir>.so from
# include/lsq_hip_<dir>.h; the version symbol is lsq_<dir>_abi_version, the first of the prototypes.  ``pattern`` is the regex
# of the names the header may declare.
SubLib = collections.namedtuple('SubLib', 'dir header version_symbol version pattern prototypes')


def _entry(dir, pattern, prototypes, version=1):
    symbol = f'lsq_{dir}_abi_version'
    return SubLib(dir, f'lsq_hip_{dir}.h', symbol, version, f'lsq_{dir}_[a-z0-9_]+' + pattern, {symbol: (i32, []), **prototypes})


SUBLIBS = (
    _entry('train', '', {
        'lsq_train_wgrad_workspace_bytes': (sz, [gp, i32]),
        'lsq_train_wgrad': (i32, [vp, i32, vp, vp, gp, vp, vp, sz, vp])}),
    _entry('linear', '', {
        'lsq_linear_xnor': (i32, [vp, i32, vp, i64, vp, vp, i32, vp, vp, i64, i64, i64, vp, vp])}),
    _entry('linear_fp', '|lsq_linear_signw[a-z0-9_]*', {
        'lsq_linear_signw': (i32, [vp, f32, vp, i32, vp, vp, i64, i64, i64, vp, vp])}),
    _entry('linear_train', '|lsq_linear_signw_dgrad[a-z0-9_]*', {
        'lsq_linear_signw_dgrad': (i32, [vp, vp, i32, vp, i64, i64, i64, vp, vp, sz, vp]),
        'lsq_linear_signw_dgrad_workspace_bytes': (sz, [i32, i64, i64])}),
    _entry('linear_train_half', '|lsq_linear_signw_dgrad_half[a-z0-9_]*', {
        'lsq_linear_signw_dgrad_half_workspace_bytes': (sz, [i32, i64, i64]),
        'lsq_linear_signw_dgrad_half': (i32, [vp, i32, vp, i32, vp, i64, i64, i64, vp, i64, i32, vp, f32, vp, i32, vp, sz, vp])}),
    _entry('linear_wgrad', '|lsq_linear_signx_wgrad[a-z0-9_]*', {
        'lsq_linear_signx_wgrad': (i32, [vp, vp, i32, vp, f32, i64, i64, i64, i64, vp, vp, sz, vp]),
        'lsq_linear_signx_wgrad_workspace_bytes': (sz, [i32, i64, i64, i64, i64])}),
    _entry('linear_half', '|lsq_linear_signw_half[a-z0-9_]*', {
        'lsq_linear_signw_half': (i32, [vp, i32, f32, vp, i32, vp, vp, i64, i64, i64, vp, i32, vp, sz, vp]),
        'lsq_linear_signw_half_workspace_bytes': (i64, [i64, i64, i32, i32])}),
    _entry('linear_act_half', '|lsq_linear_act_quant_half[a-z0-9_]*', {
        'lsq_linear_act_quant_half': (i32, [vp, i32, i64, i64, i32, i32, f32, vp, vp, vp, vp])}),
    _entry('linear_act_solve', '|lsq_linear_act_quant_solve_half[a-z0-9_]*', {
        'lsq_linear_act_quant_solve_half': (i32, [vp, i32, i64, i64, i32, i32, f32, vp, vp, vp, vp])}),
    _entry('conv_act_half', '|lsq_act_quant_half[a-z0-9_]*', {
        'lsq_act_quant_half': (i32, [vp, i32, vp, i32, i32, i32, f32, vp, vp, vp, vp, vp])}),
    _entry('conv_half', '|lsq_signw_conv2d_half[a-z0-9_]*', {
        'lsq_signw_conv2d_half_plan': (i32, [vp]),
        'lsq_signw_conv2d_half_workspace_bytes': (i64, [vp, i32, i32]),
        'lsq_signw_conv2d_half': (i32, [vp, i32, f32, vp, i32, vp, vp, vp, vp, i32, vp, sz, vp])}),
    _entry('conv_train', '|lsq_signw_conv2d_dgrad[a-z0-9_]*', {
        'lsq_signw_conv2d_dgrad_plan': (i32, [vp, vp]),
        'lsq_signw_conv2d_dgrad_workspace_bytes': (sz, [vp, i32]),
        'lsq_signw_conv2d_dgrad': (i32, [vp, vp, i32, vp, vp, vp, vp, sz, vp])}),
    _entry('conv_train_half', '|lsq_signw_conv2d_dgrad_half[a-z0-9_]*', {
        'lsq_signw_conv2d_dgrad_half_plan': (i32, [vp, vp]),
        'lsq_signw_conv2d_dgrad_half_workspace_bytes': (sz, [vp, i32]),
        'lsq_signw_conv2d_dgrad_half': (i32, [vp, i32, vp, i32, vp, vp, vp, i32, vp, f32, vp, i32, vp, sz, vp])}),
    _entry('conv_proj', '|lsq_xnor_conv2d_proj[a-z0-9_]*', {
        'lsq_xnor_conv2d_proj': (i32, [vp, i32, vp, vp, vp, i32, vp, vp, gp, i32, vp, vp, vp, ctypes.POINTER(Proj), vp, vp])}),
    _entry('conv_xnor_half', '|lsq_xnor_conv2d_half[a-z0-9_]*', {
        'lsq_xnor_conv2d_half_workspace_bytes': (sz, [gp, i32, i32]),
        'lsq_xnor_conv2d_half': (i32, [vp, i32, vp, vp, vp, i32, vp, vp, gp, i32, vp, vp, vp, i32, vp, vp, sz, vp])}),
    _entry('train_half', '|lsq_train_wgrad_half[a-z0-9_]*', {
        'lsq_train_wgrad_half_workspace_bytes': (sz, [gp, i32, i32]),
        'lsq_train_wgrad_half': (i32, [vp, i32, vp, vp, i32, gp, vp, vp, vp, sz, vp])}),
    _entry('linear_wgrad_half', '|lsq_linear_signx_wgrad_half[a-z0-9_]*', {
        'lsq_linear_signx_wgrad_half_workspace_bytes': (sz, [i32, i64, i64, i64, i64]),
        'lsq_linear_signx_wgrad_half': (i32, [vp, vp, i32, i32, vp, f32, i64, i64, i64, i64, vp, i32, vp, vp, vp, sz, vp])}),
    _entry('conv_act_bn_half', '|lsq_act_quant_bn_half[a-z0-9_]*', {
        'lsq_act_quant_bn_half': (i32, [vp, i32, vp, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp])}),
    _entry('conv_proj_half', '|lsq_pointwise_conv_half|lsq_xnor_conv2d_proj_half', {
        'lsq_pointwise_conv_half': (i32, [vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp]),
        'lsq_xnor_conv2d_proj_half': (i32, [vp, i32, vp, vp, vp, i32, vp, vp, gp, i32, vp, vp, vp, ctypes.POINTER(ProjHalf),
                                            i32, vp, vp])}),
    _entry('conv_fused_half', '|lsq_signw_conv2d_fused_half[a-z0-9_]*', {
        'lsq_signw_conv2d_fused_half_plan': (i32, [vp]),
        'lsq_signw_conv2d_fused_half_workspace_bytes': (i64, [vp, i32, i32]),
        'lsq_signw_conv2d_fused_half': (i32, [vp, i32, f32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, sz, vp])}),
    _entry('bn_train', '|lsq_bn_apply|lsq_quant_values_bn|lsq_bn_ste_backward[a-z0-9_]*', {
        'lsq_bn_train_workspace_bytes': (sz, [i32, i32, i32, i32]),
        'lsq_bn_train_stats': (i32, [vp, i32, i32, i32, i32, vp, vp, f32, f32, i64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        'lsq_bn_apply': (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp]),
        'lsq_quant_values_bn': (i32, [vp, i32, i32, i32, i32, vp, vp, i32, vp, f32, vp, vp]),
        'lsq_bn_ste_backward_workspace_bytes': (sz, [i32, i32, i32, i32]),
        'lsq_bn_ste_backward': (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, f32, vp, vp, vp, vp, sz, vp])}),
)
BY_DIR = {s.dir: s for s in SUBLIBS}


def soname(s: SubLib) -> str:
    return f'liblsq_hip_{s.dir}.so'


def apply_prototypes(handle, prototypes: dict) -> None:
    for symbol, (restype, argtypes) in prototypes.items():
        fn = getattr(handle, symbol)
        fn.restype, fn.argtypes = restype, argtypes
