"""``QuantConv2d``: 2-D convolution of scaled-binary-quantized activations and weights.

Drop-in for the reference's ``quant/binary/binary_conv.py`` (:48-173): same constructor
(positional ``x_quant, w_quant, in_channels, out_channels, kernel_size, clamp,
moving_average_mode, moving_average_momentum`` then ``nn.Conv2d`` kwargs), same attributes
(``x_approximate``, ``w_approximate``, ``clamping_fn``, ``quantized_parameters``), same
``state_dict`` keys and the same ``ValueError`` on bad schemes / clamp kinds.

Dispatch of ``forward``:
  * CUDA (ROCm) tensor, ``eval()`` mode, no gradient wanted for the input -> gfx950 kernels via
    the C ABI (``quant._hip``): clamp + per-sample scale solve + sign packing in one kernel,
    then an XNOR-popcount convolution (binary activations) or a bf16-MFMA convolution
    (fp activations) against weight sign planes packed once per ``eval()`` session.  There is
    no fallback on this branch: a missing library or a failed launch raises.
  * CUDA tensor in ``train()`` mode, plain geometry -> the same kernels for the forward and the kernels of
    ``quant.binary.hip_train`` for the backward (straight-through estimator, transposed sign-weight convolution), one
    ``torch.autograd.Function`` per call;
  * with ``act_half`` set (class attribute, False by default): a bf16 / fp16 CUDA tensor in ``eval()`` mode, binary
    activations, fp32 weights, autocast off or set to the input's own type -> lsq_act_quant_half
    (liblsq_hip_conv_act_half.so) reads the 16-bit samples as they are (the clamp bound rounded into their type), then the
    XNOR convolution as above; the output is its fp32 result rounded once into the input's type.  With
    ``act_half_kernel = False`` the samples go through ``x.float()`` -> lsq_act_quant instead: the same bits;
    ``act_half_solve = False`` keeps free-running ``ls-2`` / ``ls-T`` on torch.  No fallback on this branch;
  * with ``fp_half`` set (class attribute, False by default, a switch of its own beside ``act_half``): a bf16 / fp16 CUDA
    tensor in ``eval()`` mode, ``fp`` activations, binary fp32 weights, autocast off or set to the input's own type ->
    lsq_signw_conv2d_half (liblsq_hip_conv_half.so) reads the 16-bit samples as they are (the clamp bound rounded into their
    type) against the weight sign planes, with fp32 weight scales and fp32 accumulation; the output is its fp32 result
    rounded once into the input's type.  With ``fp_half_kernel = False`` the samples go through ``x.float()`` ->
    lsq_signw_conv2d instead, the comparator of DESIGN 4.19.  No fallback on this branch;
  * with ``hip_train_half`` set (class attribute, False by default): a bf16 / fp16 CUDA tensor in ``train()`` mode, binary fp32
    weights, autocast off or set to the input's own type -> the 16-bit step of ``quant.binary.hip_train``:
    lsq_act_quant_half / lsq_signw_conv2d_half forward, one lsq_signw_conv2d_dgrad_half for the input gradient;
  * with ``xnor_half`` set on top of ``act_half`` / ``hip_train_half`` (class attribute, False by default): the XNOR
    convolution of a 16-bit input is lsq_xnor_conv2d_half (liblsq_hip_conv_xnor_half.so), which writes the input's type itself
    -- the same bits, no fp32 y --, and ``fused_forward`` hands it non-linearity and 16-bit residuals; a
    residual given as a ``ProjectionShortcut`` of a 16-bit input (``quant.models.resnet.PROJ_HALF``) is computed inside that
    launch, lsq_xnor_conv2d_proj_half (liblsq_hip_conv_proj_half.so);
  * with ``act_half_bn_fold`` set on top of ``act_half`` (class attribute, False by default): ``fused_forward`` folds an
    eval-mode ``pre_bn`` of a 16-bit input into the quantizer's read, lsq_act_quant_bn_half
    (liblsq_hip_conv_act_bn_half.so), instead of running it in torch;
  * with ``fp_half_fused`` set on top of ``fp_half`` (class attribute, False by default): ``fused_forward`` on a 16-bit input
    with ``fp`` activations hands non-linearity and 16-bit residuals to ONE lsq_signw_conv2d_fused_half
    (liblsq_hip_conv_fused_half.so), which rounds once; with ``fp_half_bn_fold`` on top of it an eval-mode ``pre_bn`` goes
    into that launch's read too instead of running in torch;
  * anything else (CPU tensors, grouped / dilated training convolutions, 16-bit inputs with binary activations without
    ``act_half`` or with ``fp`` activations without ``fp_half``, 16-bit weights, an autocast of another type) -> the torch
    formulation in ``quant.binary``.

Construction, the quantizer / clamp factories, cache invalidation, workspace retention and the eval-side activation
quantization are ``quant.binary.hip_module.HipQuantModule``'s, shared with ``QuantLinear``; this file keeps what is the
convolution's own: the kernels' limits, packed weights, the folded batch norm, chaining and the fused epilogue.
"""

from typing import Any, Dict, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from quant.binary.hip_module import HipQuantModule


class ProjectionShortcut:
    """A residual operand of ``QuantConv2d.fused_forward`` given as its recipe instead of a tensor: the folded projection
    shortcut ``conv2d(x, w[:, :, None, None], b, stride)`` of a down-sampling block (CUDA fp32 ``x`` [N, C, H, W], ``w`` [O, C],
    channels multiples of 64).  Passed as ``res_pre`` or ``res_post``, it is computed inside the XNOR convolution where
    lsq_xnor_conv2d_proj takes the call and by lsq_pointwise_conv in front of it elsewhere -- the same bits either way.
    ``tensor()`` is that separate launch; ``self[rows]`` the shortcut of the samples ``rows`` alone (what a reader of the
    residual of a few samples needs, e.g. a layer-by-layer check).

    ``x`` may be bf16 / fp16 (``quant.models.resnet.PROJ_HALF``; ``w`` and ``b`` stay fp32): the consumer is then
    lsq_xnor_conv2d_proj_half, which keeps the shortcut in fp32 registers and rounds the block's output once, and ``tensor()``
    is lsq_pointwise_conv_half, a tensor of ``x``'s type -- the shortcut rounded on its own, so in 16 bits the two are NOT the
    same bits (include/lsq_hip_conv_proj_half.h)."""

    def __init__(self, x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], stride: int) -> None:
        self.x, self.w, self.b, self.stride = x.detach(), w, b, int(stride)

    def tensor(self, rows=None) -> torch.Tensor:
        from quant import _hip
        x = self.x if rows is None else self.x[rows]
        if x.dtype in (torch.bfloat16, torch.float16):
            return _hip.pointwise_conv_half(x.contiguous(), self.w, self.b, self.stride)
        return _hip.pointwise_conv(x, self.w, self.b, self.stride)

    def out_shape(self) -> tuple:
        n, _, h, w = self.x.shape
        return (n, self.w.shape[0], (h - 1) // self.stride + 1, (w - 1) // self.stride + 1)

    def __getitem__(self, rows) -> torch.Tensor:
        return self.tensor(rows)


class QuantConv2d(HipQuantModule, nn.Conv2d):
    """``Conv2d(x_quant(clamp(x)), w_quant(w))`` with schemes fp | ls-1 | ls-2 | ls-T | gf-k."""

    def __init__(self, x_quant: str, w_quant: str, in_channels: int, out_channels: int,
                 kernel_size: Union[int, Tuple[int, int]], clamp: Optional[Dict] = None,
                 moving_average_mode: str = 'off', moving_average_momentum: float = 0.99,
                 **kwargs: Any) -> None:
        super().__init__(x_quant, w_quant, clamp, moving_average_mode, moving_average_momentum,
                         in_channels, out_channels, kernel_size, **kwargs)

    # ------------------------------------------------------------------ forward
    #: train-mode CUDA tensors through the kernels (False: the torch formulation, e.g. to compare the two in tests)
    hip_train = True

    #: a bf16 / fp16 input (fp32 weights, binary activations, eval mode, autocast off or set to the input's type) takes the
    #: kernels: lsq_act_quant_half reads the 16-bit samples, lsq_xnor_conv2d computes in fp32 and the result is rounded once
    #: into the input's type.  False: the torch formulation, the default until the kernel is measured
    act_half = False

    #: with act_half: the 16-bit input is quantized by lsq_act_quant_half (True) or, for the comparison of DESIGN 4.18, by
    #: lsq_act_quant on x.float() with the bound rounded into the type (False): the same planes and output bits
    act_half_kernel = True

    #: with act_half: free-running ls-2 / ls-T activations on a 16-bit input take the kernels too (False: the torch formulation)
    act_half_solve = True

    #: a bf16 / fp16 input with ``fp`` activations (binary fp32 weights, eval mode, autocast off or set to the input's type)
    #: takes lsq_signw_conv2d_half: the 16-bit samples against the sign planes, fp32 scales and accumulation, rounded once into
    #: the input's type.  False: the torch formulation, the default until the kernel is measured
    fp_half = False

    #: with fp_half: the 16-bit input is convolved by lsq_signw_conv2d_half (True) or, for the comparison of DESIGN 4.19, by
    #: lsq_signw_conv2d on x.float() with the bound rounded into the type (False)
    fp_half_kernel = True

    #: a bf16 / fp16 input in ``train()`` mode (binary fp32 weights, autocast off or set to the input's type) takes the kernels
    #: forward and backward: ``hip_train._QuantConv2dStepHalf``, whose input gradient is one lsq_signw_conv2d_dgrad_half.
    #: A switch of its own, independent of ``act_half`` / ``fp_half``.  False: the torch formulation, the default whatever the
    #: measurement says in the change that adds it
    hip_train_half = False

    #: with ``act_half`` (eval) or ``hip_train_half`` (train): the XNOR convolution of a bf16 / fp16 input writes its result in
    #: the input's type itself (lsq_xnor_conv2d_half: no fp32 y, no ``.to()`` pass -- the same bits), and ``fused_forward`` on
    #: such an input hands ``relu`` / ``prelu`` and 16-bit residuals to that one launch, which rounds once.  A switch of its
    #: own; False: lsq_xnor_conv2d + ``.to()`` and the composition in torch, the default whatever the measurement says in the
    #: change that adds it
    xnor_half = False

    #: with ``act_half`` and ``act_half_kernel``: ``fused_forward`` on a bf16 / fp16 CUDA input with binary activations does
    #: not run an eval-mode ``pre_bn`` (running statistics) in torch but hands its folded (scale, shift) to the quantizer's
    #: read (lsq_act_quant_bn_half): one read and one write of the activation tensor fewer.  The result is bit for bit the
    #: layer on ``(x.float() * scale + shift).to(x.dtype)``, which is within one rounding of the type of torch's own batch
    #: norm but not its bits.  A switch of its own; False: torch's batch norm in front of lsq_act_quant_half, the default
    #: whatever the measurement says in the change that adds it
    act_half_bn_fold = False

    #: with ``fp_half`` and ``fp_half_kernel``: ``fused_forward`` on a bf16 / fp16 CUDA input with ``fp`` activations runs the
    #: batch norm in torch in front (if any) and then ONE lsq_signw_conv2d_fused_half, which adds ``res_pre``, applies ReLU /
    #: PReLU and adds ``res_post`` in fp32 and rounds once, where the composition in torch rounds after every step: other
    #: bits, within the roundings it saves.  Residuals of another type or shape take the composition.  A switch of its own;
    #: False: the composition around lsq_signw_conv2d_half, the default whatever the measurement says in the change that adds
    #: it
    fp_half_fused = False

    #: with ``fp_half_fused``: an eval-mode ``pre_bn`` (running statistics, on x's device) is not run in torch but handed to
    #: that launch as its folded (scale, shift): the layer on ``(x.float() * scale + shift).to(x.dtype)``, within one rounding
    #: of the type of torch's own batch norm but not its bits.  A train-mode batch norm keeps the whole composition, as with
    #: both switches off.  False by default
    fp_half_bn_fold = False

    #: with ``hip_train``: a train-mode ``nn.BatchNorm2d`` in front of this convolution (``XnorBasicBlock``'s bn -> conv pairs,
    #: fp32 input) is not run in torch but joins the step, ``hip_train._BNQuantConv2dStep``: lsq_bn_train_stats computes the
    #: batch statistics in one read of x, the quantizer applies fmaf(x, scale, shift) inside its own read and backward is one
    #: lsq_bn_ste_backward for the straight-through estimator and the batch norm together; bn(x) is never written or saved.
    #: The statistics and gradients are within the stated roundings of torch's batch norm, not its bits.  A switch of its own;
    #: False: ``conv(bn(x))`` as before, the default whatever the measurement says in the change that adds it
    train_bn_fold = False

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._wants_hip(x):
            return self._forward_hip(x)
        if self.training and self.hip_train and x.is_cuda:
            from quant.binary import hip_train
            if hip_train.supported(self, x):
                return hip_train.train_step_forward(self, x)
        return self._forward_torch(x)

    def _forward_torch(self, x: torch.Tensor) -> torch.Tensor:
        x_q = self.x_approximate(self.clamping_fn(x))
        w_q = self.w_approximate(self.weight)
        return F.conv2d(x_q, w_q, self.bias, self.stride, self.padding, self.dilation, self.groups)

    def _wants_hip(self, x: torch.Tensor) -> bool:
        if not x.is_cuda or self.training:
            return False
        if torch.is_grad_enabled() and x.requires_grad:
            return False
        if self.padding_mode != 'zeros' or isinstance(self.padding, str) or x.dim() != 4:
            return False
        if self.w_quant == 'fp':          # nothing binary on the weight side: plain conv
            return False
        if x.dtype != torch.float32:
            if torch.is_autocast_enabled('cuda') and torch.get_autocast_dtype('cuda') != x.dtype:
                return False              # (a 16-bit input under an autocast of another type: torch decides the types)
            if (self.x_quant in ('ls-2', 'ls-T') and not self.act_half_solve
                    and self.x_approximate.eval_scales(x.shape[0]) is None):
                return False
        return self._hip_supports(x)

    def _hip_supports(self, x: torch.Tensor) -> bool:
        """The limits of the kernels (include/lsq_hip.h); anything outside them takes the torch formulation,
        exactly as training and CPU tensors do: fp32 (bf16 / fp16 inputs with ``act_half`` / ``fp_half``), at most 8 bit planes, kernels up to 8x8 on the
        XNOR path, at most 2^22 sub-sampled keys per row for the LS-2 / LS-T solve."""
        # (memoised per input dtype and row shape: the rest is fixed at construction; _apply -- .to(), .half() -- clears the cache)
        key = ('sup', x.dtype, x.shape[1], x.shape[2], x.shape[3])
        if x.dtype != torch.float32:
            key += (self.act_half, self.fp_half)
            if self.x_quant == 'fp':      # (lsq_signw_conv2d_half's index limits depend on the batch size too)
                key += (x.shape[0],)
        hit = self._hip_cache.get(key)
        if hit is None:
            if sum(1 for kk in self._hip_cache if isinstance(kk, tuple) and kk[0] == 'sup') >= 16:      # (many image sizes)
                for kk in [kk for kk in self._hip_cache if isinstance(kk, tuple) and kk[0] == 'sup']:
                    del self._hip_cache[kk]
            hit = self._hip_cache[key] = self._hip_supports_uncached(x)
        return hit

    def _hip_supports_uncached(self, x: torch.Tensor) -> bool:
        from quant import _hip
        if self.weight.dtype != torch.float32:
            return False
        if x.dtype != torch.float32:      # bf16 / fp16, on request: lsq_act_quant_half in front of the fp32 XNOR convolution,
            if x.dtype not in (torch.bfloat16, torch.float16):          # or lsq_signw_conv2d_half for fp activations
                return False
            if not (self.fp_half if self.x_quant == 'fp' else self.act_half):
                return False
            if self.x_quant == 'fp' and not _hip.signw_conv2d_half_supported(self._geom_of(x, _hip)):
                return False              # (past the library's 32-bit index limits, include/lsq_hip_conv_half.h)
        if getattr(self.w_approximate, 'k', 1) > _hip.MAX_PLANES:      # gf-k weights: k planes
            return False
        if self.x_quant != 'fp':
            if getattr(self.x_approximate, 'n_planes', 1) > _hip.MAX_PLANES or max(self.kernel_size) > _hip.MAX_XNOR_KERNEL:
                return False
            if self.x_quant in ('ls-2', 'ls-T'):
                m = x.shape[1] * x.shape[2] * x.shape[3]
                if (m + self.act_skip - 1) // self.act_skip >= _hip.MAX_SOLVER_KEYS:
                    return False
        return True

    # ------------------------------------------------------------------ HIP path
    def _geom_of(self, x: torch.Tensor, _hip):
        n, c, h, w = x.shape
        kh, kw = self.kernel_size
        return _hip.make_geom(n, c, h, w, self.out_channels, kh, kw, self.stride, self.padding, self.dilation, self.groups)

    def _packed_weights(self, geom, _hip, prep: bool = True):
        """(wbits, wsum, wscales, wprep) of this eval session.  ``prep``: the caller reads ``wprep``, the bf16 operand image of
        lsq_signw_conv2d's 3x3 fast path (fp activations only); it is built with the planes, or by the first call that asks
        for it -- lsq_signw_conv2d_half never does."""
        wq = self.w_approximate
        bufs = wq.cached_scales()
        w = self._parameters['weight']
        stamp = (w._version, w.data_ptr(), geom.key()[4:]) + tuple((b._version, b.data_ptr()) for b in bufs)
        hit = self._hip_cache.get('w')
        if hit is None or hit[0] != stamp:
            scales = wq.plane_scales().to(torch.float32).contiguous()
            wbits, wsum = _hip.pack_weight(self.weight.detach(), geom, scales)
            hit = [stamp, wbits, wsum, scales, None, False]          # (wprep, and whether it has been asked for)
            self._hip_cache['w'] = hit
        if prep and not hit[5]:
            # fp activations: the bf16 operand image of the 3x3 fast path, built once per session
            hit[4] = _hip.signw_prepare_weight(hit[1], hit[3].shape[0], geom) if self.x_quant == 'fp' else None
            hit[5] = True
        return hit[1], hit[2], hit[3], hit[4]

    def fused_forward(self, x: torch.Tensor, pre_bn: Optional[nn.BatchNorm2d] = None, relu: bool = False,
                      res_pre: Optional[torch.Tensor] = None, res_post: Optional[torch.Tensor] = None,
                      prelu: Optional[torch.Tensor] = None, next_q: Optional[tuple] = None,
                      res_ready: Optional[torch.cuda.Event] = None) -> torch.Tensor:
        """``act(self(pre_bn(x)) + res_pre) + res_post`` -- one residual-block half (quant/models/resnet.py:
        95-100, 182-190); ``act`` = ReLU (``relu=True``), PReLU (``prelu`` = the nn.PReLU weight) or identity.
        One of the two residuals may be a ``ProjectionShortcut`` in place of a tensor.
        On the HIP path the eval-mode batch norm is folded into the quantizer's read and the non-linearity /
        shortcut additions into the convolution's epilogue, so none of them is a separate pass over HBM;
        elsewhere it is the plain composition of the modules."""
        xin = None
        # act_half_bn_fold: the batch norm of a 16-bit input goes into the quantizer's read (lsq_act_quant_bn_half) instead of
        # a torch pass of its own -- here and in the composition below
        fold = self.act_half_bn_fold and pre_bn is not None and self._folds_half_bn(x, pre_bn)
        if self.xnor_half and x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and self.x_quant != 'fp':
            # a 16-bit input with ``xnor_half``: the batch norm in torch in front of the quantizer (lsq_act_quant_half folds
            # none; with ``act_half_bn_fold`` lsq_act_quant_bn_half reads through it), then non-linearity and 16-bit residuals
            # in the epilogue of lsq_xnor_conv2d_half -- one launch, one rounding.  Residuals of another type or shape take
            # the composition below.  A ProjectionShortcut of x's own type (resnet.PROJ_HALF) goes down as it is: the launch
            # is then lsq_xnor_conv2d_proj_half; one of an fp32 x becomes its fp32 tensor here, as before.
            if isinstance(res_pre, ProjectionShortcut) and res_pre.x.dtype != x.dtype:
                res_pre = res_pre.tensor()
            if isinstance(res_post, ProjectionShortcut) and res_post.x.dtype != x.dtype:
                res_post = res_post.tensor()
            if fold:
                if self._half_epilogue_fits(x, res_pre, res_post, prelu):
                    return self._forward_hip(x, pre_bn, relu, res_pre, res_post, prelu, None, res_ready)
            else:
                xin = x if pre_bn is None else pre_bn(x)
                if self._wants_hip(xin) and self._half_epilogue_fits(xin, res_pre, res_post, prelu):
                    return self._forward_hip(xin, None, relu, res_pre, res_post, prelu, None, res_ready)
        if self._fuses_fp_half(x, pre_bn) and self._half_epilogue_fits(x, res_pre, res_post, prelu):
            # a 16-bit input with fp activations and ``fp_half_fused``: the batch norm in torch in front (with
            # ``fp_half_bn_fold`` in the launch's read), then non-linearity and 16-bit residuals in the epilogue of
            # lsq_signw_conv2d_fused_half -- one launch, one rounding.  A ProjectionShortcut of x's type is its tensor first.
            pre = self._folded_bn(pre_bn) if pre_bn is not None and self._folds_fp_half_bn(x, pre_bn) else None
            # (an eval-mode batch norm that runs here runs ONCE: should its result be of another type, the composition below
            # takes ``xin`` as it is instead of calling ``pre_bn`` again; a train-mode one never gets here)
            xin = x if pre_bn is None or pre is not None else pre_bn(x)
            if xin.dtype == x.dtype and xin.shape == x.shape:
                if isinstance(res_pre, ProjectionShortcut):
                    res_pre = res_pre.tensor()
                if isinstance(res_post, ProjectionShortcut):
                    res_post = res_post.tensor()
                return self._forward_fp_half_fused(xin, pre, relu, res_pre, res_post, prelu, res_ready)
        if (x.dtype == torch.float32 and self._wants_hip(x)
                and (pre_bn is None or (not pre_bn.training and pre_bn.track_running_stats))):
            # next_q = (batch norm or None, QuantConv2d) that will consume the result: with 1-bit activations on both
            # sides the consumer's quantizer runs in THIS convolution's epilogue (quant.binary.chain)
            # res_ready: the residual operands were produced on another stream (the projection shortcut, models/resnet.py);
            # the quantizer does not need them, the convolution's launch waits for the event
            return self._forward_hip(x, pre_bn, relu, res_pre, res_post, prelu, next_q, res_ready)
        if isinstance(res_pre, ProjectionShortcut):
            res_pre = res_pre.tensor()
        if isinstance(res_post, ProjectionShortcut):
            res_post = res_post.tensor()
        if res_ready is not None:
            torch.cuda.current_stream(x.device).wait_event(res_ready)
        if fold:                          # the layer alone on the kernels, the batch norm in its quantizer's read
            y = self._forward_hip(x, pre_bn)
        else:
            y = self(xin if xin is not None else (x if pre_bn is None else pre_bn(x)))
        if res_pre is not None:
            y = y + res_pre
        if relu:
            y = torch.relu(y)
        if prelu is not None:
            y = F.prelu(y, prelu)
        return y if res_post is None else y + res_post

    def _folds_half_bn(self, x: torch.Tensor, bn: nn.BatchNorm2d) -> bool:
        """Whether ``fused_forward`` folds ``bn`` into the 16-bit quantizer's read (``act_half_bn_fold``): a bf16 / fp16 CUDA
        input this layer takes on the kernels (eval mode, ``act_half``: ``_wants_hip`` needs x's type and shape alone, which
        the batch norm does not change), binary activations, lsq_act_quant_half in use (not the cast comparator), an eval-mode
        batch norm with running statistics on x's device.  A train-mode layer keeps torch's batch norm: autograd runs
        through it."""
        return (self.act_half_bn_fold and self.act_half_kernel and self.x_quant != 'fp' and x.is_cuda
                and x.dtype in (torch.bfloat16, torch.float16) and not bn.training and bn.track_running_stats
                and bn.running_mean is not None and bn.running_mean.device == x.device and self._wants_hip(x))

    def _fuses_fp_half(self, x: torch.Tensor, pre_bn: Optional[nn.BatchNorm2d] = None) -> bool:
        """Whether ``fused_forward`` hands its epilogue to lsq_signw_conv2d_fused_half (``fp_half_fused``): a bf16 / fp16 CUDA
        input with ``fp`` activations that this layer takes on lsq_signw_conv2d_half (``fp_half``, not the cast comparator;
        eval mode and the rest of ``_wants_hip``), and no train-mode batch norm in front (that one keeps the composition as it
        is: autograd and the running statistics are torch's).  The operands must pass ``_half_epilogue_fits`` besides."""
        return (self.fp_half_fused and self.fp_half and self.fp_half_kernel and self.x_quant == 'fp' and x.is_cuda
                and x.dtype in (torch.bfloat16, torch.float16) and (pre_bn is None or not pre_bn.training) and self._wants_hip(x))

    def _folds_fp_half_bn(self, x: torch.Tensor, bn: nn.BatchNorm2d) -> bool:
        """Whether that launch reads through ``bn`` (``fp_half_bn_fold``): the conditions of ``_folds_half_bn`` on the
        ``fp`` side -- an eval-mode batch norm with running statistics on x's device."""
        return (self.fp_half_bn_fold and self._fuses_fp_half(x, bn) and not bn.training and bn.track_running_stats
                and bn.running_mean is not None and bn.running_mean.device == x.device)

    def _forward_fp_half_fused(self, x: torch.Tensor, pre, relu: bool, res_pre: Optional[torch.Tensor],
                               res_post: Optional[torch.Tensor], prelu: Optional[torch.Tensor],
                               res_ready: Optional[torch.cuda.Event]) -> torch.Tensor:
        """One lsq_signw_conv2d_fused_half: the route of ``_forward_hip`` for a 16-bit input with fp activations, with the
        folded batch norm ``pre`` (or None) and the epilogue's operands handed down."""
        from quant import _hip
        x = x.detach().contiguous()
        geom = self._geom_of(x, _hip)
        wbits, _, wscales, _ = self._packed_weights(geom, _hip, prep=False)
        res_pre = None if res_pre is None else res_pre.detach().contiguous()
        res_post = None if res_post is None else res_post.detach().contiguous()
        bias = None if self.bias is None else self.bias.detach()
        if res_ready is not None:        # residual operands from a side stream: in front of the convolution
            torch.cuda.current_stream(x.device).wait_event(res_ready)
        return _hip.signw_conv2d_fused_half(x, self._alpha_in(x.dtype), wbits, wscales, bias, geom, pre, relu, res_pre, res_post,
                                            prelu)

    def _half_epilogue_fits(self, x: torch.Tensor, res_pre, res_post, prelu) -> bool:
        """Whether lsq_xnor_conv2d_half's epilogue (and lsq_signw_conv2d_fused_half's, which takes a ``ProjectionShortcut`` as
        its tensor) takes these operands: residuals that are CUDA tensors of the input's type
        and the output's shape, PReLU slopes in fp32 (1 or one per out-channel).  At most one of the residuals may be a
        ``ProjectionShortcut`` whose ``x`` is such a tensor and whose result has the output's shape (lsq_xnor_conv2d_proj_half,
        or lsq_pointwise_conv_half in front where that call is refused)."""
        from quant import _hip
        if x.dtype not in (torch.bfloat16, torch.float16) or x.dim() != 4:
            return False
        shape = (x.shape[0], self.out_channels) + tuple(_hip.out_hw(self._geom_of(x, _hip)))
        if isinstance(res_pre, ProjectionShortcut) and isinstance(res_post, ProjectionShortcut):
            return False
        for r in (res_pre, res_post):
            if isinstance(r, ProjectionShortcut):
                if not (r.x.is_cuda and r.x.device == x.device and r.x.dtype == x.dtype and r.x.dim() == 4
                        and r.out_shape() == shape):
                    return False
            elif r is not None and not (isinstance(r, torch.Tensor) and r.is_cuda and r.device == x.device and r.dtype == x.dtype
                                        and tuple(r.shape) == shape):
                return False
        return prelu is None or (prelu.is_cuda and prelu.dtype == torch.float32 and prelu.numel() in (1, self.out_channels))

    def _folded_bn(self, bn: nn.BatchNorm2d):
        """(scale, shift) with bn(x) = x * scale + shift in eval mode; cached on the BN's buffer versions."""
        # (read straight from the module's dicts: nn.Module.__getattr__ costs more than the rest of this check)
        b, p = bn._buffers, bn._parameters
        mean, var = b['running_mean'], b['running_var']
        stamp = (id(bn), bn.eps, mean._version, mean.data_ptr(), var._version, var.data_ptr())
        if bn.affine:
            gw, gb = p['weight'], p['bias']
            stamp += (gw._version, gw.data_ptr(), gb._version, gb.data_ptr())
        hit = self._hip_cache.get('bn')
        if hit is None or hit[0] != stamp:
            with torch.no_grad():
                inv = torch.rsqrt(bn.running_var.float() + bn.eps)
                scale = inv * bn.weight.float() if bn.affine else inv
                shift = (bn.bias.float() if bn.affine else 0) - bn.running_mean.float() * scale
            hit = (stamp, scale.contiguous(), shift.contiguous())
            self._hip_cache['bn'] = hit
        return hit[1], hit[2]

    def _chain_target(self, next_q, n: int, ho: int, wo: int, device, _hip):
        """``lsq_next_ls1`` for the consumer ``next_q = (bn, conv)`` of this layer's output, or None when the pair cannot
        be chained (other schemes, moving-average scales, no clamp, channel counts)."""
        from quant.binary import chain
        if next_q is None or not chain.ENABLED or self.x_quant != 'ls-1' or self.out_channels % 64:
            return None
        if n * self.out_channels * ho * wo > chain.MAX_ELEMENTS:    # (large layers: the separate HBM-bound sweep is cheaper)
            return None
        if self.out_channels * ho * wo > chain.MAX_ROW_ELEMENTS:    # (lsq_xnor_conv2d_chain refuses it: include/lsq_hip.h)
            return None
        bn, conv = next_q
        if not isinstance(conv, QuantConv2d) or conv.x_quant != 'ls-1' or conv.training or conv.w_quant == 'fp':
            return None
        if conv.in_channels != self.out_channels or conv.groups != 1 or isinstance(conv.padding, str) or conv.padding_mode != 'zeros':
            return None
        if conv.weight.device != device or (bn is not None and bn.running_mean.device != device):
            return None                 # (a replica whose ``chain_next`` still names the original module, e.g. nn.DataParallel)
        if conv._alpha() <= 0 or conv.x_approximate.eval_scales(n) is not None:
            return None
        if bn is not None and (bn.training or not bn.track_running_stats):
            return None
        pre = None if bn is None else conv._folded_bn(bn)
        ph, pw = conv.padding
        words = n * (self.out_channels // 64) * (ho + 2 * ph) * (wo + 2 * pw)
        planes = conv._workspace('pre', (n, self.out_channels, ho, wo, ph, pw, device, _hip.stream_ptr(device)),
                                 lambda: torch.zeros((words,), dtype=torch.int64, device=device))   # zero halo; the interior is rewritten
        units = chain.accumulator(n, device)
        nxt = _hip.NextLs1(planes.data_ptr(), units.data_ptr(), None if pre is None else pre[0].data_ptr(),
                           None if pre is None else pre[1].data_ptr(), conv._alpha(), ph, pw)
        keep = (planes, units, pre)
        return nxt, chain.PreQuant(conv, bn, planes, units, (n, self.out_channels, ho, wo), _hip.stream_ptr(device)), keep

    def _proj_in_kernel(self, x: torch.Tensor, chain, sc: ProjectionShortcut) -> bool:
        """Whether this call ends in the plain XNOR launch that can compute the projection shortcut ``sc`` itself: binary
        activations, not a chained 1-bit layer, and an fp32 input with an fp32 ``sc.x`` (lsq_xnor_conv2d_proj) or, with
        ``xnor_half``, a 16-bit input with an ``sc.x`` of its type (lsq_xnor_conv2d_proj_half)."""
        if self.x_quant == 'fp' or (self.x_quant == 'ls-1' and chain.ENABLED):
            return False
        if x.dtype == torch.float32:
            return sc.x.dtype == torch.float32
        return self.xnor_half and sc.x.dtype == x.dtype

    def _forward_hip(self, x: torch.Tensor, pre_bn: Optional[nn.BatchNorm2d] = None, relu: bool = False,
                     res_pre: Optional[torch.Tensor] = None, res_post: Optional[torch.Tensor] = None,
                     prelu: Optional[torch.Tensor] = None, next_q: Optional[tuple] = None,
                     res_ready: Optional[torch.cuda.Event] = None) -> torch.Tensor:
        from quant import _hip
        from quant.binary import chain
        # a ProjectionShortcut in a residual slot: only the plain two-plane XNOR call at the end computes it itself (at most
        # one: the kernel has one residual array in registers); everywhere else it is a launch of its own, here
        proj = None
        if isinstance(res_post, ProjectionShortcut) and res_pre is None and self._proj_in_kernel(x, chain, res_post):
            proj, res_post = (res_post, True), None
        elif isinstance(res_pre, ProjectionShortcut) and self._proj_in_kernel(x, chain, res_pre):
            proj, res_pre = (res_pre, False), None
        if isinstance(res_pre, ProjectionShortcut):
            res_pre = res_pre.tensor()
        if isinstance(res_post, ProjectionShortcut):
            res_post = res_post.tensor()
        handed = chain.pending(x)                  # (an attribute of the tensor object: read before detach())
        x = x.detach()
        pre = None if pre_bn is None else self._folded_bn(pre_bn)
        n = x.shape[0]
        geom = self._geom_of(x, _hip)
        half_kernel = x.dtype != torch.float32 and self.x_quant == 'fp' and self.fp_half_kernel
        wbits, wsum, wscales, wprep = self._packed_weights(geom, _hip, prep=not half_kernel)
        ho, wo = _hip.out_hw(geom)
        res_pre = None if res_pre is None else res_pre.detach().contiguous()
        res_post = None if res_post is None else res_post.detach().contiguous()
        bias = None if self.bias is None else self.bias.detach()
        if half_kernel:
            # a 16-bit input with fp activations (fp_half): the samples as they are against the sign planes, the clamp bound as
            # Tensor.clamp would round it into their type; the kernel rounds its fp32 result once into the input's type
            return _hip.signw_conv2d_half(x.contiguous(), self._alpha_in(x.dtype), wbits, wscales, bias, geom)
        half_out = self.xnor_half and x.dtype != torch.float32 and self.x_quant != 'fp'      # (lsq_xnor_conv2d_half allocates its y)
        y = None if half_out else torch.empty((n, self.out_channels, ho, wo), dtype=torch.float32, device=x.device)
        def join():                      # residual operands from a side stream: in front of the convolution, behind the quantizer
            if res_ready is not None:
                torch.cuda.current_stream(x.device).wait_event(res_ready)
        if x.dtype != torch.float32:
            # a 16-bit input (act_half / fp_half): the samples are read as they are (or cast: the comparator), the clamp bound
            # as Tensor.clamp would round it into their type; the fp32 result is rounded once.  A folded batch norm only where
            # fused_forward hands one down (act_half_bn_fold: binary activations on lsq_act_quant_bn_half), no chaining; a
            # fused epilogue only with xnor_half (elsewhere fused_forward composes it in torch).
            x16 = x.contiguous()
            if self.x_quant == 'fp':          # (fp_half_kernel = False: the cast route, the comparator of DESIGN 4.19)
                _hip.signw_conv2d(x16.float(), self._alpha_in(x.dtype), wbits, wscales, bias, geom, y, wprep=wprep)
                return y.to(x.dtype)
            k = self.x_approximate.n_planes
            planes, scales = self._act_planes(x16 if self.act_half_kernel else x16.float(), geom, k, _hip,
                                              (geom.pad_h, geom.pad_w, self.groups, x.dtype), pre, alpha=self._alpha_in(x.dtype))
            self.last_act_scales = scales
            if half_out:
                # xnor_half: the 16-bit result straight from the convolution's epilogue, with whatever fused_forward handed
                # down (a plain forward hands nothing) -- the bits of the two lines below
                join()
                if proj is not None:
                    # a 16-bit projection shortcut (resnet.PROJ_HALF) computed in this launch's residual registers, never
                    # rounded on its own; refused: the shortcut as a 16-bit tensor in front (rounded there: other bits)
                    sc, post = proj
                    took, y16 = _hip.xnor_conv2d_proj_half(planes, k, scales, wbits, wsum, wscales, bias, geom,
                                                           (sc.x.contiguous(), sc.w, sc.b, sc.stride, post), x.dtype, relu,
                                                           res_pre, res_post, prelu)
                    if took:
                        return y16
                    if post:
                        res_post = sc.tensor()
                    else:
                        res_pre = sc.tensor()
                return _hip.xnor_conv2d_half(planes, k, scales, wbits, wsum, wscales, bias, geom, x.dtype, relu, res_pre,
                                             res_post, prelu)
            _hip.xnor_conv2d(planes, k, scales, wbits, wsum, wscales, bias, geom, y)
            return y.to(x.dtype)
        if self.x_quant == 'fp':
            join()
            _hip.signw_conv2d(x, self._alpha(), wbits, wscales, bias, geom, y, pre, relu, res_pre, res_post, prelu, wprep)
            return y
        xq = self.x_approximate
        k = xq.n_planes
        if self.x_quant == 'ls-1' and chain.ENABLED:
            # chained 1-bit layers: take the planes and row sums the producer's epilogue left for THIS call, and / or leave
            # the consumer's in this call's epilogue
            stream = _hip.stream_ptr(x.device)
            if not (handed is not None and handed.consumer is self and handed.pre_bn is pre_bn and handed.stream == stream
                    and handed.shape == tuple(x.shape) and xq.eval_scales(n) is None and self._alpha() > 0):
                handed = None
            target = self._chain_target(next_q, n, ho, wo, x.device, _hip)
            if handed is not None or target is not None:
                planes_in, scales_in, units_in = None, None, None
                if handed is not None:
                    planes_in, units_in = handed.planes, handed.units
                else:
                    planes_in, scales_in = self._act_planes(x, geom, k, _hip, (geom.pad_h, geom.pad_w, self.groups), pre)
                join()
                if _hip.xnor_conv2d_chain(planes_in, scales_in, units_in, self._alpha(), wbits, wsum, wscales, bias, geom, y,
                                          relu, res_pre, res_post, prelu, None if target is None else target[0]):
                    self.last_act_scales = scales_in          # (None when the scale came from the producer's row sums)
                    if target is not None:
                        chain.attach(y, target[1], target[2])
                    return y
                if handed is None and scales_in is not None:   # outside the matrix-core kernel: the plain call, same planes
                    _hip.xnor_conv2d(planes_in, k, scales_in, wbits, wsum, wscales, bias, geom, y, relu, res_pre, res_post, prelu)
                    self.last_act_scales = scales_in
                    return y
        planes, scales = self._act_planes(x, geom, k, _hip, (geom.pad_h, geom.pad_w, self.groups), pre)
        join()
        if proj is not None:
            sc, post = proj
            if _hip.xnor_conv2d_proj(planes, k, scales, wbits, wsum, wscales, bias, geom, y, (sc.x, sc.w, sc.b, sc.stride, post),
                                     relu, res_pre, res_post, prelu):
                self.last_act_scales = scales
                return y
            if post:                                     # refused: the two launches, same bits
                res_post = sc.tensor()
            else:
                res_pre = sc.tensor()
        _hip.xnor_conv2d(planes, k, scales, wbits, wsum, wscales, bias, geom, y, relu, res_pre, res_post, prelu)
        self.last_act_scales = scales
        return y
