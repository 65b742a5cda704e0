"""Host side of the depth networks' layers that run on hand-written HIP kernels: both depth nets (MiDaS, hourglass) and the
`--use_cnn` U-Net build their convolutions from this file.

  * the DVD_AB measurement switches and the fp16 activation storage's loss-scale state (`AB`, `GRAD_SCALE`);
  * element-wise and pooling layers: `bn_eval_relu`, `to_half`, `add_f16`, `upsample_bilinear2x`, `maxpool3s2`, `AvgPool2d`,
    the depth heads (`head1x1`, `head3x3`, `depth_tail`);
  * the 8-per-group 3x3 kernels (csrc/gconv.hip: the `conv2` of the ResNeXt-101 32x8d stage-1 bottlenecks,
    third_party/midas_blocks.py:35-50) and the legacy fp32 32-per-group ones (csrc/gconv32.hip, DVD_AB=gconv32);
  * the ResNeXt stem as a stride-1 5x5 convolution over the space-to-depth image (`stem_conv_bn_relu`);
  * dense and grouped 'same' convolutions on the split-operand MFMA kernels (csrc/xconv.hip, csrc/xwgrad3.hip): the packed
    weight cache and its per-step plan (`xconv_packed`, `xconv_packed_scaled`, `PACK_PLAN`), the launch (`_xconv_run`), the
    weight gradient (`xconv_wgrad`), the autograd Functions `_XConv` and `_XConvBn` (stride 1 and the native stride 2) with
    their fused gradient joins and ReLU-mask hand-over (`_Site`);
  * `_route`: the one place where a layer's hyper-parameters, the tensor and the AB switches become a choice of kernels, and
    the entry points that run it: `xconv2d`, `conv_bn_act`, `XConv2d` and its subclasses `GroupedConv3x3C8 / C16 / C32`.

Every module keeps the parameter names and shapes of the `nn.Conv2d` it replaces, so state_dicts interchange.  Tensors that
the kernels do not cover (CPU tensors of the oracle / tests, other dtypes) take the ATen ops; on a GPU in fp32 or fp16 the HIP
path is the one that runs.
"""
import collections
import ctypes
import os as _os
import weakref

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .ops import _p, _stream, _workspace, amax_of, chansum, known_amax, new_scalar, set_amax

# Same-box A/B measurement switches (previous-generation kernels / MIOpen against the kernels in use), read ONCE at
# import from DVD_AB="gconv32,no_alias,...".  Not product configuration: every default is the fastest measured path.
#   gconv32     32-per-group 3x3 on round 1's fp32-MFMA kernels (csrc/gconv32.hip) instead of the grouped xconv path
#   no_xwgrad3  dense weight gradients on the exact-fp32 MFMA kernel (csrc/xwgrad.hip)
#   no_alias    gradient joins of residual blocks by autograd's accumulation (ATen add) instead of the backward-data epilogue
#   no_maskfuse the ReLU mask of a BatchNorm+ReLU site always in the site's own mask pass (never in its consumer's epilogue)
#   no_s2       stride-2 3x3 convolutions as rounds 2-5 ran them: the stride-1 kernel's output sub-sampled, the gradient
#               zero-interleaved in HBM (csrc/pool.hip) in front of the stride-1 backward-data kernel
#   rowsum      bookkeeping only: the sites that run no pass of their own (see _XConvBn.backward: the default wherever the weight
#               gradient kernel delivers the per-channel sums) are counted as STATS['sites_no_pass'] instead of 'sites_premasked'.
#               (No key turns that default off: bench.py and the tests pin the six keys, so its A/B is against the parent build.)
AB = {k: False for k in ('gconv32', 'no_xwgrad3', 'no_alias', 'no_maskfuse', 'no_s2', 'rowsum')}
for _k in filter(None, _os.environ.get('DVD_AB', '').split(',')):
    if _k not in AB:
        raise RuntimeError('DVD_AB: unknown switch %r (known: %s)' % (_k, ', '.join(sorted(AB))))
    AB[_k] = True


# ---- fp16 activation storage (BASELINE configs[4]) ------------------------------------------------------------------
# Activations between the encoder stem and the depth head may be torch.float16 tensors: the same autograd Functions then call the
# "_h" / "_t" entry points (csrc/xconv.hip IN16 / OUT16, csrc/xwgrad3.hip H16, the templated helper kernels).  fp16 gradients
# carry the step's loss scale S (csrc/a16.hip); every PARAMETER gradient is multiplied by 1 / S where it is produced, so the
# flat gradient buffers hold true fp32 gradients.  The loss-scale state (16 floats on the device) belongs to the model that is
# stepping; it is registered here because the backward Functions need its address.
ACT_DTYPES = (torch.float32, torch.float16)
GRAD_SCALE = {'state': None}


def set_grad_scale_state(state):
    """state: the 16-float device tensor of dvd_gscale_* (or None).  Its address is baked into captured HIP graphs, so a model
    allocates it once and keeps it for its lifetime."""
    GRAD_SCALE['state'] = state


def _is16(t):
    return t.dtype == torch.float16


def _gs_state():
    st = GRAD_SCALE['state']
    if st is None:
        raise RuntimeError('fp16 gradients need a loss-scale state (conv.set_grad_scale_state; Model does it with --act_fp16)')
    return st


def _gs(i):
    """1-element view of the loss-scale state: 1 = 1 / S (out_scale of parameter gradients), 3 = observed max |S g|."""
    return _gs_state()[i:i + 1]


def _gscale_begin(gy, weight, n):
    """Start the backward pass's loss scale from max|g_out| and max|w| over the head's n weights (csrc/a16.hip) -> the state."""
    from .ops import amax
    state = _gs_state()
    _lib.check(_lib.load().dvd_gscale_begin(_p(state), _p(amax(gy)), _p(weight), n, _stream()), 'dvd_gscale_begin')
    return state


def _fwd_monitor():
    """Slot [6] of the loss-scale state: max |activation| that the fp16-output convolution epilogues and the depth head fold
    in during the forward pass (NaN as +Inf).  dvd_gscale_end skips the step when an activation left fp16's range: its Inf
    would otherwise reach the weight gradients (Inf x 0 = NaN) without any GRADIENT monitor seeing it.  None
    without a state (inference with fp16 activations outside a training model)."""
    st = GRAD_SCALE['state']
    return None if st is None else st[6:7]


class _BnRelu(torch.autograd.Function):
    """y = relu(bn_eval(x) (+ residual)); see csrc/bnrelu.hip."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, mean, var, eps, relu):
        x = x.contiguous()
        N, C = x.shape[0], x.shape[1]
        HW = x.numel() // (N * C)
        if residual is not None:
            residual = residual.contiguous()
        y = torch.empty_like(x)
        lib = _lib.load()
        # fp32 storage: max|y| from the same pass (the 1x1 convolution that follows takes its operand scale from it; until
        # round 6 a dvd_amax pass over y: 18 of them per step behind the 8- and 16-per-group and the strided convolutions)
        y_amax = None if _is16(x) else new_scalar(x.device)
        _lib.check(lib.dvd_bnrelu_fwd_m(_p(x), _p(residual), _p(gamma), _p(beta), _p(mean), _p(var), float(eps), _p(y),
                                        int(_is16(x)), N, C, HW, int(relu), _p(y_amax), _stream()), 'dvd_bnrelu_fwd')
        ctx.save_for_backward(x, y if relu else None, gamma, mean, var)
        ctx.cfg = (N, C, HW, float(eps), int(relu), residual is not None)
        if y_amax is not None:
            ctx.mark_non_differentiable(y_amax)
        return y, y_amax

    @staticmethod
    def backward(ctx, gy, _g_amax=None):
        x, y, gamma, mean, var = ctx.saved_tensors
        N, C, HW, eps, relu, has_res = ctx.cfg
        gy = gy.contiguous()
        need = ctx.needs_input_grad
        gx = torch.empty_like(x) if need[0] else None
        gr = torch.empty_like(x) if (has_res and need[1]) else None
        gg = torch.empty_like(gamma) if need[2] else None
        gb = torch.empty_like(gamma) if need[3] else None
        lib = _lib.load()
        ws = _workspace(lib.dvd_bnrelu_bwd_workspace_bytes(N, C, HW), x.device)
        h16 = _is16(gy)
        # fp32: max|gx| (and max|g| for the residual branch) come with the pass; the convolutions' backward found neither
        # attached and ran a dvd_amax pass each (12 per step)
        gx_amax = new_scalar(gy.device) if (gx is not None and not h16) else None
        gr_amax = new_scalar(gy.device) if (gr is not None and not h16) else None
        _lib.check(lib.dvd_bnrelu_bwd_m(_p(gy), _p(y), _p(x), _p(gamma), _p(mean), _p(var), eps, _p(gx), _p(gr), _p(gg),
                                        _p(gb), _p(ws), ctypes.c_size_t(ws.numel()), int(h16), _p(_gs(1)) if h16 else None, N, C,
                                        HW, relu, _p(_gs(3)) if h16 else _p(gr_amax), _p(gx_amax), _stream()), 'dvd_bnrelu_bwd')
        if gx_amax is not None:
            set_amax(gx, gx_amax)
        if gr_amax is not None:
            set_amax(gr, gr_amax)
        return gx, gr, gg, gb, None, None, None, None


def bn_eval_relu(bn, x, residual=None, relu=True):
    """relu(bn(x) (+ residual)) for an nn.BatchNorm2d in eval mode (running statistics; gamma / beta keep
    their gradients) on the fused HIP kernel; anything else (training-mode BN, CPU, other dtypes) takes the
    ATen ops the reference uses."""
    if (not bn.training and bn.track_running_stats and x.is_cuda and x.dtype in ACT_DTYPES):
        if bn.affine:
            gamma, beta = bn.weight, bn.bias
        else:                                   # hourglass inception blocks: BatchNorm2d(affine=False)
            gamma, beta = torch.ones_like(bn.running_mean), torch.zeros_like(bn.running_mean)
        y, y_amax = _BnRelu.apply(x, residual, gamma, beta, bn.running_mean, bn.running_var, bn.eps, relu)
        return set_amax(y, y_amax)
    y = bn(x)
    if residual is not None:
        y = y + residual
    return F.relu(y) if relu else y


class _ToHalf(torch.autograd.Function):
    """The fp32 -> fp16 boundary behind the encoder stem: forward casts; backward hands the fp32 stem the TRUE gradient, i.e.
    the fp16 gradient times 1 / (loss scale) (dvd_cast_scale_f32), so the stem's parameter gradients need no special case."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.float16)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        if g.numel() % 4:
            return g.float() * _gs(1)
        out = torch.empty(g.shape, device=g.device, dtype=torch.float32)
        _lib.check(_lib.load().dvd_cast_scale_f32(_p(g), 1, _p(out), ctypes.c_longlong(g.numel()), _p(_gs(1)), _stream()),
                   'dvd_cast_scale_f32')
        return out


def to_half(x):
    return _ToHalf.apply(x)


class _Head1x1(torch.autograd.Function):
    """`Conv2d(C, 1, 1)(relu(x))` of the depth head (third_party/MiDaS.py:192-194) with fp16 (or fp32) features and fp32
    output: the fp16 / fp32 boundary at the network's end.  Backward starts the pass's loss scale (dvd_gscale_begin from
    max|g_out| and max|w|), then writes the feature gradient times S in x's storage and the fp32 weight / bias gradients
    (csrc/a16.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu_in):
        x = x.contiguous()
        N, C, H, W = x.shape
        y = torch.empty(N, 1, H, W, device=x.device, dtype=torch.float32)
        # (fp16 features: the head output's max|y| goes to the forward monitor of the overflow guard, state[6])
        _lib.check(_lib.load().dvd_head1x1_fwd(_p(x), int(_is16(x)), _p(weight), _p(bias), _p(y),
                                               _p(_fwd_monitor()) if _is16(x) else None, N, C, H * W, int(bool(relu_in)),
                                               _stream()), 'dvd_head1x1_fwd')
        ctx.save_for_backward(x, weight)
        ctx.cfg = (bool(relu_in), bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        relu_in, has_bias = ctx.cfg
        gy = gy.contiguous().float()
        N, C, H, W = x.shape
        lib = _lib.load()
        h16 = _is16(x)
        state = _gscale_begin(gy, weight, C) if h16 else None
        gx = torch.empty_like(x)
        gw = torch.empty_like(weight)
        gb = torch.empty(1, device=x.device, dtype=torch.float32) if has_bias else None
        ws = _workspace(lib.dvd_head1x1_bwd_workspace_bytes(C), x.device)
        _lib.check(lib.dvd_head1x1_bwd(_p(x), int(h16), _p(weight), _p(gy), _p(state), _p(gx), _p(gw), _p(gb), _p(ws),
                                       ctypes.c_size_t(ws.numel()), N, C, H * W, int(relu_in), _stream()), 'dvd_head1x1_bwd')
        return gx, gw, gb, None


class _DepthTail(torch.autograd.Function):
    """`10000 / torch.clamp(relu(v), min=1e-2)` (third_party/MiDaS.py:192-195,240-242) as one HIP pass each way
    (csrc/elementwise.hip dvd_depth_tail_*): the forward value is torch's (reciprocal, then x 10000), the backward autograd's formula."""

    @staticmethod
    def forward(ctx, v):
        v = v.contiguous()
        out = torch.empty_like(v)
        _lib.check(_lib.load().dvd_depth_tail_fwd(_p(v), _p(out), v.numel(), _stream()), 'dvd_depth_tail_fwd')
        ctx.save_for_backward(v)
        return out

    @staticmethod
    def backward(ctx, g):
        v, = ctx.saved_tensors
        g = g.contiguous()
        gv = torch.empty_like(v)
        _lib.check(_lib.load().dvd_depth_tail_bwd(_p(v), _p(g), _p(gv), v.numel(), _stream()), 'dvd_depth_tail_bwd')
        return gv


def depth_tail(v):
    """10000 / clamp(relu(v), 1e-2): the HIP pass for fp32 GPU tensors, the reference's ATen expression otherwise."""
    if v.is_cuda and v.dtype == torch.float32:
        return _DepthTail.apply(v)
    return 10000 / torch.clamp(F.relu(v), min=1e-2)


def head1x1(conv, x, relu_in=True):
    """conv(relu(x)) for an nn.Conv2d(C, 1, 1) on the boundary kernel (GPU tensors, C <= 64, H * W % 4 == 0)."""
    return _Head1x1.apply(x, conv.weight, conv.bias, relu_in)


class _Head3x3(torch.autograd.Function):
    """`Conv2d(C, 1, 3, padding=1)(x)`, the hourglass's `pred_layer` (third_party/hourglass.py), with fp16 features and fp32
    output: the fp16 / fp32 boundary at that network's end, as _Head1x1 is for MiDaS.  Forward folds max|y| into the forward
    monitor (state[6]); backward starts the pass's loss scale (dvd_gscale_begin from max|g_out| and the head weights), then writes
    S * gx as fp16 and the unscaled fp32 weight / bias gradients (csrc/a16.hip dvd_head3x3_*)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        N, C, H, W = x.shape
        y = torch.empty(N, 1, H, W, device=x.device, dtype=torch.float32)
        _lib.check(_lib.load().dvd_head3x3_fwd(_p(x), _p(weight), _p(bias), _p(y), _p(_fwd_monitor()), N, C, H, W, _stream()),
                   'dvd_head3x3_fwd')
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous().float()
        N, C, H, W = x.shape
        lib = _lib.load()
        state = _gscale_begin(gy, weight, weight.numel())
        gx = torch.empty_like(x)
        gw = torch.empty_like(weight)
        gb = torch.empty(1, device=x.device, dtype=torch.float32) if ctx.has_bias else None
        ws = _workspace(lib.dvd_head3x3_bwd_workspace_bytes(N, C, H, W), x.device)
        _lib.check(lib.dvd_head3x3_bwd(_p(x), _p(weight), _p(gy), _p(state), _p(gx), _p(gw), _p(gb), _p(ws),
                                       ctypes.c_size_t(ws.numel()), N, C, H, W, _stream()), 'dvd_head3x3_bwd')
        return gx, gw, gb


def head3x3_supported(conv, x):
    """Is `conv` a Conv2d(C <= 64, 1, 3, padding 1) that the boundary kernels take for the fp16 GPU tensor x?"""
    return (x.is_cuda and _is16(x) and x.dim() == 4 and conv.out_channels == 1 and conv.in_channels <= 64 and
            conv.kernel_size == (3, 3) and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (1, 1) and
            tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros' and
            conv.weight.dtype == torch.float32)


def head3x3(conv, x):
    """conv(x) with fp16 features in and fp32 out, for a Conv2d(C, 1, 3, padding=1) (see head3x3_supported)."""
    if not head3x3_supported(conv, x):
        raise RuntimeError('head3x3: %r on a %s %s tensor is not the fp16 depth head' % (conv, x.device, x.dtype))
    return _Head3x3.apply(x, conv.weight, conv.bias)


class _AddF16(torch.autograd.Function):
    """a + b for fp16 GPU tensors on csrc/a16.hip (dvd_add_f16), max|a + b| folded into the forward monitor (state[6]) -- an
    fp16 sum can overflow where its summands did not, and the fused ReLUs downstream would hide the Inf from every later
    epilogue.  Backward hands the gradient to both summands."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        y = torch.empty_like(a)
        _lib.check(_lib.load().dvd_add_f16(_p(a), _p(b), _p(y), ctypes.c_longlong(a.numel()), _p(_fwd_monitor()), _stream()),
                   'dvd_add_f16')
        return y

    @staticmethod
    def backward(ctx, g):
        return g, g


def add_f16(a, b):
    """a + b of two fp16 GPU tensors of the same shape under the overflow guard (see _AddF16)."""
    if not (a.is_cuda and _is16(a) and _is16(b) and a.shape == b.shape and a.device == b.device):
        raise RuntimeError('add_f16: needs two fp16 GPU tensors of one shape (got %s %s, %s %s)' % (a.dtype, tuple(a.shape), b.dtype,
                                                                                                  tuple(b.shape)))
    return _AddF16.apply(a, b)


class _UpsampleBilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, out_hw, align_corners):
        x = x.contiguous()
        N, C, H, W = x.shape
        Ho, Wo = out_hw
        y = torch.empty(N, C, Ho, Wo, device=x.device, dtype=x.dtype)
        lib = _lib.load()
        _lib.check(lib.dvd_upsample_bilinear_fwd_t(_p(x), _p(y), int(_is16(x)), N * C, H, W, Ho, Wo, int(align_corners),
                                                   _stream()), 'dvd_upsample_bilinear_fwd')
        ctx.shape, ctx.align = (N, C, H, W, Ho, Wo), int(align_corners)
        return y

    @staticmethod
    def backward(ctx, gy):
        N, C, H, W, Ho, Wo = ctx.shape
        gy = gy.contiguous()
        gx = torch.empty(N, C, H, W, device=gy.device, dtype=gy.dtype)
        lib = _lib.load()
        _lib.check(lib.dvd_upsample_bilinear_bwd_t(_p(gy), _p(gx), int(_is16(gy)), N * C, H, W, Ho, Wo, ctx.align, _stream()),
                   'dvd_upsample_bilinear_bwd')
        return gx, None, None


def upsample_bilinear2x(x, align_corners):
    """F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=...) of the MiDaS decoder."""
    if x.is_cuda and x.dtype in ACT_DTYPES:
        y = _UpsampleBilinear.apply(x, (2 * x.shape[2], 2 * x.shape[3]), bool(align_corners))
        return set_amax(y, known_amax(x))            # a convex combination never exceeds the largest input magnitude
    return F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=align_corners)


class _GConv3x3C8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        x = x.contiguous()
        w = w.contiguous()
        N, C, H, W = x.shape
        y = torch.empty_like(x)
        lib = _lib.load()
        _lib.check(lib.dvd_gconv3x3_c8_fwd_t(_p(x), _p(w), _p(y), int(_is16(x)), N, C, H, W, _stream()), 'dvd_gconv3x3_c8_fwd')
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        N, C, H, W = x.shape
        lib = _lib.load()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _lib.check(lib.dvd_gconv3x3_c8_bwd_data_t(_p(gy), _p(w), _p(gx), int(_is16(gy)), N, C, H, W, _stream()),
                       'dvd_gconv3x3_c8_bwd_data')
        if ctx.needs_input_grad[1]:
            gw = torch.empty_like(w)
            nws = lib.dvd_gconv3x3_c8_wgrad_workspace_bytes(N, C, H, W)
            ws = _workspace(nws, x.device)
            h16 = _is16(gy)
            _lib.check(lib.dvd_gconv3x3_c8_bwd_weight_t(_p(x), _p(gy), _p(gw), 0, _p(ws), ctypes.c_size_t(ws.numel()), int(h16),
                                                        _p(_gs(1)) if h16 else None, N, C, H, W, _stream()),
                       'dvd_gconv3x3_c8_bwd_weight')
        return gx, gw


class _GConv3x3C32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        x = x.contiguous()
        w = w.contiguous()
        N, C, H, W = x.shape
        y = torch.empty_like(x)
        lib = _lib.load()
        ws = _workspace(lib.dvd_gconv3x3_c32_workspace_bytes(N, C, H, W), x.device)
        _lib.check(lib.dvd_gconv3x3_c32_fwd(_p(x), _p(w), _p(y), _p(ws), ctypes.c_size_t(ws.numel()), N, C, H, W,
                                            _stream()), 'dvd_gconv3x3_c32_fwd')
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        N, C, H, W = x.shape
        lib = _lib.load()
        ws = _workspace(lib.dvd_gconv3x3_c32_workspace_bytes(N, C, H, W), x.device)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            _lib.check(lib.dvd_gconv3x3_c32_bwd_data(_p(gy), _p(w), _p(gx), _p(ws), ctypes.c_size_t(ws.numel()), N, C, H,
                                                     W, _stream()), 'dvd_gconv3x3_c32_bwd_data')
        if ctx.needs_input_grad[1]:
            gw = torch.empty_like(w)
            _lib.check(lib.dvd_gconv3x3_c32_bwd_weight(_p(x), _p(gy), _p(gw), 0, _p(ws), ctypes.c_size_t(ws.numel()),
                                                       N, C, H, W, _stream()), 'dvd_gconv3x3_c32_bwd_weight')
        return gx, gw


def gconv3x3_c32(x, weight):
    """y = conv2d(x, weight, padding=1, groups=C // 32) for weight [C, 32, 3, 3] on the legacy kernels.  An entry for tests and
    tools/ (a bare weight, no module): the modules take _route."""
    if x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32:
        return _GConv3x3C32.apply(x, weight)
    return F.conv2d(x, weight, None, 1, 1, 1, x.shape[1] // 32)


# ---- the ResNeXt stem natively (round 4) ------------------------------------------------------------------------------
# `conv1 = Conv2d(3, 64, 7, stride 2, padding 3)` + `bn1` + ReLU + `MaxPool2d(3, 2, 1)` (torchvision's ResNet stem, reached
# through third_party/midas_blocks.py:35-45).  Round 3 left all four to ATen / MIOpen.  A stride-2 7x7 convolution is a
# STRIDE-1 convolution over the 2x2 space-to-depth image: with x'[4c + 2py + px][Y][X] = x[c][2Y + py][2X + px] and
# ky - 3 = 2a + py (a in -2..1), out[y][x] = sum w[c][ky][kx] x'[4c + 2py + px][y + a][x + b] -- a 4x4 kernel, embedded in a
# 5x5 "same" one (zero taps at a = 2 / b = 2).  That runs on the kernels this package already has: xconv (csrc/xconv.hip) with
# the eval-mode BatchNorm + ReLU in its epilogue, and the k x k weight gradient (xwgradk in csrc/xwgrad3.hip, KS = 5); the image
# needs no gradient.  The rearranged weight is a gather of the module's [64,3,7,7] parameter, so its gradient flows back through
# autograd's index backward and the state_dict keeps the reference's key and shape.
_S2D_IDX = {}


def _s2d_index(device):
    key = str(device)
    if key not in _S2D_IDX:
        idx = torch.full((2, 2, 5, 5), 49, dtype=torch.long)
        for py in range(2):
            for a in range(-2, 3):
                ky = 2 * a + py + 3
                if not 0 <= ky <= 6:
                    continue
                for px in range(2):
                    for b in range(-2, 3):
                        kx = 2 * b + px + 3
                        if 0 <= kx <= 6:
                            idx[py, px, a + 2, b + 2] = ky * 7 + kx
        _S2D_IDX[key] = idx.reshape(-1).to(device)
    return _S2D_IDX[key]


def s2d_weight(w):
    """[Cout, C, 7, 7] (stride 2, padding 3) -> the equivalent [Cout, 4C, 5, 5] (stride 1, padding 2) over pixel_unshuffle(x, 2)."""
    Co, C = w.shape[0], w.shape[1]
    w_ext = torch.cat([w.reshape(Co, C, 49), w.new_zeros(Co, C, 1)], 2)
    return w_ext.index_select(2, _s2d_index(w.device)).reshape(Co, C * 4, 5, 5)


def is_resnet_stem(conv, bn):
    """The 7x7 / stride 2 / padding 3 convolution + eval-mode BatchNorm that stem_conv_bn_relu implements (any other stem
    stays on ATen: MidasNet.forward checks this before it takes the native path -- ADVICE round 4)."""
    return (isinstance(conv, torch.nn.Conv2d) and isinstance(bn, torch.nn.BatchNorm2d) and conv.kernel_size == (7, 7) and
            conv.stride == (2, 2) and conv.padding == (3, 3) and conv.groups == 1 and conv.dilation == (1, 1) and
            not bn.training and bn.track_running_stats)


def stem_conv_bn_relu(conv, bn, x):
    """relu(bn(conv(x))) for the 7x7 / stride 2 / padding 3 stem convolution and its eval-mode BatchNorm, GPU fp32 tensors."""
    if not is_resnet_stem(conv, bn):
        raise RuntimeError('stem_conv_bn_relu: not the ResNet stem (%r)' % (conv,))
    H, W = x.shape[2], x.shape[3]
    if H % 2 or W % 2:                    # the zero row / column the convolution's padding would have supplied
        x = F.pad(x, (0, W % 2, 0, H % 2))
    x4 = F.pixel_unshuffle(x, 2).contiguous()
    w5 = s2d_weight(conv.weight)
    gamma, beta = (bn.weight, bn.bias) if bn.affine else (None, None)
    out_site = _Site()
    y, y_amax = _XConvBn.apply(x4, amax_of(x4), w5, conv.bias, gamma, beta, bn.running_mean, bn.running_var, bn.eps, None, True,
                               1, False, None, out_site)
    y._dvd_site = out_site
    return set_amax(y, y_amax)


class _MaxPool3s2(torch.autograd.Function):
    """nn.MaxPool2d(3, 2, 1) on csrc/pool.hip (ATen's tie rule; deterministic gather backward).  to_half: the output is
    written as fp16 -- the fp32 / fp16 boundary of fp16 activation storage, fused into the pooling; the backward then hands
    the fp32 stem the TRUE gradient (fp16 gradient times 1 / loss scale)."""

    @staticmethod
    def forward(ctx, x, to_half):
        x = x.contiguous()
        N, C, H, W = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty(N, C, Ho, Wo, device=x.device, dtype=torch.float16 if to_half else torch.float32)
        idx = torch.empty(N, C, Ho, Wo, device=x.device, dtype=torch.uint8)
        _lib.check(_lib.load().dvd_maxpool3s2_fwd(_p(x), _p(y), int(bool(to_half)), _p(idx), ctypes.c_longlong(N * C), H, W,
                                                  _stream()), 'dvd_maxpool3s2_fwd')
        ctx.save_for_backward(idx)
        ctx.shape = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        idx, = ctx.saved_tensors
        N, C, H, W = ctx.shape
        gy = gy.contiguous()
        h16 = _is16(gy)
        gx = torch.empty(N, C, H, W, device=gy.device, dtype=torch.float32)
        _lib.check(_lib.load().dvd_maxpool3s2_bwd(_p(gy), int(h16), _p(idx), _p(gx), _p(_gs(1)) if h16 else None,
                                                  ctypes.c_longlong(N * C), H, W, _stream()), 'dvd_maxpool3s2_bwd')
        return gx, None


def maxpool3s2(x, to_half=False):
    y = _MaxPool3s2.apply(x, bool(to_half))
    return y if to_half else set_amax(y, known_amax(x))      # a maximum of inputs never exceeds the largest input magnitude


def add_bounded(a, b):
    """a + b; when both operands carry a max|.| scalar the sum's bound is their sum (one tiny kernel instead of a reduction
    pass over the sum when it feeds a convolution)."""
    y = a + b
    ka, kb = known_amax(a), known_amax(b)
    return set_amax(y, ka + kb) if (ka is not None and kb is not None) else y


class _Subsample2(torch.autograd.Function):
    """x[:, :, ::2, ::2] as a contiguous tensor on csrc/pool.hip (dvd_subsample2_*): one gather forward, one zero-interleaving
    pass backward (ATen: a strided copy; a fill and a strided copy)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        N, C, H, W = x.shape
        y = torch.empty(N, C, (H + 1) // 2, (W + 1) // 2, device=x.device, dtype=x.dtype)
        _lib.check(_lib.load().dvd_subsample2_fwd(_p(x), _p(y), int(_is16(x)), N * C, H, W, _stream()), 'dvd_subsample2_fwd')
        ctx.shape = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        N, C, H, W = ctx.shape
        gy = gy.contiguous()
        gx = torch.empty(N, C, H, W, device=gy.device, dtype=gy.dtype)
        _lib.check(_lib.load().dvd_subsample2_bwd(_p(gy), _p(gx), int(_is16(gy)), N * C, H, W, _stream()), 'dvd_subsample2_bwd')
        k = known_amax(gy)
        return gx if k is None else set_amax(gx, k)


def _subsample(t, st):
    """t[:, :, ::st, ::st] as a contiguous tensor; max|t| stays an upper bound of the result's."""
    if st == 2 and t.is_cuda and t.dtype in ACT_DTYPES and t.dim() == 4:
        y = _Subsample2.apply(t)
    else:
        y = t[:, :, ::st, ::st].contiguous()
    k = known_amax(t)                     # the producer's bound if there is one; else reduce the (st^2 x smaller) result
    return set_amax(y, k) if k is not None else y


class _AvgPool(torch.autograd.Function):
    """F.avg_pool2d(x, k, stride, pad) with PyTorch's defaults on csrc/pool.hip (dvd_avgpool_*; ATen's arithmetic)."""

    @staticmethod
    def forward(ctx, x, k, st, pad):
        x = x.contiguous()
        N, C, H, W = x.shape
        Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
        y = torch.empty(N, C, Ho, Wo, device=x.device, dtype=x.dtype)
        _lib.check(_lib.load().dvd_avgpool_fwd(_p(x), _p(y), int(_is16(x)), N * C, H, W, k, st, pad, _stream()), 'dvd_avgpool_fwd')
        ctx.cfg = (N, C, H, W, k, st, pad)
        return y

    @staticmethod
    def backward(ctx, gy):
        N, C, H, W, k, st, pad = ctx.cfg
        gy = gy.contiguous()
        gx = torch.empty(N, C, H, W, device=gy.device, dtype=gy.dtype)
        _lib.check(_lib.load().dvd_avgpool_bwd(_p(gy), _p(gx), int(_is16(gy)), N * C, H, W, k, st, pad, _stream()), 'dvd_avgpool_bwd')
        # at most ceil(k / st)^2 windows of weight 1 / k^2 hold a pixel: |gx| <= ceil(k / st)^2 / k^2 * max|gy| <= max|gy|.  Attained
        # only for stride 1 (AvgPool2d(2): a quarter, AvgPool2d(3, 2, 1): 4 / 9 of it), there up to the rounding of the summed
        # quotients gy / k^2 -- ulps, far inside the two bits of headroom pow2_scale leaves (tests/test_41_operand_scales_gpu.py)
        kg = known_amax(gy)
        return (gx if kg is None else set_amax(gx, kg)), None, None, None


class AvgPool2d(nn.AvgPool2d):
    """Drop-in nn.AvgPool2d: GPU fp32 / fp16 tensors of the default configuration (floor mode, count_include_pad, square
    window, 2 * padding <= kernel) run on csrc/pool.hip -- the hourglass's AvgPool2d(2) (third_party/hourglass.py:60-158) and
    FCNUnet's AvgPool2d(3, 2, 1) (networks/FCNUnet.py:64); everything else, and CPU tensors, take ATen."""

    def forward(self, x):
        def one(v):
            return v if isinstance(v, int) else (v[0] if v[0] == v[1] else None)
        k, st, pad = one(self.kernel_size), one(self.stride), one(self.padding)
        if (x.is_cuda and x.dtype in ACT_DTYPES and x.dim() == 4 and None not in (k, st, pad) and not self.ceil_mode and
                self.count_include_pad and self.divisor_override is None and 1 <= k <= 7 and 2 * pad <= k):
            y = _AvgPool.apply(x, k, st, pad)
            # an average of inputs (and padding zeros) never exceeds the largest magnitude -- up to the k^2 roundings of the window
            # sum: a window of equal extremes can come out k^2 ulps above them for k >= 3 (never for the hourglass's k = 2).  The
            # two bits of headroom pow2_scale leaves absorb that (tests/test_41_operand_scales_gpu.py)
            kx = known_amax(x)
            return y if kx is None else set_amax(y, kx)
        return super().forward(x)


def _pair_groups_of_16(weight):
    """[C,16,3,3] (16 channels per group) -> the equivalent [C,32,3,3] with groups paired into blocks of 32
    channels and zeros off the 16x16 diagonal blocks (exact: the extra products are with 0.0)."""
    C = weight.shape[0]
    w = weight.view(C // 32, 2, 16, 16, 3, 3)
    w32 = weight.new_zeros(C // 32, 2, 16, 2, 16, 3, 3)
    w32[:, 0, :, 0] = w[:, 0]
    w32[:, 1, :, 1] = w[:, 1]
    return w32.view(C, 32, 3, 3)


def gconv3x3_c8(x, weight):
    """y = conv2d(x, weight, padding=1, groups=C // 8) for weight [C, 8, 3, 3].  An entry for tests and tools/ (a bare weight,
    no module): the modules take _route."""
    if x.is_cuda and x.dtype in ACT_DTYPES and weight.dtype == torch.float32:
        return _GConv3x3C8.apply(x, weight)
    return F.conv2d(x, weight, None, 1, 1, 1, x.shape[1] // 8)


# ---------------------------------------------------------------------------------------
# Dense stride-1 convolutions on the split-operand MFMA kernels (csrc/xconv.hip; two fp16 terms per operand, csrc/dvd_split.h)

class _PackPlan(object):
    """Every packing a captured depth-net graph needs, made by TWO launches per optimiser step (dvd_xconv_pack_many) instead
    of two per weight tensor and per captured chunk (round 5: 964 launches, 6.3 ms of a 668 ms step).

    Eager calls of xconv_packed / xconv_packed_scaled (the warm-up passes before a capture) leave a REQUEST on the weight;
    `extend()` -- called by the model right before it opens a capture -- gives every requested packing a persistent buffer and
    a row of the device table; under capture xconv_packed then returns that buffer and launches nothing.  The buffers hold
    the packing of the weights' CURRENT values only after `ensure_current()`: the owner of the graphs calls it before every
    replay (it compares version counters / the fused Adam's epoch on the host and launches only after a change).
    Entries hold weak references: a discarded model's rows are dropped at the next extend()."""

    def __init__(self):
        self.requests = {}                    # id(weight) -> weak reference: weights with a '_dvd_pack_req' not taken yet
        self.entries = []
        self.items = None
        self.table = None
        self.key = None
        self.dirty = False
        self.launches = 0                     # (tests / bench read it)

    def request(self, weight, kind, groups, gamma=None, var=None, eps=0.0):
        planned = getattr(weight, '_dvd_plan', None)
        if planned is not None and kind in planned:
            e = planned[kind]
            if kind != 'Ts' or (e['gamma']() is gamma and e['var']() is var and e['eps'] == float(eps)):
                return
        req = getattr(weight, '_dvd_pack_req', None)
        if req is None:
            req = {}
            weight._dvd_pack_req = req
        req[kind] = (int(groups), gamma, var, float(eps))
        if id(weight) not in self.requests:
            key = id(weight)
            self.requests[key] = weakref.ref(weight, lambda _r, key=key, reqs=self.requests: reqs.pop(key, None))

    @staticmethod
    def _ref(t):
        return weakref.ref(t) if t is not None else (lambda: None)

    def extend(self):
        """Take the pending requests (not during a capture) and bring every buffer up to date."""
        if torch.cuda.is_current_stream_capturing():
            return
        lib = _lib.load()
        live =[e for e in self.entries if e['w']() is not None]
        if len(live) != len(self.entries):
            self.entries, self.dirty = live, True
        for ref in list(self.requests.values()):
            weight = ref()
            if weight is None:
                continue
            req = getattr(weight, '_dvd_pack_req', None) or {}
            planned = getattr(weight, '_dvd_plan', None)
            if planned is None:
                planned = {}
                weight._dvd_plan = planned
            Cout, Cin, KS, _ = weight.shape
            for kind, (groups, gamma, var, eps) in req.items():
                transposed = kind != 'F'
                nbytes = lib.dvd_xconv_packed_bytes(Cout, Cin * groups, KS, groups, int(transposed))
                if nbytes == 0 or not weight.is_contiguous() or weight.dtype != torch.float32:
                    continue
                old = planned.get(kind)
                if old is not None:
                    self.entries = [e for e in self.entries if e is not old]
                e = dict(w=weakref.ref(weight), kind=kind, groups=groups, gamma=self._ref(gamma), var=self._ref(var), eps=eps,
                         packed=torch.empty(nbytes, device=weight.device, dtype=torch.uint8), shape=(Cout, Cin * groups, KS))
                planned[kind] = e
                self.entries.append(e)
                self.dirty = True
            weight._dvd_pack_req = None
        self.requests.clear()
        self.ensure_current()

    @staticmethod
    def _entry_state(e):
        """(addresses, versions) of an entry's tensors, or None if its weight is gone."""
        w, g, v = e['w'](), e['gamma'](), e['var']()
        if w is None:
            return None
        return ((w.data_ptr(), None if g is None else g.data_ptr(), None if v is None else v.data_ptr()),
                (w._version, None if g is None else g._version, None if v is None else v._version))

    def ensure_current(self):
        """Re-pack if any planned weight (or BatchNorm scale) changed since the last packing.  Host cost: one tuple of version
        counters per entry; device cost: two launches after an optimiser step, none otherwise."""
        if not self.entries:
            return
        from . import ops
        states = [self._entry_state(e) for e in self.entries]
        if any(st is None for st in states):
            self.entries = [e for e, st in zip(self.entries, states) if st is not None]
            states = [st for st in states if st is not None]
            self.dirty = True
            if not self.entries:
                return
        addresses = tuple(st[0] for st in states)
        key = (ops.WEIGHT_EPOCH[0], addresses, tuple(st[1] for st in states))
        if key == self.key and not self.dirty:
            return
        lib = _lib.load()
        n = len(self.entries)
        upload = int(self.dirty or self.items is None or self.key is None or addresses != self.key[1])
        if upload:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('xconv pack plan: the item table changed during a graph capture (call extend() before it)')
            items = (_lib.XPackItem * n)()
            for i, e in enumerate(self.entries):
                Cout, Cin, KS = e['shape']
                wp, gp, vp = addresses[i]
                items[i] = _lib.XPackItem(wp, e['packed'].data_ptr(), gp, vp, e['eps'], Cout, Cin, KS, e['groups'],
                                          int(e['kind'] != 'F'))
            self.items = items
            self.table = torch.empty(lib.dvd_xconv_pack_table_bytes(n), device=self.entries[0]['packed'].device,
                                     dtype=torch.uint8)
        _lib.check(lib.dvd_xconv_pack_many(ctypes.cast(self.items, ctypes.c_void_p), n, _p(self.table),
                                           ctypes.c_size_t(self.table.numel()), upload, _stream()), 'dvd_xconv_pack_many')
        self.key, self.dirty = key, False
        self.launches += 1

    def lookup(self, weight, kind, gamma=None, var=None, eps=0.0):
        planned = getattr(weight, '_dvd_plan', None)
        e = planned.get(kind) if planned is not None else None
        if e is None or e['w']() is not weight:
            return None
        if kind == 'Ts' and not (e['gamma']() is gamma and e['var']() is var and e['eps'] == float(eps)):
            return None
        return e['packed']


PACK_PLAN = _PackPlan()


def _xconv_packed(weight, kind, groups, gamma=None, var=None, eps=0.0):
    """The packed copy of `weight` of one of the plan's kinds: 'F' forward, 'T' transposed (backward-data), 'Ts' transposed with
    row co scaled by gamma[co] / sqrt(var[co] + eps).  Eager calls are served from a cache that hangs on the weight tensor
    OBJECT (not on its address: allocators reuse addresses), one buffer per kind, re-packed in place when the key changed."""
    from . import ops
    w = weight.detach()
    if not w.is_contiguous():
        w = w.contiguous()
    Cout, Cin, KS, _ = w.shape
    Cin *= groups
    lib = _lib.load()
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing:
        planned = PACK_PLAN.lookup(weight, kind, gamma, var, eps)
        if planned is not None:             # kept current by the graph's owner (PACK_PLAN.ensure_current before a replay)
            return planned
    else:
        PACK_PLAN.request(weight, kind, groups, gamma, var, eps)
    # HIP-graph capture without a plan entry: the pack launch must be PART of the graph (a replay runs no Python, and the
    # weights change between replays), into a buffer of the graph's own pool -- the cache is neither read nor filled
    hit = None
    if not capturing:
        key = (w.data_ptr(), weight._version, ops.WEIGHT_EPOCH[0], tuple(w.shape))
        if kind == 'Ts':                    # ... also follows gamma (optimiser steps) and the running variance
            key += (None if gamma is None else (gamma.data_ptr(), gamma._version), var.data_ptr(), var._version, float(eps))
        cache = getattr(weight, '_dvd_xpack', None)
        if cache is None:
            cache = weight._dvd_xpack = {}
        hit = cache.get(kind)
        if hit is not None and hit[0] == key:
            return hit[1]
    nbytes = lib.dvd_xconv_packed_bytes(Cout, Cin, KS, groups, int(kind != 'F'))
    if nbytes == 0:
        raise RuntimeError('xconv: unsupported weight shape %s' % (tuple(w.shape),))
    packed = hit[1] if (hit is not None and hit[1].numel() == nbytes) else torch.empty(nbytes, device=w.device, dtype=torch.uint8)
    if kind == 'Ts':
        _lib.check(lib.dvd_xconv_pack_scaled(_p(w), _p(packed), Cout, Cin, KS, groups, 1, _p(gamma), _p(var), float(eps),
                                             _stream()), 'dvd_xconv_pack_scaled')
    else:
        _lib.check(lib.dvd_xconv_pack(_p(w), _p(packed), Cout, Cin, KS, groups, int(kind == 'T'), _stream()), 'dvd_xconv_pack')
    if not capturing:
        cache[kind] = (key, packed)
    return packed


def xconv_packed(weight, transposed, groups=1):
    """Fragment-ordered, pre-split copy of a conv weight [Cout,Cin/groups,k,k], rebuilt when the weight changed: new storage,
    autograd version counter, or an optimiser step of the fused Adam (ops.WEIGHT_EPOCH)."""
    return _xconv_packed(weight, 'T' if transposed else 'F', groups)


def xconv_packed_scaled(weight, groups, gamma, var, eps):
    """Transposed packing with row co scaled by gamma[co] / sqrt(var[co] + eps): backward-data through a fused BatchNorm."""
    return _xconv_packed(weight, 'Ts', groups, gamma, var, eps)


def _xconv_run(x, packed, Cout, KS, bias=None, residual=None, mask_src=None, relu_in=False, relu_out=False,
               res_relu=False, groups=1, bn=None, x_amax=None, y_amax=None, stride=1, out_hw=None):
    """bn = (gamma | None, beta | None, mean, var, eps): eval-mode BatchNorm of the output, fused into the epilogue.
    x_amax: the input's max|x| scalar (computed here if not given); y_amax: optional zeroed 1-element tensor that
    receives max|y|.  stride 2: the 3x3 / stride 2 / padding 1 forward; stride -2: its backward-data pass (x is the gradient
    of the strided output, out_hw the full-resolution height and width), see include/dvd_hip.h."""
    N, Cin, H, W = x.shape
    h16 = _is16(x)
    if x_amax is None and not h16:
        x_amax = amax_of(x)
    flags = int(bool(relu_in)) | (int(bool(relu_out)) << 1) | (int(bool(res_relu)) << 2)
    if stride == 2:
        y = torch.empty(N, Cout, (H + 1) // 2, (W + 1) // 2, device=x.device, dtype=x.dtype)
        flags |= 8
    elif stride == -2:
        if ((out_hw[0] + 1) // 2, (out_hw[1] + 1) // 2) != (H, W):
            raise RuntimeError('xconv: a %dx%d gradient is not the stride-2 image of %dx%d' % (H, W, out_hw[0], out_hw[1]))
        H, W = int(out_hw[0]), int(out_hw[1])
        y = torch.empty(N, Cout, H, W, device=x.device, dtype=x.dtype)
        flags |= 16
    else:
        y = torch.empty(N, Cout, H, W, device=x.device, dtype=x.dtype)
    lib = _lib.load()
    bnp = None
    if bn is not None:
        g, b, m, v, eps = bn
        bnp = ctypes.byref(_lib.BnParams(g.data_ptr() if g is not None else None, b.data_ptr() if b is not None else None,
                                         m.data_ptr(), v.data_ptr(), float(eps)))
    if h16:        # fp16 activations: no operand scale, two MFMAs per product (csrc/xconv.hip IN16 / OUT16)
        for t, name in ((residual, 'residual'), (mask_src, 'mask source')):
            if t is not None and not _is16(t):
                raise RuntimeError('xconv: fp16 convolution with an fp32 %s' % name)
        _lib.check(lib.dvd_xconv_fwd_h(_p(x), _p(packed), _p(bias), _p(residual), _p(mask_src), bnp, _p(y), _p(y_amax), N, Cin,
                                       Cout, H, W, KS, groups, flags, 1, _stream()), 'dvd_xconv_fwd_h')
        return y
    _lib.check(lib.dvd_xconv_fwd(_p(x), _p(x_amax), _p(packed), _p(bias), _p(residual), _p(mask_src), bnp, _p(y), _p(y_amax),
                                 N, Cin, Cout, H, W, KS, groups, flags, _stream()), 'dvd_xconv_fwd')
    return y


STATS = {'sites_premasked': 0, 'sites_masked': 0, 'sites_no_pass': 0}      # how many BatchNorm+ReLU sites took which backward (tests read it)


class _Site(object):
    """Hand-over between a BatchNorm+ReLU site and the convolution that consumes its output (round 3).  The site's backward
    needs g = gy * [y > 0]; the consumer's backward-data kernel PRODUCES gy and has y in hand (its own saved input), so it
    applies the mask in its epilogue (`mask_src`) and records which tensor it wrote.  If the gradient the site receives is
    exactly that tensor, unmodified (same storage address, same version counter: autograd neither replaced it by a sum nor
    accumulated into it), the site's mask pass shrinks to the per-channel sums (4 instead of 12 bytes per element).  Masking
    is idempotent, so a consumer that masks although the site will mask again (several consumers) costs time, never
    correctness; the proof obligation sits with the site alone."""
    __slots__ = ('ref', 'version', 'amax')

    def __init__(self):
        self.ref, self.version, self.amax = None, -1, None

    def wrote(self, g, amax=None):
        """amax: the device scalar max|g| the writing kernel's epilogue produced (the site's operand scale).
        The hand-over is by tensor OBJECT (a weak reference), not by address: a sum (gA + gB) + gC that the allocator
        happens to place at a freed gA's address has version 0 like every kernel-written tensor, but it is another object."""
        self.ref, self.version, self.amax = weakref.ref(g), g._version, amax

    def is_exactly(self, g):
        return self.ref is not None and self.ref() is g and self.version == g._version


def _fwd_amax(ctx, x):
    """Where a forward epilogue leaves max|y| -> (the scalar the Function returns beside y | None, the slot the kernel writes).
    fp32: a fresh scalar, a non-differentiable output; fp16 activations carry no operand scale: their epilogue folds max|y| into
    the overflow guard's forward monitor."""
    if _is16(x):
        return None, _fwd_monitor()
    y_amax = new_scalar(x.device)
    ctx.mark_non_differentiable(y_amax)
    return y_amax, y_amax


def _gy_reductions(gy, want_gb, want_amax):
    """What a backward reads off the output gradient before its gradient kernels run -> (bias gradient | None, max|gy| | None):
    the bias gradient and (if nobody attached it) max|gy| from ONE read of gy (rounds 1-5: ATen sum + dvd_amax); one max|gy|,
    shared by both gradient kernels.  No bias gradient from here for fp16 or non-GPU gradients: _bias_grad_sum."""
    gb = None
    if want_gb and gy.is_cuda and gy.dtype == torch.float32 and gy.dim() == 4:
        gb = chansum(gy, want_amax=want_amax and known_amax(gy) is None)
    return gb, (amax_of(gy) if want_amax else None)


def _bias_grad_sum(gy):
    """The bias gradient where dvd_chansum does not serve (fp16 gradients carry the loss scale: times 1 / S)."""
    return gy.sum((0, 2, 3), dtype=torch.float32) * _gs(1) if _is16(gy) else gy.sum((0, 2, 3))


def _xconv_bwd_data(ctx, g, g_amax, weight, groups, mask_src, g_alias=None, bn_scale=None, **strided):
    """The backward-data launch of the two xconv Functions and what goes with it: max|gx| comes from the epilogue (fp16: into
    the loss-scale policy's observed maximum) and is attached to gx (used by the next backward if autograd hands this very
    tensor on); the BatchNorm+ReLU site x came from is told which tensor carries its mask (see _Site).  g_alias: the gradient of
    x's other consumers, added in the epilogue; bn_scale = (gamma, var, eps): through a fused BatchNorm; strided: see _strided_bwd."""
    h16 = _is16(g)
    gx_amax = _gs(3) if h16 else new_scalar(g.device)
    packed = xconv_packed(weight, True, groups) if bn_scale is None else xconv_packed_scaled(weight, groups, *bn_scale)
    gx = _xconv_run(g, packed, weight.shape[1] * groups, weight.shape[2], mask_src=mask_src, groups=groups, x_amax=g_amax,
                    y_amax=gx_amax, residual=g_alias.contiguous() if g_alias is not None else None, **strided)
    if not h16:
        set_amax(gx, gx_amax)
    if ctx.in_site is not None:
        ctx.in_site.wrote(gx, None if h16 else gx_amax)
    return gx


def _strided(stride):
    """The keyword that _xconv_run's forward and xconv_wgrad take for a stride-2 convolution (nothing at stride 1)."""
    return {'stride': 2} if stride == 2 else {}


def _strided_bwd(stride, x):
    """_xconv_run's keywords for the backward-data pass of a stride-2 convolution of x: the kernel reads the compact gradient as
    if it were zero-interleaved (csrc/xconv.hip XArgs::ZI) and writes x's resolution."""
    return dict(stride=-2, out_hw=(x.shape[2], x.shape[3])) if stride == 2 else {}


class _XConv(torch.autograd.Function):
    """y = conv2d(act(x), w, stride 1, padding k//2) + bias + res'   with act = ReLU or identity and
    res' = residual or relu(residual).  Forward and backward-data on csrc/xconv.hip; backward-weight on
    csrc/xwgrad3.hip (deterministic).

    stride=2: y = conv2d(x, w, bias, stride 2, padding 1) for a 3x3 kernel with whole 16-channel chunks per group
    (torchvision's Bottleneck.conv2 at the entry of ResNeXt stages 2-4, third_party/midas_blocks.py:35-50), without ReLU,
    residual or alias: the forward stages the haloed input tile as four phase planes (csrc/xconv.hip XArgs::S2), the
    backward-data kernel reads the compact gradient (_strided_bwd), the weight gradient takes it zero-interleaved (xconv_wgrad).

    Fused gradient joins (round 3).  `alias`: the Function also returns its input as a second differentiable output; the
    OTHER consumers of x (a residual connection, a shortcut convolution) take that alias instead of x, so their gradient
    arrives HERE, as an argument of backward, and is added in the backward-data kernel's epilogue (`residual` operand) --
    autograd's own accumulation (an ATen add over the whole tensor: read 8, write 4 bytes per element) never runs.  With
    relu_in the epilogue masks AFTER the add, (dgrad + g_alias) * [x > 0], so the alias's consumer must hand over its
    gradient UNMASKED: that is `res_unmasked` on the consuming convolution, whose residual is relu(alias) (the
    ResidualConvUnit of the MiDaS decoder: both terms carry the same mask [x > 0])."""

    @staticmethod
    def forward(ctx, x, x_amax, weight, bias, residual, relu_in, res_relu, groups=1, alias=False, res_unmasked=False,
                in_site=None, stride=1):
        if stride == 2 and (residual is not None or relu_in or alias):
            raise RuntimeError('xconv: the stride-2 forms take no residual, input ReLU or alias')
        ctx.set_materialize_grads(False)
        ctx.in_site = in_site if (in_site is not None and not relu_in and not AB['no_maskfuse']) else None
        x = x.contiguous()
        if residual is not None:
            residual = residual.contiguous()
        Cout, _, KS, _ = weight.shape
        y_amax, amax_slot = _fwd_amax(ctx, x)
        y = _xconv_run(x, xconv_packed(weight, False, groups), Cout, KS, bias=bias, residual=residual, relu_in=relu_in,
                       res_relu=res_relu, groups=groups, x_amax=x_amax, y_amax=amax_slot, **_strided(stride))
        ctx.save_for_backward(x, residual if (res_relu and not res_unmasked) else None, x_amax)
        ctx.wparam = weight          # the tensor object that carries the packed copies
        ctx.cfg = (bool(relu_in), bool(res_relu), bias is not None, residual is not None, groups, bool(res_unmasked), int(stride))
        if alias:
            return y, y_amax, x
        return y, y_amax

    @staticmethod
    def backward(ctx, gy, _g_amax, g_alias=None):
        x, residual, x_amax = ctx.saved_tensors
        weight = ctx.wparam
        relu_in, res_relu, has_bias, has_res, groups, res_unmasked, stride = ctx.cfg
        if gy is None:                      # only the alias was used downstream
            return (g_alias,) + (None,) * 11
        gy = gy.contiguous()
        need = ctx.needs_input_grad
        gx = gw = gr = None
        gb, g_amax = _gy_reductions(gy, has_bias and need[3], (need[0] or need[2]) and not _is16(gy))
        if need[0]:
            # the mask [x > 0]: of the fused input ReLU, or of the BatchNorm+ReLU site whose output x is (ReLU is already applied)
            gx = _xconv_bwd_data(ctx, gy, g_amax, weight, groups, x if (relu_in or ctx.in_site is not None) else None, g_alias,
                                 **_strided_bwd(stride, x))
        if need[2]:
            gw = xconv_wgrad(x, gy, weight.shape, relu_in, groups, x_amax=x_amax, g_amax=g_amax, **_strided(stride))
        if has_bias and need[3] and gb is None:
            gb = _bias_grad_sum(gy)
        if has_res and need[4]:
            gr = gy * (residual > 0).to(gy.dtype) if (res_relu and not res_unmasked) else gy
        return gx, None, gw, gb, gr, None, None, None, None, None, None, None


def _xconv(x, weight, bias, residual, relu_in, res_relu, groups=1, alias=False, res_unmasked=False, stride=1):
    """_XConv with the max|.| scalars threaded through: the input's is looked up (or computed), the output's attached.
    alias=True returns (y, alias of x), see _XConv."""
    x_amax = None if _is16(x) else amax_of(x)
    out = _XConv.apply(x, x_amax, weight, bias, residual, relu_in, res_relu, groups, bool(alias), res_unmasked,
                       getattr(x, '_dvd_site', None), stride)
    y = set_amax(out[0], out[1])
    return (y, set_amax(out[2], x_amax)) if len(out) == 3 else y


def wgrad_reports_rowsum(wshape, groups):
    """Does xconv_wgrad(..., rowsum=t) fill t?  (dense 1x1: csrc/xwgrad3.hip dvd_xwgrad1s_rowsum)"""
    return wshape[2] == 1 and groups == 1 and not AB['no_xwgrad3']


# (kernel size, fp16 operands?, the exact-fp32 kernel?) -> (entry point, the one taken when a `rowsum` tensor is given | None,
# workspace query, the integer that follows N, Cin, Cout, H, W in their argument lists: 'groups', the kernel size, or none).
# The exact-fp32 MFMA kernel (csrc/xwgrad.hip) is the one the split-operand kernels replaced: dense fp32 gradients under
# DVD_AB=no_xwgrad3.  The entry points of _XWGRAD_ROWSUM_SLOT have a rowsum pointer (null or not) behind the gradient's.
_XWGRAD = {
    (1, False, False): ('dvd_xwgrad1s_rowsum', 'dvd_xwgrad1s_rowsum', 'dvd_xwgrad1s_workspace_bytes', None),
    (3, False, False): ('dvd_xwgrad3', 'dvd_xwgrad3_rowsum', 'dvd_xwgrad3_workspace_bytes', 'groups'),
    (5, False, False): ('dvd_xwgradk', None, 'dvd_xwgradk_workspace_bytes', 5),
    (7, False, False): ('dvd_xwgradk', None, 'dvd_xwgradk_workspace_bytes', 7),
    (11, False, False): ('dvd_xwgradk', None, 'dvd_xwgradk_workspace_bytes', 11),
    (1, True, False): ('dvd_xwgrad1s_h', None, 'dvd_xwgrad1s_workspace_bytes', None),
    (3, True, False): ('dvd_xwgrad3_h', None, 'dvd_xwgrad3_workspace_bytes', 'groups'),
    (5, True, False): ('dvd_xwgradk_h', None, 'dvd_xwgradk_workspace_bytes', 5),
    (7, True, False): ('dvd_xwgradk_h', None, 'dvd_xwgradk_workspace_bytes', 7),
    (11, True, False): ('dvd_xwgradk_h', None, 'dvd_xwgradk_workspace_bytes', 11),
    (1, False, True): ('dvd_xwgrad', None, 'dvd_xwgrad_workspace_bytes', 1),
    (3, False, True): ('dvd_xwgrad', None, 'dvd_xwgrad_workspace_bytes', 3),
    (5, False, True): ('dvd_xwgrad', None, 'dvd_xwgrad_workspace_bytes', 5),
    (7, False, True): ('dvd_xwgrad', None, 'dvd_xwgrad_workspace_bytes', 7),
    (11, False, True): ('dvd_xwgrad', None, 'dvd_xwgrad_workspace_bytes', 11),
}
_XWGRAD_ROWSUM_SLOT = ('dvd_xwgrad1s_rowsum', 'dvd_xwgrad3_rowsum')


def xconv_wgrad(x, gy, wshape, relu_in, groups=1, x_amax=None, g_amax=None, rowsum=None, stride=1):
    """dW[co][ci][tap] = sum_{n,p} gy[n][co][p] * act(x)[n][ci][p + tap] on the split-operand MFMA kernels of csrc/xwgrad3.hip:
    1x1, 3x3 (dense or grouped) and dense 5x5 / 7x7 / 11x11 (xwgradk: the hourglass's inception branches and the stem's
    space-to-depth form).  fp16 operands take one MFMA per product and the result times 1 / (loss scale) (H16).
    rowsum: [Cout] tensor that receives sum_{n,p} gy[n][co][p] from the fp32 1x1 and 3x3 entry points (dvd_xwgrad1s_rowsum;
    dvd_xwgrad3_rowsum: the 32 x 32 grouped kernel sums the rows it stages, other shapes take a pass over gy); the other entry
    points have no such form and leave it alone (wgrad_reports_rowsum, dvd_xwgrad_rowsum_in_kernel: ask before relying on it).
    stride=2: gy is the compact gradient of a 3x3 / stride 2 / padding 1 convolution of x; the stride-1 kernels take its
    zero-interleaved copy at x's resolution (csrc/pool.hip dvd_subsample2_bwd; the zeros add nothing to dW or to rowsum)."""
    Cout, KS = wshape[0], wshape[2]
    h16 = _is16(gy)
    if h16 and not _is16(x):
        raise RuntimeError('xconv_wgrad: fp16 gradient with an fp32 activation')
    if KS not in (1, 3, 5, 7, 11) or (groups > 1 and KS != 3):
        raise RuntimeError('xconv: the weight gradient exists for 1x1, 3x3 (dense or grouped) and dense 5x5 / 7x7 / 11x11 kernels '
                           '(got %s, %d groups)' % (tuple(wshape), groups))
    entry, with_sums, query, extra = _XWGRAD[(KS, h16, AB['no_xwgrad3'] and groups == 1 and not h16)]
    lib = _lib.load()
    N, Cin, H, W = x.shape
    dims = (N, Cin, Cout, H, W) + {None: (), 'groups': (groups,)}.get(extra, (extra,))
    if not h16:                                 # the operands' scales (fp16 operands carry none); the compact gradient's
        if x_amax is None:                      # maximum is the interleaved one's
            x_amax = amax_of(x)
        if g_amax is None:
            g_amax = amax_of(gy)
    if stride == 2:
        gyf = torch.empty(N, Cout, H, W, device=gy.device, dtype=gy.dtype)
        _lib.check(lib.dvd_subsample2_bwd(_p(gy), _p(gyf), int(h16), N * Cout, H, W, _stream()), 'dvd_subsample2_bwd')
        gy = gyf
    if h16:
        operands = (_p(x), _p(gy), _p(_gs(1)))
    elif entry == 'dvd_xwgrad':
        operands = (_p(x), _p(gy))
    else:
        operands = (_p(x), _p(x_amax), _p(gy), _p(g_amax))
    if rowsum is not None and with_sums is not None:
        entry = with_sums
    sums = (_p(rowsum),) if entry in _XWGRAD_ROWSUM_SLOT else ()
    gw = torch.empty(wshape, device=x.device, dtype=torch.float32)
    ws = _workspace(getattr(lib, query)(*dims), x.device)
    _lib.check(getattr(lib, entry)(*operands, _p(gw), *sums, _p(ws), ctypes.c_size_t(ws.numel()), *dims, int(bool(relu_in)),
                                   _stream()), entry)
    return gw


class _XConvBn(torch.autograd.Function):
    """y = act(bn_eval(conv2d(x, w) + cbias) (+ residual)): the convolution kernel's epilogue applies the BatchNorm, so
    the pre-BN tensor is never written.  Backward: one pass masks the output gradient (g = gy * [y > 0]) and sums it per
    channel (dbeta) -- no pass at all where the consumer's epilogue has masked the gradient and the weight-gradient kernel
    delivers the sums; backward-data runs on g with the weights packed transposed AND scaled by gamma * rstd; backward-weight
    runs on g unscaled, and a tiny kernel derives dW, dgamma and the conv-bias gradient from it (csrc/bnrelu.hip)."""

    @staticmethod
    def forward(ctx, x, x_amax, weight, cbias, gamma, beta, mean, var, eps, residual, relu, groups, alias=False, in_site=None,
                out_site=None, stride=1):
        """stride 2: the 3x3 / stride 2 / padding 1 forms of the kernels (see _XConv), with the same site protocol."""
        ctx.set_materialize_grads(False)    # (alias: see _XConv -- the gradient of the input's other consumers arrives in backward)
        ctx.in_site = in_site if (in_site is not None and not AB['no_maskfuse']) else None      # see _Site
        ctx.out_site = out_site if relu else None
        x = x.contiguous()
        if residual is not None:
            residual = residual.contiguous()
        Cout, _, KS, _ = weight.shape
        y_amax, amax_slot = _fwd_amax(ctx, x)
        y = _xconv_run(x, xconv_packed(weight, False, groups), Cout, KS, bias=cbias, residual=residual, relu_out=relu,
                       groups=groups, bn=(gamma, beta, mean, var, eps), x_amax=x_amax, y_amax=amax_slot,
                       **_strided(stride))
        ctx.save_for_backward(x, y if relu else None, gamma, mean, var, cbias, x_amax)
        ctx.wparam = weight
        ctx.cfg = (float(eps), bool(relu), residual is not None, groups, int(stride))
        if alias:
            return y, y_amax, x
        return y, y_amax

    @staticmethod
    def backward(ctx, gy, _g_amax, g_alias=None):
        x, y, gamma, mean, var, cbias, x_amax = ctx.saved_tensors
        weight = ctx.wparam
        eps, relu, has_res, groups, stride = ctx.cfg
        if gy is None:                      # only the alias was used downstream
            return (g_alias,) + (None,) * 15
        gy = gy.contiguous()
        Cout, Cing, KS, _ = weight.shape
        N, _, H, W = gy.shape
        need = ctx.needs_input_grad
        lib = _lib.load()
        # masked gradient + per-channel sums
        dbeta = torch.empty(Cout, device=gy.device, dtype=torch.float32)
        # the consumer's backward-data epilogue has applied [y > 0] already and nothing touched the tensor since: sums only
        premasked = relu and ctx.out_site is not None and ctx.out_site.is_exactly(gy) and not AB['no_maskfuse']
        mask = relu and not premasked
        need_w = need[2] or (gamma is not None and need[4]) or (cbias is not None and need[3])
        # ... and the sum pass of a pre-masked fp32 site read the whole gradient for one add per element, right before the weight
        # gradient kernel stages the same rows: the dense 1x1 and the grouped 3x3 kernels report the per-channel sums of the rows
        # they stage, the consumer's epilogue has left max|g| -- no pass of this site's own at all.  Only where the kernel itself
        # sums (dvd_xwgrad_rowsum_in_kernel): the entry points' fallback pass for other shapes is slower than the site's pass.
        # A ReLU site that masks for itself takes dbeta from the weight gradient call too (its pass runs for g and max|g| and
        # writes no sums): the sums are then the same bits however the mask was obtained, which
        # tests/test_09_fused_joins_gpu.py asserts of every gradient.  Sites without a ReLU have no such twin and keep their pass.
        # (stride 2: the weight gradient runs at the input's resolution, on the zero-interleaved gradient -- the zeros add nothing
        # to a sum; where that kernel does not sum, the site's pass below sums the compact gradient)
        grouped3 = KS == 3 and groups > 1
        wH, wW = (x.shape[2], x.shape[3]) if stride == 2 else (H, W)
        wgrad_sums = (relu and need_w and gy.dtype == torch.float32 and (grouped3 or wgrad_reports_rowsum(weight.shape, groups)) and
                      lib.dvd_xwgrad_rowsum_in_kernel(N, Cing * groups, Cout, wH, wW, KS, groups) == 1)
        no_pass = premasked and wgrad_sums and ctx.out_site.amax is not None
        if relu:         # (sites_premasked says how the mask was obtained; sites_no_pass only under DVD_AB=rowsum)
            STATS['sites_no_pass' if (no_pass and AB['rowsum']) else ('sites_premasked' if premasked else 'sites_masked')] += 1
        g = torch.empty_like(gy) if mask else gy
        h16 = _is16(gy)
        if no_pass:
            g_amax = ctx.out_site.amax
        else:
            ws = _workspace(lib.dvd_bnrelu_bwd_workspace_bytes(N, Cout, H * W), gy.device)
            # max|masked gradient|, folded in by the mask pass (it reads every element anyway); fp16: the policy's observed maximum
            g_amax = _gs(3) if h16 else new_scalar(gy.device)
            _lib.check(lib.dvd_bnrelu_bwd_t(_p(gy), _p(y) if mask else None, None, _p(var), _p(mean), _p(var), eps, None,
                                            _p(g) if mask else None, None, None if wgrad_sums else _p(dbeta), _p(ws),
                                            ctypes.c_size_t(ws.numel()),
                                            int(h16), _p(_gs(1)) if h16 else None, N, Cout, H * W, int(mask), _p(g_amax),
                                            _stream()), 'dvd_bnrelu_bwd')
        gx = gw = gcb = gg = None
        if need[0]:                 # (+ the other consumers' gradient) * [x > 0] for the site x came from
            gx = _xconv_bwd_data(ctx, g, g_amax, weight, groups, x if ctx.in_site is not None else None, g_alias,
                                 bn_scale=(gamma, var, eps), **_strided_bwd(stride, x))
        elif g_alias is not None:
            gx = g_alias
        if need_w:
            gw = xconv_wgrad(x, g, weight.shape, False, groups, x_amax=x_amax, g_amax=g_amax, rowsum=dbeta if wgrad_sums else None,
                             **_strided(stride))
            gg = torch.empty_like(gamma) if gamma is not None else None
            gcb = torch.empty_like(cbias) if cbias is not None else None
            _lib.check(lib.dvd_convbn_finalize(_p(weight.detach()), _p(gw), _p(dbeta), _p(gamma), _p(mean), _p(var), eps,
                                               _p(cbias), Cout, Cing * KS * KS, _p(gg), _p(gcb), _stream()),
                       'dvd_convbn_finalize')
        return (gx, None, gw, gcb, gg, (dbeta if need[5] else None), None, None, None, (g if has_res else None), None, None, None,
                None, None, None)


class _GConvBn(torch.autograd.Function):
    """y = relu(bn_eval(conv2d(x, w, padding 1, groups C // 8))) for fp32 tensors with the site inside the kernels of
    csrc/gconv.hip (dvd_gconv3x3_c8_bn_*): `_XConvBn`'s site protocol on the 8-per-group family.  The forward epilogue applies
    BatchNorm + ReLU and leaves max|y|; backward-data takes the masked, unscaled gradient and scales it while staging, masks its
    result for the site x came from (`in_site`) and leaves max|gx|; the weight gradient kernel delivers dbeta with dW, whether
    the mask came pre-applied or from this site's own pass (the same bits either way).  The family takes no operand scales, so
    a pre-masked site runs no pass at all."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, mean, var, eps, in_site, out_site):
        ctx.set_materialize_grads(False)
        ctx.in_site = in_site if (in_site is not None and not AB['no_maskfuse']) else None
        ctx.out_site = out_site
        x = x.contiguous()
        N, C, H, W = x.shape
        y = torch.empty_like(x)
        y_amax = new_scalar(x.device)
        ctx.mark_non_differentiable(y_amax)
        _lib.check(_lib.load().dvd_gconv3x3_c8_bn_fwd(_p(x), _p(weight), _p(gamma), _p(beta), _p(mean), _p(var), float(eps), _p(y),
                                                      _p(y_amax), N, C, H, W, _stream()), 'dvd_gconv3x3_c8_bn_fwd')
        ctx.save_for_backward(x, y, weight, gamma, mean, var)
        ctx.eps = float(eps)
        return y, y_amax

    @staticmethod
    def backward(ctx, gy, _g_amax):
        x, y, weight, gamma, mean, var = ctx.saved_tensors
        if gy is None:
            return (None,) * 9
        gy = gy.contiguous()
        N, C, H, W = x.shape
        eps = ctx.eps
        need = ctx.needs_input_grad
        lib = _lib.load()
        premasked = ctx.out_site is not None and ctx.out_site.is_exactly(gy) and not AB['no_maskfuse']
        STATS['sites_premasked' if premasked else 'sites_masked'] += 1
        g = gy
        if not premasked:                   # g = gy * [y > 0]; no sums, no maximum: the gradient kernels below need neither
            g = torch.empty_like(gy)
            ws = _workspace(lib.dvd_bnrelu_bwd_workspace_bytes(N, C, H * W), gy.device)
            _lib.check(lib.dvd_bnrelu_bwd_t(_p(gy), _p(y), None, _p(var), _p(mean), _p(var), eps, None, _p(g), None, None, _p(ws),
                                            ctypes.c_size_t(ws.numel()), 0, None, N, C, H * W, 1, None, _stream()), 'dvd_bnrelu_bwd')
        gx = gw = gg = dbeta = None
        if need[0]:
            gx = torch.empty_like(x)
            gx_amax = new_scalar(gy.device)
            _lib.check(lib.dvd_gconv3x3_c8_bn_bwd_data(_p(g), _p(weight), _p(gamma), _p(var), eps,
                                                       _p(x) if ctx.in_site is not None else None, _p(gx), _p(gx_amax), N, C, H, W,
                                                       _stream()), 'dvd_gconv3x3_c8_bn_bwd_data')
            set_amax(gx, gx_amax)
            if ctx.in_site is not None:
                ctx.in_site.wrote(gx, gx_amax)
        if need[1] or need[2] or need[3]:
            gw = torch.empty_like(weight)
            dbeta = torch.empty(C, device=gy.device, dtype=torch.float32)
            ws = _workspace(lib.dvd_gconv3x3_c8_bn_wgrad_workspace_bytes(N, C, H, W), gy.device)
            _lib.check(lib.dvd_gconv3x3_c8_bn_bwd_weight(_p(x), _p(g), _p(gw), _p(dbeta), _p(ws), ctypes.c_size_t(ws.numel()), N, C,
                                                         H, W, _stream()), 'dvd_gconv3x3_c8_bn_bwd_weight')
            gg = torch.empty_like(gamma)
            _lib.check(lib.dvd_convbn_finalize(_p(weight), _p(gw), _p(dbeta), _p(gamma), _p(mean), _p(var), eps, None, C, 72,
                                               _p(gg), None, _stream()), 'dvd_convbn_finalize')
        return gx, gw, gg, (dbeta if need[3] else None), None, None, None, None, None


# ---- which kernels serve a convolution --------------------------------------------------------------------------------
# family: 'xconv' (split-operand MFMA kernels, csrc/xconv.hip + csrc/xwgrad3.hip), 'gconv' (8 per group, csrc/gconv.hip),
# 'gconv32' (the fp32 MFMA kernels of csrc/gconv32.hip, under DVD_AB=gconv32 only) or None (ATen); groups: what the kernels are
# told; paired: the weight goes through _pair_groups_of_16; stride: the kernel's own (1, or 2: the native 3x3 / stride 2 forms);
# subsample: None, 'out' (a strided 'same' 3x3 is the stride-1 result at [s*i][s*j]: the stride-1 kernel's output sub-sampled)
# or 'in' (a strided 1x1 without padding: the 1x1 kernel on the sub-sampled input); plain: None, or the family that serves the
# bare conv(x) in place of `family` -- kernels without epilogue operands, so everything that fuses (xconv2d, conv_bn_act) stays
# on `family`.
_Route = collections.namedtuple('_Route', 'family groups paired stride subsample plain')
_ATEN = _Route(None, 1, False, 1, None, None)


def _route(conv, x):
    """The route of nn.Conv2d `conv` applied to x, from the layer's hyper-parameters, x's device / dtype / rank and the AB
    switches -- and from nothing else: the module classes below, xconv2d and conv_bn_act all take it from here."""
    k, st, g = conv.kernel_size, tuple(conv.stride), conv.groups
    if not (x.is_cuda and x.dtype in ACT_DTYPES and x.dim() == 4 and conv.weight.dtype == torch.float32 and k[0] == k[1] and
            st[0] == st[1] and tuple(conv.dilation) == (1, 1)):
        return _ATEN
    k, st, pad = k[0], st[0], tuple(conv.padding)
    if k == 1 and st > 1:                   # the ResNeXt down-sampling shortcut
        return _Route('xconv', 1, False, 1, 'in', None) if (g == 1 and pad == (0, 0)) else _ATEN
    if not (k % 2 == 1 and k <= 11 and pad == (k // 2, k // 2) and conv.padding_mode == 'zeros'):
        return _ATEN
    cpg = conv.in_channels // g
    square3 = k == 3 and conv.in_channels == conv.out_channels and conv.bias is None
    conv2 = square3 and g > 1               # the shape of a ResNeXt bottleneck's `conv2`
    if conv2 and cpg == 8:                  # stage 1
        return _Route('gconv', g, False, 1, None, None) if st == 1 else _ATEN
    # stage 2, 16 per group: two groups share one 32 x 32 tile of the grouped kernels with a block-diagonal weight (MIOpen's
    # immediate mode runs this shape per image as im2col + small GEMMs, ~80 launches per call)
    paired = conv2 and cpg == 16 and conv.in_channels % 32 == 0
    if paired:
        g, cpg = g // 2, 32
    if (g > 1 and (k != 3 or cpg < 32)) or (st > 1 and k != 3):
        return _ATEN
    plain = None
    if AB['gconv32'] and conv2 and cpg == 32:
        # the legacy kernels are fp32 and stride 1: the bare forward of a 32-per-group layer; under the switch the pairing exists
        # for them alone
        legacy = st == 1 and x.dtype == torch.float32
        if paired:
            return _Route('gconv32', g, True, 1, None, None) if legacy else _ATEN
        plain = 'gconv32' if legacy else None
    if st == 1:
        if square3 and conv.in_channels == 8:           # one group of 8: GroupedConv3x3C8(8)'s forward is the 8-per-group kernels'
            plain = 'gconv'
        return _Route('xconv', g, paired, 1, None, plain)
    # the strided forms need whole 16-channel chunks per group (the buffer-addressed main loop); DVD_AB=no_s2, other strides and
    # other channel counts: 4x (s^2 x) the needed work at stride 1, still half of MIOpen's per-image im2col + GEMM + col2im path
    if st == 2 and not AB['no_s2'] and cpg % 16 == 0 and (conv.out_channels // g) % 16 == 0:
        return _Route('xconv', g, paired, 2, None, None)
    return _Route('xconv', g, paired, 1, 'out', None)


def _xconv_s1(r):
    """Does the stride-1 xconv kernel take the layer's own weight at x's resolution -- the form that has every epilogue operand
    (input ReLU, residual, BatchNorm, alias)?"""
    return r.family == 'xconv' and not r.paired and r.stride == 1 and r.subsample is None


def _route_weight(r, conv):
    """The weight the route's kernels take.  The paired one is a tensor derived per call: it has no PACK_PLAN entry, so its
    packings (the scaled transposed one included) are launched with the pass, inside a captured graph too, and follow the
    parameters on every replay."""
    return _pair_groups_of_16(conv.weight) if r.paired else conv.weight


def _routed(r, conv, x):
    """conv(x) on route r."""
    family = r.plain or r.family
    if family is None:
        return nn.Conv2d.forward(conv, x)
    if family == 'gconv':
        return _GConv3x3C8.apply(x, conv.weight)
    if family == 'gconv32':
        return _GConv3x3C32.apply(x, _route_weight(r, conv))
    if r.subsample == 'in':
        x = _subsample(x, conv.stride[0])
    y = _xconv(x, _route_weight(r, conv), conv.bias, None, False, False, r.groups, stride=r.stride)
    return _subsample(y, conv.stride[0]) if r.subsample == 'out' else y


def _bn_site(r, conv, bn, x, residual, relu):
    """Which fused site takes `conv` on route r followed by BatchNorm `bn` (+ residual, + ReLU) -> 'xconv' (the stride-1 kernel,
    also on the sub-sampled input of a strided 1x1: fp32 and fp16, any epilogue), or one of the ResNeXt `conv2` kinds 'c8'
    (_GConvBn), 'c16' (paired groups) and 's2' (the native stride-2 forms), or None: conv(x) followed by bn_eval_relu.
    The `conv2` kinds are fp32 ReLU sites without residual.  fp16 activations keep the composition there: their passes move half
    the bytes, and the loss scale would have to be threaded through dbeta and dvd_convbn_finalize first."""
    if r.family is None or bn.training or not bn.track_running_stats:
        return None
    if _xconv_s1(r) or r.subsample == 'in':
        return 'xconv'
    if not (x.dtype == torch.float32 and relu and residual is None and bn.affine and conv.bias is None and
            (conv.groups == 1 or conv.in_channels == conv.out_channels)):
        return None
    if r.family == 'gconv':
        return 'c8'
    if r.family == 'xconv' and r.subsample is None:
        return 's2' if r.stride == 2 else 'c16'
    return None


def conv_bn_act(conv, bn, x, residual=None, relu=True, alias=False):
    """relu(bn(conv(x)) (+ residual)) for an nn.Conv2d followed by an eval-mode nn.BatchNorm2d.  Convolutions the stride-1 xconv
    kernel covers run as ONE launch (BatchNorm, residual and ReLU in the epilogue), and so do, for fp32 tensors, the ResNeXt
    `conv2` layers outside that form: 8 and 16 channels per group and the 3x3 / stride 2 entries (_bn_site); everything else
    (CPU tensors, training-mode statistics, those `conv2` layers with fp16 activations) is conv(x) followed by the fused
    BatchNorm+ReLU kernel / the ATen ops.
    alias=True returns (y, x'): x' carries x's values and must be used by every OTHER consumer of x (the block's shortcut);
    on the 'xconv' site their gradient is then added inside this convolution's backward-data kernel instead of by autograd's
    accumulation pass (see _XConv); on the other paths x' is x itself."""
    r = _route(conv, x) if isinstance(conv, nn.Conv2d) else _ATEN
    kind = _bn_site(r, conv, bn, x, residual, relu)
    if kind is None:
        y = bn_eval_relu(bn, conv(x), residual=residual, relu=relu)
        return (y, x) if alias else y
    stats = (bn.running_mean, bn.running_var, bn.eps)
    out_site = _Site() if relu else None
    if kind == 'c8':
        out = _GConvBn.apply(x, conv.weight, bn.weight, bn.bias, *stats, getattr(x, '_dvd_site', None), out_site)
    else:
        xin = _subsample(x, conv.stride[0]) if r.subsample == 'in' else x
        gamma, beta = (bn.weight, bn.bias) if bn.affine else (None, None)
        x_amax = None if _is16(xin) else amax_of(xin)
        join = bool(kind == 'xconv' and alias and xin is x and not AB['no_alias'])
        # (xin may be a BatchNorm+ReLU site's output, see _Site)
        out = _XConvBn.apply(xin, x_amax, _route_weight(r, conv), conv.bias, gamma, beta, *stats, residual, relu, r.groups, join,
                             getattr(xin, '_dvd_site', None), out_site, r.stride)
    out[0]._dvd_site = out_site
    y = set_amax(out[0], out[1])
    if len(out) == 3:
        return y, set_amax(out[2], x_amax)
    return (y, x) if alias else y


def _conv2_site_kind(conv, bn, x, residual, relu):
    """_bn_site's answer where it is one of the `conv2` kinds ('c8', 'c16', 's2'), else None."""
    kind = _bn_site(_route(conv, x), conv, bn, x, residual, relu)
    return None if kind == 'xconv' else kind


def xconv_supported(conv, x):
    return _xconv_s1(_route(conv, x))


def xconv_s2_supported(conv, x):
    """3x3 / stride 2 / padding 1 on the strided forms of csrc/xconv.hip?"""
    r = _route(conv, x)
    return r.family == 'xconv' and r.stride == 2


def xconv_strided_1x1_supported(conv, x):
    """A dense strided 1x1 convolution without padding: the 1x1 kernel on the sub-sampled input?"""
    return _route(conv, x).subsample == 'in'


def xconv2d(conv, x, relu_in=False, residual=None, res_relu=False, alias=False, res_unmasked=False):
    """`conv(relu(x) if relu_in else x) + (relu(residual) if res_relu else residual)` for an nn.Conv2d `conv`.
    GPU fp32 / fp16 tensors of a stride-1 'same' convolution the xconv kernel covers run as one launch; CPU tensors (the oracle /
    golden-fixture generator instantiates these modules on the CPU) take the ATen ops the reference uses."""
    if xconv_supported(conv, x):
        if AB['no_alias']:
            y = _xconv(x, conv.weight, conv.bias, residual, relu_in, res_relu, conv.groups)
            return (y, x) if alias else y
        return _xconv(x, conv.weight, conv.bias, residual, relu_in, res_relu, conv.groups, alias, res_unmasked)
    if x.is_cuda and x.dtype in ACT_DTYPES and conv.groups == 1 and tuple(conv.stride) == (1, 1):
        raise RuntimeError('xconv2d: convolution %r is not covered by the HIP kernels' % (conv,))
    y = conv(F.relu(x) if relu_in else x)
    if residual is not None:
        y = y + (F.relu(residual) if res_relu else residual)
    return (y, x) if alias else y


class XConv2d(nn.Conv2d):
    """Drop-in nn.Conv2d (same parameters / state_dict keys) that runs on the HIP kernels wherever _route finds a family for
    the layer and the tensor: stride-1 'same' convolutions (dense, or grouped 3x3 with 8, 16 or at least 32 channels per
    group), 3x3 'same' convolutions of stride 2 (the strided forms of the kernel) and of other strides (the stride-1 kernel's
    output sub-sampled), and the strided 1x1 without padding (the ResNeXt down-sampling shortcut).  Anything else, and CPU
    tensors, take ATen."""

    def forward(self, x):
        return _routed(_route(self, x), self, x)


class GroupedConv3x3C8(XConv2d):
    """nn.Conv2d(C, C, 3, stride=1, padding=1, groups=C // 8, bias=False): the `conv2` of the ResNeXt-101 32x8d stage-1 bottlenecks."""

    def __init__(self, channels):
        if channels % 8:
            raise ValueError('GroupedConv3x3C8 needs a multiple of 8 channels')
        super().__init__(channels, channels, 3, stride=1, padding=1, groups=channels // 8, bias=False)


class GroupedConv3x3C16(XConv2d):
    """nn.Conv2d(C, C, 3, stride=stride, padding=1, groups=C // 16, bias=False) (ResNeXt stage 2)."""

    def __init__(self, channels, stride=1):
        if channels % 32:
            raise ValueError('GroupedConv3x3C16 needs a multiple of 32 channels')
        super().__init__(channels, channels, 3, stride=stride, padding=1, groups=channels // 16, bias=False)


class GroupedConv3x3C32(XConv2d):
    """nn.Conv2d(C, C, 3, stride=1, padding=1, groups=C // 32, bias=False) (ResNeXt stages 3 and 4): on the grouped xconv kernels,
    0.097 ms forward / 0.37 ms backward per 16-image call at [1024, 24, 42] against 0.156 / 0.42 ms of the fp32-MFMA kernels
    (tools/microbench_gx.py)."""

    def __init__(self, channels):
        if channels % 32:
            raise ValueError('GroupedConv3x3C32 needs a multiple of 32 channels')
        super().__init__(channels, channels, 3, stride=1, padding=1, groups=channels // 32, bias=False)
