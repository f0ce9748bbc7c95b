"""Autograd operators over the C-ABI of libupflow_hip.so (include/upflow_hip.h).

Each operator = one HIP launch on the current torch stream.  Flows, sampling positions and masks
are fp32 whatever the feature dtype.  No CPU path: non-GPU tensors raise.
"""
import os

import torch
from torch.autograd import Function

from . import _lib
from ._operand_cache import OperandCache
from ._lib import MASK_NONE, MASK_LITERAL, MASK_ROBUST, UpflowHipError  # noqa: F401

_MASKS = {None: MASK_NONE, 'none': MASK_NONE, 'literal': MASK_LITERAL, 'robust': MASK_ROBUST,
          MASK_NONE: MASK_NONE, MASK_LITERAL: MASK_LITERAL, MASK_ROBUST: MASK_ROBUST}


def _f32(t):
    return t if t.dtype == torch.float32 else t.float()


# ------------------------------------------------------------------------------------------------
# pitched NCHW tensors (round 5)
# ------------------------------------------------------------------------------------------------
# A 16-bit NCHW tensor of a RAGGED pyramid level (KITTI's native 375x1242 frames: W = 621, 311, 156, 78, 39, 20 — never a multiple
# of 8, often odd) has rows that are not even 4-byte aligned.  The inference schedule therefore keeps such tensors PITCHED: allocated
# as [B,C,H,Wp] with Wp = W rounded up to 8 and used through the view [..., :W] (shape [B,C,H,W], strides (C*H*Wp, H*Wp, Wp, 1)).
# Every row then starts on a 16-byte boundary and the kernels take their aligned forms (include/upflow_hip.h: the *_pitched entry
# points); nothing depends on what the padding columns hold.  torch operators see an ordinary strided view.
PITCH_MULTIPLE = 8


def empty_nchw(shape, dtype, device, pitched=True):
    """torch.empty(shape) for a [..., H, W] tensor; `pitched` and a 16-bit dtype and a W >= 8 that is not a multiple of 8: the
    pitched form described above."""
    W = shape[-1]
    if pitched and dtype in (torch.bfloat16, torch.float16) and W >= 8 and W % PITCH_MULTIPLE:
        Wp = (W + PITCH_MULTIPLE - 1) // PITCH_MULTIPLE * PITCH_MULTIPLE
        return torch.empty(tuple(shape[:-1]) + (Wp,), dtype=dtype, device=device)[..., :W]
    return torch.empty(tuple(shape), dtype=dtype, device=device)


def nchw_pitch(t):
    """Row pitch (elements) of a [B,C,H,W] tensor that is a channel slice of a (possibly pitched) NCHW buffer — unit-stride rows,
    planes H * pitch apart, only the batch stride free — or None for any other layout."""
    if t.dim() != 4:
        return None
    B, C, H, W = t.shape
    sb, sc, sh, sw = t.stride()
    if W > 1 and sw != 1:
        return None
    if H > 1:
        p = sh
    elif C > 1:
        p = sc                      # (a single row per plane: the plane stride is the pitch)
    else:
        p = W
    if p < W or (C > 1 and sc != H * p):
        return None
    return p


def _pitch_or_raise(t, what):
    p = nchw_pitch(t)
    if p is None:
        raise UpflowHipError('%s must be a channel slice of a (possibly row-pitched) contiguous NCHW buffer, got shape %s strides %s'
                             % (what, tuple(t.shape), tuple(t.stride())))
    return p


def _out_pitch_or_raise(t, what):
    """_pitch_or_raise for a tensor a kernel WRITES.  The pitched kernels store whole 8-pixel segments (wide epilogue) / pixel pairs
    (warp) and let the tail land in columns [W, pitch) of the row: harmless in the padding ops.empty_nchw creates (pitch a multiple
    of 8, fewer than 8 padding columns) and in contiguous rows (pitch == W: the kernels then take their exact-width stores), but a
    column crop of a wider LIVE buffer (`big[..., :W]`) has the same strides and its "padding" is somebody's data:
    rejected, as every round before the pitched forms did."""
    p = _pitch_or_raise(t, what)
    W = t.shape[3]
    if p != W and (p % PITCH_MULTIPLE or p - W >= PITCH_MULTIPLE):
        raise UpflowHipError('%s: output rows must be contiguous or padded as ops.empty_nchw pads them (pitch %% %d == 0, pitch - W < %d); '
                             'got W = %d, pitch = %d — a column crop of a wider buffer would have its neighbours overwritten'
                             % (what, PITCH_MULTIPLE, PITCH_MULTIPLE, W, p))
    return p


# ------------------------------------------------------------------------------------------------
# cost volume
# ------------------------------------------------------------------------------------------------
def _corr_pair(f1, f2, who):
    """(B, C, H, W) of the two feature tensors of a cost volume: one shape, one dtype."""
    if f1.shape != f2.shape or f1.dim() != 4 or f1.dtype != f2.dtype:
        raise UpflowHipError('%s: inputs must be two [B,C,H,W] tensors of one dtype, got %s %s / %s %s'
                             % (who, tuple(f1.shape), f1.dtype, tuple(f2.shape), f2.dtype))
    return f1.shape


def _corr_out(out, f1, dtypes, who):
    """-> (out, batch stride for the entry point): a fresh [B,81,H,W] tensor (stride 0 = contiguous) for None, else `out` checked to
    be a [B,81,H,W] channel slice of a contiguous NCHW buffer of one of `dtypes`."""
    B, C, H, W = f1.shape
    if out is None:
        return torch.empty((B, 81, H, W), dtype=f1.dtype, device=f1.device), 0
    if out.shape != (B, 81, H, W) or out.dtype not in dtypes or out.device != f1.device:
        raise UpflowHipError('%s: bad `out` %s %s' % (who, tuple(out.shape), out.dtype))
    if out.stride()[1:] != (H * W, W, 1):
        raise UpflowHipError('%s: `out` must be a channel slice of a contiguous NCHW buffer' % who)
    return out, out.stride(0)


def _corr_norm_workspace(f):
    """Scratch of the normalising cost volume's statistics launch (upf_corr81_norm_workspace_bytes)."""
    return torch.empty((_lib.lib().upf_corr81_norm_workspace_bytes(*f.shape),), dtype=torch.uint8, device=f.device)


def _timed_call(dev, name, nrep, *args):
    """-> (avg_us, min_us) of a *_timed entry point: `args`, then the current stream of `dev`, `nrep` and the two results."""
    import ctypes
    avg, mn = ctypes.c_float(), ctypes.c_float()
    with torch.cuda.device(dev):
        _lib.call(name, *args, _lib.stream_ptr(dev), int(nrep), ctypes.byref(avg), ctypes.byref(mn))
    return avg.value, mn.value


def corr81_forward_raw(f1, f2, out=None, leaky_slope=0.0):
    """One launch of upf_corr81_forward.  `out` may be a [B,81,H,W] channel-slice of a wider
    contiguous [B,Ctot,H,W] buffer (e.g. the 115-channel estimator input, model/upflow.py:565)."""
    B, C, H, W = _corr_pair(f1, f2, 'corr81')
    dev = _lib.check_gpu(f1, f2)
    out, bstride = _corr_out(out, f1, (f1.dtype,), 'corr81')
    _lib.launch(dev, 'upf_corr81_forward', _lib.ptr(f1), _lib.ptr(f2), _lib.ptr(out), B, C, H, W,
                _lib.dtype_code(f1), bstride, float(leaky_slope))
    return out


def corr_set_option(name, value):
    """Launch heuristics of the 16-bit cost volume (include/upflow_hip.h: "variant", "old_path"); returns the previous value."""
    prev = _lib.lib().upf_corr_set_option(name.encode(), int(value))
    if prev == -1000:
        raise UpflowHipError('unknown cost-volume option %r' % name)
    return prev


def corr81_norm_supported(f):
    """The fused normalise + cost-volume launch pair applies (bf16 / fp16 features with C <= 208, rows of >= 4 pixels, or
    aligned rows of any length)."""
    return (f.dtype in (torch.bfloat16, torch.float16) and f.shape[3] >= 4
            and bool(_lib.lib().upf_corr81_norm_supported(f.shape[1], _lib.dtype_code(f))))


def corr81_norm_forward_raw(f1, f2, out=None, leaky_slope=0.0):
    """corr81(normalize(f1), normalize(f2)) with the normalisation applied inside the cost volume's loader
    (upf_corr81_norm_forward: one statistics launch + one cost-volume launch; bit-identical to normalize x2 + corr81).
    Inference only.  `out` as in corr81_forward_raw."""
    B, C, H, W = _corr_pair(f1, f2, 'corr81_norm')
    dev = _lib.check_gpu(f1, f2, contiguous=False)
    fp = _feature_pair_pitch(f1, f2, 'corr81_norm')
    # (`out` may be the OTHER 16-bit type: fp16 pyramid features into a bf16 estimator buffer, the `pyramid_dtype` option)
    out, bstride = _corr_out(out, f1, (torch.bfloat16, torch.float16), 'corr81_norm')
    ws = _corr_norm_workspace(f1)
    _lib.launch(dev, 'upf_corr81_norm_forward_mixed', _lib.ptr(f1), _lib.ptr(f2), fp, _lib.ptr(out), B, C, H, W,
                _lib.dtype_code(f1), _lib.dtype_code(out), bstride, float(leaky_slope), _lib.ptr(ws))
    return out


def _feature_pair_pitch(f1, f2, who):
    """Common row pitch of two whole [B,C,H,W] feature tensors (contiguous, or pitched: empty_nchw) — items C*H*pitch apart."""
    p1, p2 = nchw_pitch(f1), nchw_pitch(f2)
    B, C, H, W = f1.shape
    if p1 is None or p1 != p2 or any(B > 1 and t.stride(0) != C * H * p1 for t in (f1, f2)):
        raise UpflowHipError('%s: f1 / f2 must be whole NCHW tensors of one row pitch (contiguous or ops.empty_nchw), got strides %s / %s'
                             % (who, tuple(f1.stride()), tuple(f2.stride())))
    return p1


CORR81_C8_OCTETS = 11


def corr81_c8_channel_map():
    """Position -> cost-volume channel of the 11 octets upf_corr81_norm_forward_c8 writes (-1 = a zero position): octet j < 9
    holds channels 9j .. 9j+7 (dy = j-4, dx = -4..3), octet 9 position p channel 9p+8 (dx = +4), octet 10 position 0 channel 80."""
    m = []
    for j in range(9):
        m += [9 * j + t for t in range(8)]
    m += [9 * p + 8 for p in range(8)]
    m += [80] + [-1] * 7
    return m


def corr81_norm_forward_c8(f1, f2, out8, leaky_slope=0.0):
    """corr81_norm_forward_raw into 11 octets `out8` [B,11,H,W,8] of a channel-octet buffer (order: corr81_c8_channel_map)."""
    B, C, H, W = _corr_pair(f1, f2, 'corr81_norm_c8')
    dev = _lib.check_gpu(f1, f2, contiguous=False)
    if not out8.is_cuda or tuple(out8.shape) != (B, CORR81_C8_OCTETS, H, W, 8) or not _c8_view_ok(out8) or out8.dtype not in (torch.bfloat16, torch.float16):
        raise UpflowHipError('corr81_norm_c8: out8 must be an octet slice [%d,11,%d,%d,8] of a 16-bit C8 buffer, got %s' % (B, H, W, tuple(out8.shape)))
    if nchw_pitch(f1) is None or nchw_pitch(f2) is None:
        f1, f2 = f1.contiguous(), f2.contiguous()
    fp = _feature_pair_pitch(f1, f2, 'corr81_norm_c8')
    ws = _corr_norm_workspace(f1)
    _lib.launch(dev, 'upf_corr81_norm_forward_c8_mixed', _lib.ptr(f1), _lib.ptr(f2), fp, _lib.ptr(out8), out8.stride(0), B, C, H, W,
                _lib.dtype_code(f1), _lib.dtype_code(out8), float(leaky_slope), _lib.ptr(ws))
    return out8


def flow_update_c8(a, b, c, out8):
    """flow_update for a 2-channel flow into ONE octet `out8` [N,1,H,W,8] of a channel-octet buffer (positions 0, 1; 2..7 = 0)."""
    a = _f32(a).contiguous()
    N, two, H, W = a.shape
    if two != 2 or tuple(out8.shape) != (N, 1, H, W, 8) or not _c8_view_ok(out8) or out8.dtype not in (torch.bfloat16, torch.float16):
        raise UpflowHipError('flow_update_c8: a [N,2,H,W] and one octet [N,1,H,W,8] of a 16-bit C8 buffer expected')
    for t in (b, c):
        if t is not None and (tuple(t.shape) != tuple(a.shape) or not t.is_contiguous() or t.dtype != out8.dtype):
            raise UpflowHipError('flow_update_c8: b / c must be contiguous tensors of the buffer dtype shaped like a')
    dev = _lib.check_gpu(a, b, c)
    if not out8.is_cuda:
        raise UpflowHipError('flow_update_c8: GPU tensors expected (there is no CPU fallback)')
    with torch.cuda.device(dev):
        _lib.call('upf_flow_update_c8', _lib.ptr(a), _lib.ptr(b), _lib.ptr(c), _lib.ptr(out8), out8.stride(0), N, H * W,
                  _lib.dtype_code(out8), _lib.stream_ptr(dev))
    return out8


def corr81_forward_timed(f1, f2, out, leaky_slope=0.0, nrep=50):
    """-> (avg_us, min_us) of `nrep` launches, each timed by HIP events recorded around the kernel on
    the current stream (upf_corr81_forward_timed).  Measurement helper for bench.py."""
    B, C, H, W = f1.shape
    dev = _lib.check_gpu(f1, f2, out)
    return _timed_call(dev, 'upf_corr81_forward_timed', nrep, _lib.ptr(f1), _lib.ptr(f2), _lib.ptr(out), B, C, H, W,
                       _lib.dtype_code(f1), 0, float(leaky_slope))


def corr81_norm_forward_timed(f1, f2, out, leaky_slope=0.0, nrep=50):
    """-> (avg_us, min_us) of `nrep` launches of the NORMALISING cost volume (the kernel inside the inference step), each
    between its own pair of HIP events; the statistics launch runs once, untimed.  Measurement helper for bench.py."""
    B, C, H, W = f1.shape
    dev = _lib.check_gpu(f1, f2, out)
    ws = _corr_norm_workspace(f1)
    return _timed_call(dev, 'upf_corr81_norm_forward_timed', nrep, _lib.ptr(f1), _lib.ptr(f2), _lib.ptr(out), B, C, H, W,
                       _lib.dtype_code(f1), 0, float(leaky_slope), _lib.ptr(ws))


def corr81_norm_forward_c8_timed(f1, f2, out8, leaky_slope=0.0, nrep=50):
    """corr81_norm_forward_timed for the octet-output form (corr81_norm_forward_c8): the launch inside the inference step at
    the levels whose flow estimator runs in the channel-octet layout."""
    B, C, H, W = f1.shape
    dev = _lib.check_gpu(f1, f2, contiguous=False)
    if tuple(out8.shape) != (B, CORR81_C8_OCTETS, H, W, 8) or not _c8_view_ok(out8):
        raise UpflowHipError('corr81_norm_c8_timed: out8 must be an octet slice [%d,11,%d,%d,8]' % (B, H, W))
    fp = _feature_pair_pitch(f1, f2, 'corr81_norm_c8_timed')
    ws = _corr_norm_workspace(f1)
    # (out8 may be the OTHER 16-bit type: fp16 features into bf16 octets — the launch of the bf16 step with its fp16 pyramid)
    return _timed_call(dev, 'upf_corr81_norm_forward_c8_timed_mixed', nrep, _lib.ptr(f1), _lib.ptr(f2), fp, _lib.ptr(out8), out8.stride(0),
                       B, C, H, W, _lib.dtype_code(f1), _lib.dtype_code(out8), float(leaky_slope), _lib.ptr(ws))


def corr81_backward_raw(f1, f2, grad_out, g1=None, g2=None):
    """g1 / g2: optional contiguous tensors shaped like f1 / f2 that the kernels write in place (the legacy FFI's outputs)."""
    B, C, H, W = f1.shape
    grad_out = grad_out.contiguous()
    dev = _lib.check_gpu(f1, f2, grad_out)
    g1 = torch.empty_like(f1) if g1 is None else g1
    g2 = torch.empty_like(f2) if g2 is None else g2
    for g, f in ((g1, f1), (g2, f2)):
        if g.shape != f.shape or g.dtype != f.dtype or g.device != f.device or not g.is_contiguous():
            raise UpflowHipError('corr81_backward: gradient outputs must be contiguous tensors like the inputs')
    with torch.cuda.device(dev):
        _lib.call('upf_corr81_backward', _lib.ptr(f1), _lib.ptr(f2), _lib.ptr(grad_out), _lib.ptr(g1), _lib.ptr(g2),
                  B, C, H, W, _lib.dtype_code(f1), _lib.stream_ptr(dev))
    return g1, g2


class Corr81Function(Function):
    """Modern static replacement of the legacy CorrelationFunction
    (model/correlation_package/correlation.py:6-44) for (pad,k,md,s1,s2) = (4,1,4,1,1)."""

    @staticmethod
    def forward(ctx, f1, f2, leaky_slope=0.0):
        f1 = f1.contiguous()
        f2 = f2.contiguous()
        out = corr81_forward_raw(f1, f2, None, leaky_slope)
        ctx.slope = float(leaky_slope)
        if ctx.slope != 0.0:
            ctx.save_for_backward(f1, f2, out)
        else:
            ctx.save_for_backward(f1, f2)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.slope != 0.0:
            f1, f2, out = ctx.saved_tensors
            grad_out = torch.ops.aten.leaky_relu_backward(grad_out.to(out.dtype), out, ctx.slope, True)   # (sign of the output = sign of the input)
        else:
            f1, f2 = ctx.saved_tensors
        g1, g2 = corr81_backward_raw(f1, f2, grad_out.to(f1.dtype))
        return g1, g2, None


def corr81(f1, f2, leaky_slope=0.0):
    return Corr81Function.apply(f1, f2, leaky_slope)


def correlation_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2):
    import ctypes
    oc, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.call('upf_correlation_out_shape', H, W, pad_size, kernel_size, max_displacement, stride1, stride2,
              ctypes.byref(oc), ctypes.byref(oh), ctypes.byref(ow))
    return oc.value, oh.value, ow.value


def correlation_forward_general(in1, in2, pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply=1, out=None):
    """upf_correlation_forward: the reference's full parameter list (correlation_cuda.cc:10-17).  `out`: a contiguous
    [B, oc, oh, ow] tensor of the inputs' dtype the kernel writes IN PLACE (the legacy FFI's caller-owned output)."""
    in1, in2 = in1.contiguous(), in2.contiguous()
    B, C, H, W = in1.shape
    dev = _lib.check_gpu(in1, in2)
    oc, oh, ow = correlation_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2)
    if out is None:
        out = torch.empty((B, oc, oh, ow), dtype=in1.dtype, device=in1.device)
    elif tuple(out.shape) != (B, oc, oh, ow) or out.dtype != in1.dtype or out.device != in1.device or not out.is_contiguous():
        raise UpflowHipError('correlation_forward: `out` must be a contiguous [%d,%d,%d,%d] %s tensor on the inputs\' device'
                             % (B, oc, oh, ow, in1.dtype))
    with torch.cuda.device(dev):
        _lib.call('upf_correlation_forward', _lib.ptr(in1), _lib.ptr(in2), _lib.ptr(out), B, C, H, W,
                  _lib.dtype_code(in1), pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply,
                  _lib.stream_ptr(dev))
    return out


def correlation_backward_general(in1, in2, grad_out, pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply=1,
                                 g1=None, g2=None):
    """upf_correlation_backward: gradients of correlation_forward_general wrt both inputs (kernel_size 1, stride1 1; the tuned
    kernels for (4,1,4,1,1)); g1 / g2 optional in-place outputs."""
    in1, in2, grad_out = in1.contiguous(), in2.contiguous(), grad_out.contiguous()
    B, C, H, W = in1.shape
    dev = _lib.check_gpu(in1, in2, grad_out)
    oc, oh, ow = correlation_out_shape(H, W, pad_size, kernel_size, max_displacement, stride1, stride2)
    if tuple(grad_out.shape) != (B, oc, oh, ow) or grad_out.dtype != in1.dtype or in2.shape != in1.shape or in2.dtype != in1.dtype:
        raise UpflowHipError('correlation_backward: grad_out must be [%d,%d,%d,%d] of the inputs\' dtype, got %s %s'
                             % (B, oc, oh, ow, tuple(grad_out.shape), grad_out.dtype))
    g1 = torch.empty_like(in1) if g1 is None else g1
    g2 = torch.empty_like(in2) if g2 is None else g2
    for g in (g1, g2):
        if g.shape != in1.shape or g.dtype != in1.dtype or g.device != in1.device or not g.is_contiguous():
            raise UpflowHipError('correlation_backward: gradient outputs must be contiguous tensors like the inputs')
    with torch.cuda.device(dev):
        _lib.call('upf_correlation_backward', _lib.ptr(in1), _lib.ptr(in2), _lib.ptr(grad_out), _lib.ptr(g1), _lib.ptr(g2), B, C, H, W,
                  _lib.dtype_code(in1), pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply, _lib.stream_ptr(dev))
    return g1, g2


# ------------------------------------------------------------------------------------------------
# backward warp
# ------------------------------------------------------------------------------------------------
class WarpFunction(Function):
    @staticmethod
    def forward(ctx, x, flow, mask_mode, batch_shift=0):
        x = x.contiguous()
        flow = _f32(flow).contiguous()
        if x.dim() != 4 or flow.shape != (x.shape[0], 2, x.shape[2], x.shape[3]):
            raise UpflowHipError('warp: x [B,C,H,W] and flow [B,2,H,W] expected, got %s / %s'
                                 % (tuple(x.shape), tuple(flow.shape)))
        B, C, H, W = x.shape
        dev = _lib.check_gpu(x, flow)
        y = torch.empty_like(x)
        with torch.cuda.device(dev):
            _lib.call('upf_warp_forward', _lib.ptr(x), _lib.ptr(flow), _lib.ptr(y), B, C, H, W,
                      _lib.dtype_code(x), mask_mode, int(batch_shift), _lib.stream_ptr(dev))
        ctx.mask_mode = mask_mode
        ctx.batch_shift = int(batch_shift)
        ctx.save_for_backward(x, flow)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, flow = ctx.saved_tensors
        B, C, H, W = x.shape
        gy = gy.to(x.dtype).contiguous()
        dev = _lib.check_gpu(x, flow, gy)
        gx = torch.empty_like(x)
        gflow = torch.empty_like(flow)
        ws = torch.empty((_lib.lib().upf_warp_backward_workspace_bytes(B, C, H, W),), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(dev):
            _lib.call('upf_warp_backward', _lib.ptr(x), _lib.ptr(flow), _lib.ptr(gy), _lib.ptr(gx), _lib.ptr(gflow), _lib.ptr(ws),
                      B, C, H, W, _lib.dtype_code(x), ctx.mask_mode, ctx.batch_shift, _lib.stream_ptr(dev))
        return gx, gflow, None, None


def warp(x, flow, mask_mode='literal', batch_shift=0):
    """mask_mode None/'none' = tools.torch_warp; 'literal' = WarpingLayer_no_div; 'robust' = exact
    in-bounds predicate (non-default).  batch_shift: output item n samples
    x[(n + batch_shift) % B] (both frames of a pair stacked along the batch: shift B/2 = the other frame)."""
    return WarpFunction.apply(x, flow, _MASKS[mask_mode], batch_shift)


def _is_channel_slice(t):
    B, C, H, W = t.shape
    return t.stride()[1:] == (H * W, W, 1) and t.stride(0) >= C * H * W


def warp_into(x_view, flow, y_view, mask_mode='literal', batch_shift=0):
    """Inference-only warp whose input / output are channel slices of wider contiguous NCHW buffers (the
    concatenation buffers the convolutions read): no slot copies.  Returns y_view."""
    if x_view.shape != y_view.shape:
        raise UpflowHipError('warp_into: x / y must be equal-shape channel slices of contiguous NCHW buffers')
    xp, yp = _pitch_or_raise(x_view, 'warp_into: x'), _out_pitch_or_raise(y_view, 'warp_into: y')
    flow = _f32(flow).contiguous()
    B, C, H, W = x_view.shape
    if flow.shape != (B, 2, H, W):
        raise UpflowHipError('warp_into: flow [B,2,H,W] expected, got %s' % (tuple(flow.shape),))
    dev = x_view.device
    if not (x_view.is_cuda and y_view.is_cuda and flow.is_cuda) or x_view.dtype != y_view.dtype:
        raise UpflowHipError('warp_into: GPU tensors of one dtype expected (there is no CPU fallback)')
    with torch.cuda.device(dev):
        _lib.call('upf_warp_forward_pitched', _lib.ptr(x_view), x_view.stride(0) if B > 1 else 0, xp, _lib.ptr(flow), _lib.ptr(y_view),
                  y_view.stride(0) if B > 1 else 0, yp, B, C, H, W, _lib.dtype_code(x_view), _MASKS[mask_mode], int(batch_shift), _lib.stream_ptr(dev))
    return y_view


def warp_c8_into(x8, flow, y8, mask_mode='literal', batch_shift=0):
    """warp_into on channel-octet tensors: x8 / y8 are octet slices [B, n_oct, H, W, 8] of C8 buffers (conv_c8_forward_raw)."""
    if x8.shape != y8.shape or not _c8_view_ok(x8) or not _c8_view_ok(y8) or x8.dtype != y8.dtype:
        raise UpflowHipError('warp_c8_into: x8 / y8 must be equal-shape octet slices of contiguous C8 buffers')
    flow = _f32(flow).contiguous()
    B, n, H, W, _ = x8.shape
    if flow.shape != (B, 2, H, W):
        raise UpflowHipError('warp_c8_into: flow [B,2,H,W] expected, got %s' % (tuple(flow.shape),))
    dev = x8.device
    if not (x8.is_cuda and y8.is_cuda and flow.is_cuda):
        raise UpflowHipError('warp_c8_into: GPU tensors expected (there is no CPU fallback)')
    with torch.cuda.device(dev):
        _lib.call('upf_warp_forward_c8', _lib.ptr(x8), x8.stride(0), _lib.ptr(flow), _lib.ptr(y8), y8.stride(0),
                  B, n, H, W, _lib.dtype_code(x8), _MASKS[mask_mode], int(batch_shift), _lib.stream_ptr(dev))
    return y8


def flow_update(a, b=None, c=None, out=None):
    """out = cast(a + (b + c)) in fp32 (b, c optional 16-bit conv outputs): the per-level flow bookkeeping
    (model/upflow.py:566-572) in one launch.  a: fp32 [N,C,H,W]; out: None (new fp32 tensor), or an fp32 / 16-bit
    tensor or channel slice [N,C,H,W]."""
    a = _f32(a).contiguous()
    N = a.shape[0]
    per = a[0].numel()
    if out is None:
        out = torch.empty_like(a)
    if tuple(out.shape) != tuple(a.shape) or not _is_channel_slice(out):
        raise UpflowHipError('flow_update: out must be a [N,C,H,W] tensor or channel slice shaped like a')
    for t in (b, c):
        if t is not None and (tuple(t.shape) != tuple(a.shape) or not t.is_contiguous() or t.dtype not in (torch.bfloat16, torch.float16)):
            raise UpflowHipError('flow_update: b / c must be contiguous bf16 / fp16 tensors shaped like a')
    ref = b if b is not None else out
    if out.dtype != torch.float32 and (out.dtype not in (torch.bfloat16, torch.float16) or (b is not None and b.dtype != out.dtype)):
        raise UpflowHipError('flow_update: out must be fp32 or the 16-bit dtype of b / c')
    if not a.is_cuda or not out.is_cuda:
        raise UpflowHipError('flow_update: GPU tensors expected (there is no CPU fallback)')
    code = _lib.dtype_code(ref) if ref.dtype != torch.float32 else _lib.UPF_BF16
    with torch.cuda.device(a.device):
        _lib.call('upf_flow_update', _lib.ptr(a), _lib.ptr(b), _lib.ptr(c), _lib.ptr(out), out.stride(0),
                  int(out.dtype == torch.float32), N, per, code, _lib.stream_ptr(a.device))
    return out


class FlowSum3Function(Function):
    """a + (b + c) in fp32 (a: fp32 flow, b / c: 16-bit convolution outputs) as ONE launch under autograd — the per-level
    `flow_up + (res + fine)` of model/upflow.py:566-572, which as tensor arithmetic is two casts and two adds forward and
    as many kernels backward.  Backward: the incoming gradient itself for a, one 16-bit cast shared by b and c."""

    @staticmethod
    def forward(ctx, a, b, c):
        ctx.dt = b.dtype
        return flow_update(a, b.contiguous(), c.contiguous())

    @staticmethod
    def backward(ctx, g):
        g16 = g.to(ctx.dt) if (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) else None
        return (g if ctx.needs_input_grad[0] else None), (g16 if ctx.needs_input_grad[1] else None), (g16 if ctx.needs_input_grad[2] else None)


def flow_sum3(a, b, c):
    return FlowSum3Function.apply(a, b, c)


class SplitBatchFunction(Function):
    """x[:B], x[B:] of a stacked-direction tensor (both flow directions along the batch) as one autograd node: the backward of
    two plain slices is two zero-filled full-size tensors, two slice copies and an add (5 launches); here it is one
    concatenation of the two incoming gradients."""

    @staticmethod
    def forward(ctx, x, B):
        ctx.B = B
        ctx.meta = (tuple(x.shape), x.dtype, x.device)
        ctx.set_materialize_grads(False)
        return x[:B], x[B:]

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None and gb is None:
            return None, None
        shape, dtype, dev = ctx.meta
        g = torch.empty(shape, dtype=dtype, device=dev)
        for part, gp in ((g[:ctx.B], ga), (g[ctx.B:], gb)):
            if gp is None:
                part.zero_()
            else:
                part.copy_(gp)
        return g, None


def split_batch(x, B):
    """-> (x[:B], x[B:]); under autograd one node whose backward is a single concatenation."""
    if torch.is_grad_enabled() and x.requires_grad:
        return SplitBatchFunction.apply(x, int(B))
    return x[:B], x[B:]


# ------------------------------------------------------------------------------------------------
# flow up-sampling
# ------------------------------------------------------------------------------------------------
class FlowUpsampleFunction(Function):
    @staticmethod
    def forward(ctx, x, h, w, if_rate):
        x = _f32(x).contiguous()
        B, C, h_, w_ = x.shape
        dev = _lib.check_gpu(x)
        y = torch.empty((B, C, h, w), dtype=torch.float32, device=x.device)
        with torch.cuda.device(dev):
            _lib.call('upf_flow_upsample_forward', _lib.ptr(x), _lib.ptr(y), B, C, h_, w_, h, w, int(bool(if_rate)),
                      _lib.stream_ptr(dev))
        ctx.geom = (B, C, h_, w_, h, w, int(bool(if_rate)))
        return y

    @staticmethod
    def backward(ctx, gy):
        B, C, h_, w_, h, w, rate = ctx.geom
        gy = _f32(gy).contiguous()
        dev = _lib.check_gpu(gy)
        gx = torch.empty((B, C, h_, w_), dtype=torch.float32, device=gy.device)
        with torch.cuda.device(dev):
            _lib.call('upf_flow_upsample_backward', _lib.ptr(gy), _lib.ptr(gx), B, C, h_, w_, h, w, rate, _lib.stream_ptr(dev))
        return gx, None, None, None


def flow_upsample(x, h, w, if_rate=True):
    return FlowUpsampleFunction.apply(x, int(h), int(w), if_rate)


# ------------------------------------------------------------------------------------------------
# SGU interpolation-blend
# ------------------------------------------------------------------------------------------------
class SguBlendFunction(Function):
    @staticmethod
    def forward(ctx, flow_init, x_out, want_inter):
        flow_init = _f32(flow_init).contiguous()
        x_out = x_out.contiguous()
        B, c3, h, w = x_out.shape
        Bf, c2, Hf, Wf = flow_init.shape
        if c3 != 3 or c2 != 2 or Bf != B:
            raise UpflowHipError('sgu_blend: flow_init [B,2,Hf,Wf], x_out [B,3,h,w] expected, got %s / %s'
                                 % (tuple(flow_init.shape), tuple(x_out.shape)))
        dev = _lib.check_gpu(flow_init, x_out)
        flow_up = torch.empty_like(flow_init)
        inter_flow = torch.empty_like(flow_init) if want_inter else None
        inter_mask = torch.empty((B, 1, Hf, Wf), dtype=torch.float32, device=x_out.device) if want_inter else None
        nws = _lib.lib().upf_sgu_blend_forward_workspace_bytes(B, h, w, Hf, Wf)
        ws = torch.empty((nws,), dtype=torch.uint8, device=x_out.device) if nws else None
        with torch.cuda.device(dev):
            _lib.call('upf_sgu_blend_forward', _lib.ptr(flow_init), _lib.ptr(x_out), _lib.ptr(flow_up),
                      _lib.ptr(inter_flow), _lib.ptr(inter_mask), _lib.ptr(ws), B, h, w, Hf, Wf, _lib.dtype_code(x_out),
                      _lib.stream_ptr(dev))
        ctx.save_for_backward(flow_init, x_out)
        ctx.set_materialize_grads(False)        # (no zero tensors for the two non-differentiable outputs: two fills per call)
        if want_inter:
            ctx.mark_non_differentiable(inter_flow, inter_mask)
            return flow_up, inter_flow, inter_mask
        return flow_up, None, None

    @staticmethod
    def backward(ctx, g_up, _gi, _gm):
        if g_up is None:
            return None, None, None
        flow_init, x_out = ctx.saved_tensors
        B, _, h, w = x_out.shape
        _, _, Hf, Wf = flow_init.shape
        g_up = _f32(g_up).contiguous()
        dev = _lib.check_gpu(flow_init, x_out, g_up)
        g_init = torch.empty_like(flow_init)
        g_xo = torch.empty((B, 3, h, w), dtype=torch.float32, device=x_out.device)
        ws = torch.empty((_lib.lib().upf_sgu_blend_backward_workspace_bytes(B, h, w, Hf, Wf),), dtype=torch.uint8, device=x_out.device)
        with torch.cuda.device(dev):
            _lib.call('upf_sgu_blend_backward', _lib.ptr(flow_init), _lib.ptr(x_out), _lib.ptr(g_up), _lib.ptr(g_init),
                      _lib.ptr(g_xo), _lib.ptr(ws), B, h, w, Hf, Wf, _lib.dtype_code(x_out), _lib.stream_ptr(dev))
        return g_init, g_xo.to(x_out.dtype), None


def sgu_blend_flow16(flow_init, x_out, flow16):
    """Inference: the decoder-level blend (upflow.py:79-88 at the flow's own resolution) -> flow_up (fp32), which is ALSO stored, rounded to
    x_out's 16-bit type, into `flow16`: a [B,2,H,W] channel slice of a contiguous NCHW buffer or one octet [B,1,H,W,8] of a channel-octet
    buffer (the flow slot of the estimator's input) — one launch instead of the blend + flow_update(_c8)."""
    flow_init = _f32(flow_init).contiguous()
    x_out = x_out.contiguous()
    B, _, H, W = x_out.shape
    if tuple(flow_init.shape) != (B, 2, H, W) or x_out.shape[1] != 3 or x_out.dtype not in (torch.bfloat16, torch.float16) or flow16.dtype != x_out.dtype:
        raise UpflowHipError('sgu_blend_flow16: flow_init [B,2,H,W] fp32, x_out [B,3,H,W] 16-bit and a 16-bit flow slot of its type expected')
    c8 = flow16.dim() == 5
    if c8:
        if tuple(flow16.shape) != (B, 1, H, W, 8) or not _c8_view_ok(flow16):
            raise UpflowHipError('sgu_blend_flow16: the octet slot must be [B,1,H,W,8]')
    elif tuple(flow16.shape) != (B, 2, H, W) or not _is_channel_slice(flow16):
        raise UpflowHipError('sgu_blend_flow16: the NCHW slot must be a [B,2,H,W] channel slice of a contiguous buffer')
    dev = _lib.check_gpu(flow_init, x_out)
    flow_up = torch.empty_like(flow_init)
    with torch.cuda.device(dev):
        _lib.call('upf_sgu_blend_forward_flow16', _lib.ptr(flow_init), _lib.ptr(x_out), _lib.ptr(flow_up), _lib.ptr(flow16), flow16.stride(0), int(c8),
                  B, H, W, _lib.dtype_code(x_out), _lib.stream_ptr(dev))
    return flow_up


def sgu_blend(flow_init, x_out, output_level_flow=None, want_inter=True):
    """model/upflow.py:79-89 -> (flow_init, flow_up, inter_flow, inter_mask).  With
    `output_level_flow` the blend runs at ITS resolution and it replaces flow_init (:84-87).
    inter_flow / inter_mask are returned for API parity and are not differentiable outputs here
    (the reference never uses them downstream: upflow.py:585-587 keeps out_flow only)."""
    base = output_level_flow if output_level_flow is not None else flow_init
    flow_up, inter_flow, inter_mask = SguBlendFunction.apply(base, x_out, want_inter)
    return base, flow_up, inter_flow, inter_mask


# ------------------------------------------------------------------------------------------------
# feature normalisation
# ------------------------------------------------------------------------------------------------
class NormalizeFunction(Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        B, C, H, W = x.shape
        dev = _lib.check_gpu(x)
        y = torch.empty_like(x)
        rstd = torch.empty((B * C,), dtype=torch.float32, device=x.device)
        ws = torch.empty((_lib.lib().upf_normalize_workspace_bytes(B * C, H * W),), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(dev):
            _lib.call('upf_normalize_forward', _lib.ptr(x), _lib.ptr(y), _lib.ptr(None), _lib.ptr(rstd), _lib.ptr(ws), B * C, H * W,
                      _lib.dtype_code(x), _lib.stream_ptr(dev))
        ctx.save_for_backward(y, rstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, rstd = ctx.saved_tensors
        B, C, H, W = y.shape
        gy = gy.to(y.dtype).contiguous()
        dev = _lib.check_gpu(y, gy)
        gx = torch.empty_like(y)
        with torch.cuda.device(dev):
            _lib.call('upf_normalize_backward', _lib.ptr(y), _lib.ptr(gy), _lib.ptr(rstd), _lib.ptr(gx), B * C, H * W,
                      _lib.dtype_code(y), _lib.stream_ptr(dev))
        return gx


def normalize(x):
    """Per-sample, per-channel (x - mean) / sqrt(unbiased var + 1e-16) over H*W."""
    return NormalizeFunction.apply(x)


def normalize_pair(a, b):
    """network_tools.normalize_features((a, b)) with moments_across_channels=False,
    moments_across_images=False (model/upflow.py:110-137): statistics are NOT shared."""
    return normalize(a), normalize(b)


# ------------------------------------------------------------------------------------------------
# occlusion check (no gradient: the outputs are thresholded masks)
# ------------------------------------------------------------------------------------------------
def occ_check(flow_f, flow_b, alpha1=0.1, alpha2=0.5):
    ff = _f32(flow_f.detach()).contiguous()
    fb = _f32(flow_b.detach()).contiguous()
    B, _, H, W = ff.shape
    dev = _lib.check_gpu(ff, fb)
    o1 = torch.empty((B, 1, H, W), dtype=torch.float32, device=ff.device)
    o2 = torch.empty_like(o1)
    with torch.cuda.device(dev):
        _lib.call('upf_occ_check', _lib.ptr(ff), _lib.ptr(fb), _lib.ptr(o1), _lib.ptr(o2), B, H, W,
                  float(alpha1), float(alpha2), _lib.stream_ptr(dev))
    return o1, o2


# ------------------------------------------------------------------------------------------------
# 3x3 convolution on the matrix cores (inference, bf16 / fp16)
# ------------------------------------------------------------------------------------------------
# fp32 tensors (the parity mode) take the split-precision kernel (csrc/conv_x3.hip): this many fp16 products per operand pair
CONV_X3_NPROD = [3]


def conv3x3_pack(weight):
    """[Cout,Cin,k,k] (k = 3 or 1) -> the kernel's packed layout (done once per layer).  bf16 / fp16 weights: the 16-bit operand
    of upf_conv_forward; fp32 weights: fp16 hi / lo operand pairs for upf_conv_x3_forward."""
    w = weight.detach().contiguous()
    Cout, Cin, kh, kw = w.shape
    if kh != kw or kh not in (1, 3):
        raise UpflowHipError('conv pack: 3x3 or 1x1 kernels only')
    dev = _lib.check_gpu(w)
    if w.dtype == torch.float32:
        packed = torch.empty((_lib.lib().upf_conv_x3_packed_bytes(Cin, Cout, kh) // 2,), dtype=torch.float16, device=w.device)
        with torch.cuda.device(dev):
            _lib.call('upf_conv_x3_pack_weights', _lib.ptr(w), _lib.ptr(packed), Cin, Cout, kh, _lib.stream_ptr(dev))
        return packed
    nbytes = _lib.lib().upf_conv_packed_bytes(Cin, Cout, kh)
    packed = torch.empty((nbytes // 2,), dtype=w.dtype, device=w.device)
    with torch.cuda.device(dev):
        _lib.call('upf_conv_pack_weights', _lib.ptr(w), _lib.ptr(packed), Cin, Cout, kh, _lib.dtype_code(w), _lib.stream_ptr(dev))
    return packed


def conv3x3_supported(x_view, Cout, dilation, stride=1, kernel_size=3):
    """Shapes the matrix-core kernels take (16-bit: rows of >= 8 pixels; fp32, split precision: any size); everything else
    stays with MIOpen."""
    return (x_view.is_cuda and x_view.dtype in (torch.bfloat16, torch.float16, torch.float32) and kernel_size in (1, 3)
            and 1 <= dilation <= 16 and (stride == 1 or (stride == 2 and dilation == 1 and kernel_size == 3))
            and (x_view.shape[3] >= 8 or x_view.dtype == torch.float32))


def mfma_f16_denorm_probe(device):
    """True if the fp16 matrix instruction multiplies subnormal inputs un-flushed (the low halves of small fp32 operands)."""
    out = torch.zeros(1, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.call('upf_mfma_f16_denorm_probe', _lib.ptr(out), _lib.stream_ptr(device))
    return float(out.item()) == 2.0 ** -6


def conv_set_option(name, value):
    """Launch heuristics of the convolution (include/upflow_hip.h: "sk_grid", "small_grid", "rpw4_min");
    returns the previous value."""
    prev = _lib.lib().upf_conv_set_option(name.encode(), int(value))
    if prev == -2 ** 31:
        raise UpflowHipError('unknown convolution option %r' % name)
    return prev


def conv3x3_out_hw(H, W, stride=1):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def conv3x3_forward_raw(x_view, packed, bias32, y_view, dilation=1, leaky_slope=0.0, stride=1, kernel_size=3):
    """x_view / y_view: [B,Cin,H,W] / [B,Cout,Ho,Wo] channel slices of contiguous NCHW buffers."""
    B, Cin, H, W = x_view.shape
    Cout = y_view.shape[1]
    Ho, Wo = conv3x3_out_hw(H, W, stride)
    if tuple(y_view.shape) != (B, Cout, Ho, Wo):
        raise UpflowHipError('conv: output must be [%d,%d,%d,%d], got %s' % (B, Cout, Ho, Wo, tuple(y_view.shape)))
    xp, yp = _pitch_or_raise(x_view, 'conv: x'), _out_pitch_or_raise(y_view, 'conv: y')
    dev = x_view.device
    if x_view.dtype == torch.float32:
        if xp != W or yp != Wo:
            raise UpflowHipError('conv (fp32, split precision): contiguous rows expected (no row pitch)')
        if y_view.dtype != torch.float32 or packed.dtype != torch.float16:
            raise UpflowHipError('conv (fp32, split precision): fp32 output and weights packed from fp32 expected')
        with torch.cuda.device(dev):
            _lib.call('upf_conv_x3_forward', _lib.ptr(x_view), x_view.stride(0), _lib.ptr(packed), _lib.ptr(bias32),
                      _lib.ptr(y_view), y_view.stride(0), B, Cin, Cout, H, W, int(kernel_size), int(dilation), int(stride),
                      float(leaky_slope), int(CONV_X3_NPROD[0]), _lib.stream_ptr(dev))
        return y_view
    if y_view.dtype != x_view.dtype:
        # the OTHER 16-bit type out (the `pyramid_dtype` option): the 1x1 projections of the pyramid features only
        if kernel_size != 1 or stride != 1 or Cout > 32 or y_view.dtype not in (torch.bfloat16, torch.float16):
            raise UpflowHipError('conv: an output type other than the operands\' is offered for 1x1 convolutions with Cout <= 32 only')
        with torch.cuda.device(dev):
            _lib.call('upf_conv1x1_forward_mixed', _lib.ptr(x_view), x_view.stride(0), xp, _lib.ptr(packed), _lib.ptr(bias32), _lib.ptr(y_view),
                      y_view.stride(0), yp, 0, B, Cin, Cout, H, W, float(leaky_slope), _lib.dtype_code(x_view), _lib.dtype_code(y_view), _lib.stream_ptr(dev))
        return y_view
    with torch.cuda.device(dev):
        _lib.call('upf_conv_forward_pitched', _lib.ptr(x_view), x_view.stride(0), xp, _lib.ptr(packed), _lib.ptr(bias32),
                  _lib.ptr(y_view), y_view.stride(0), yp, B, Cin, Cout, H, W, int(kernel_size), int(dilation), int(stride),
                  float(leaky_slope), _lib.dtype_code(x_view), _lib.stream_ptr(dev))
    return y_view


def conv3x3_forward_gated_raw(x_view, packed, bias32, y_view, add, act, mask_slope):
    """3x3 stride-1 convolution whose epilogue is `act_grad`'s arithmetic (upf_conv_forward_gated): y = round16(round16(conv) + add)
    * (act > 0 ? 1 : mask_slope) — bit-identical to conv3x3_forward_raw followed by act_grad(y, act, mask_slope, add, dst=y).
    add, act (either may be None): [B,Cout,H,W] channel slices of y's dtype and row pitch."""
    B, Cin, H, W = x_view.shape
    Cout = y_view.shape[1]
    if tuple(y_view.shape) != (B, Cout, H, W):
        raise UpflowHipError('conv (gated): output must be [%d,%d,%d,%d], got %s' % (B, Cout, H, W, tuple(y_view.shape)))
    xp, yp = _pitch_or_raise(x_view, 'conv (gated): x'), _out_pitch_or_raise(y_view, 'conv (gated): y')
    if add is None and act is None:
        raise UpflowHipError('conv (gated): neither add nor act given')
    for t, name in ((add, 'add'), (act, 'act')):
        if t is None:
            continue
        if tuple(t.shape) != (B, Cout, H, W) or t.dtype != y_view.dtype or _pitch_or_raise(t, 'conv (gated): ' + name) != yp:
            raise UpflowHipError('conv (gated): %s must be a [%d,%d,%d,%d] channel slice of the output\'s dtype and row pitch' % (name, B, Cout, H, W))
    if x_view.dtype not in (torch.bfloat16, torch.float16) or y_view.dtype != x_view.dtype or not x_view.is_cuda:
        raise UpflowHipError('conv (gated): 16-bit GPU operands of one type expected (there is no CPU fallback)')
    dev = x_view.device
    with torch.cuda.device(dev):
        _lib.call('upf_conv_forward_gated', _lib.ptr(x_view), x_view.stride(0), xp, _lib.ptr(packed), _lib.ptr(bias32), _lib.ptr(y_view),
                  y_view.stride(0), yp, _lib.ptr(add), (add.stride(0) if add is not None else 0), _lib.ptr(act), (act.stride(0) if act is not None else 0),
                  float(mask_slope), B, Cin, Cout, H, W, _lib.dtype_code(x_view), _lib.stream_ptr(dev))
    return y_view


# ------------------------------------------------------------------------------------------------
# the same convolutions with operands in the channel-octet layout (csrc/conv_c8.hip; include/upflow_hip.h)
# ------------------------------------------------------------------------------------------------
def c8_empty(B, C, H, W, dtype, device):
    """A C8 tensor [B, ceil(C/8), H, W, 8]: the 8 channels of a pixel are one 16-byte entry."""
    return torch.empty((B, (C + 7) // 8, H, W, 8), dtype=dtype, device=device)


def to_c8(x):
    """NCHW -> C8 (zero padded to whole octets); plain torch ops — tests and slow paths only."""
    B, C, H, W = x.shape
    n = (C + 7) // 8
    if n * 8 != C:
        x = torch.cat([x, x.new_zeros(B, n * 8 - C, H, W)], 1)
    return x.view(B, n, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def from_c8(x8, C=None):
    """C8 -> NCHW (the first C channels)."""
    B, n, H, W, _ = x8.shape
    x = x8.permute(0, 1, 4, 2, 3).reshape(B, n * 8, H, W)
    return x if C is None else x[:, :C]


def conv_c8_k(n8_oct, C2):
    return _lib.lib().upf_conv_c8_k(int(n8_oct), int(C2))


def conv_c8_pack(weight, c8_channels=(), tail_channels=()):
    """[Cout,Cin,k,k] bf16/fp16 -> packed operand for a layer whose input is a C8 slice followed by an NCHW tail.
    c8_channels: for every channel position of the C8 slice (a whole number of octets) the input channel of `weight` it
    carries, -1 for padding; tail_channels: the same for the planes of the NCHW tail."""
    w = weight.detach().contiguous()
    Cout, Cin, kh, kw = w.shape
    if kh != kw or kh not in (1, 3):
        raise UpflowHipError('conv pack: 3x3 or 1x1 kernels only')
    c8_channels, tail_channels = list(c8_channels), list(tail_channels)
    if len(c8_channels) % 8:
        raise UpflowHipError('conv_c8_pack: the C8 slice must be whole octets')
    K = conv_c8_k(len(c8_channels) // 8, len(tail_channels))
    p8 = (len(c8_channels) + 31) // 32 * 32 if c8_channels else 0
    kmap = [-1] * K
    kmap[:len(c8_channels)] = c8_channels
    kmap[p8:p8 + len(tail_channels)] = tail_channels
    dev = _lib.check_gpu(w)
    kmap_t = torch.tensor(kmap, dtype=torch.int32, device=w.device)
    nbytes = _lib.lib().upf_conv_packed_bytes_k(K, Cout, kh)
    packed = torch.empty((nbytes // 2,), dtype=w.dtype, device=w.device)
    with torch.cuda.device(dev):
        _lib.call('upf_conv_pack_weights_kmap', _lib.ptr(w), _lib.ptr(packed), Cin, Cout, kh, _lib.ptr(kmap_t), K,
                  _lib.dtype_code(w), _lib.stream_ptr(dev))
    return packed


def conv_c8_narrow_ok(Cout, kernel_size, dilation, stride, has_tail):
    """Layers upf_conv_forward_c8_narrow takes (the 16-output-channel matrix instruction): Cout <= 16, 3x3, dilation 1, stride 1,
    octet input only."""
    return Cout <= 16 and kernel_size == 3 and dilation == 1 and stride == 1 and not has_tail


def conv_c8_pack16(weight, c8_channels):
    """conv_c8_pack for upf_conv_forward_c8_narrow (Cout <= 16): the k-map padded to whole 32-channel chunks."""
    w = weight.detach().contiguous()
    Cout, Cin, kh, kw = w.shape
    c8_channels = list(c8_channels)
    if kh != 3 or kw != 3 or len(c8_channels) % 8 or not c8_channels:
        raise UpflowHipError('conv_c8_pack16: 3x3 kernels, a C8 slice of whole octets')
    K = (len(c8_channels) + 31) // 32 * 32
    kmap = c8_channels + [-1] * (K - len(c8_channels))
    dev = _lib.check_gpu(w)
    kmap_t = torch.tensor(kmap, dtype=torch.int32, device=w.device)
    packed = torch.empty((_lib.lib().upf_conv_packed_bytes_k16(K, Cout) // 2,), dtype=w.dtype, device=w.device)
    with torch.cuda.device(dev):
        _lib.call('upf_conv_pack_weights_kmap16', _lib.ptr(w), _lib.ptr(packed), Cin, Cout, _lib.ptr(kmap_t), K,
                  _lib.dtype_code(w), _lib.stream_ptr(dev))
    return packed


def conv_c8_forward_narrow_raw(x8, packed16, bias32, y, leaky_slope=0.0):
    """conv_c8_forward_raw for a layer with Cout <= 16 packed by conv_c8_pack16 (3x3, dilation 1, stride 1, octet input)."""
    B, n, H, W, _ = x8.shape
    Cout = bias32.shape[0]
    y_is_c8 = y.dim() == 5
    if not _c8_view_ok(x8):
        raise UpflowHipError('conv_c8_narrow: x8 must be an octet slice of a contiguous C8 buffer')
    if y_is_c8:
        if not _c8_view_ok(y) or tuple(y.shape) != (B, (Cout + 7) // 8, H, W, 8):
            raise UpflowHipError('conv_c8_narrow: C8 output must be [%d,%d,%d,%d,8], got %s' % (B, (Cout + 7) // 8, H, W, tuple(y.shape)))
    elif tuple(y.shape) != (B, Cout, H, W) or y.stride()[1:] != (H * W, W, 1):
        raise UpflowHipError('conv_c8_narrow: NCHW output must be a [%d,%d,%d,%d] channel slice' % (B, Cout, H, W))
    dev = x8.device
    if not (x8.is_cuda and y.is_cuda) or x8.dtype != y.dtype:
        raise UpflowHipError('conv_c8_narrow: GPU tensors of one dtype expected (there is no CPU fallback)')
    with torch.cuda.device(dev):
        _lib.call('upf_conv_forward_c8_narrow', _lib.ptr(x8), x8.stride(0), n, _lib.ptr(packed16), _lib.ptr(bias32), _lib.ptr(y), y.stride(0),
                  int(y_is_c8), B, Cout, H, W, float(leaky_slope), _lib.dtype_code(x8), _lib.stream_ptr(dev))
    return y


def _partial_ok(partial, B, H, W):
    return (partial.dtype == torch.float32 and partial.dim() == 5 and partial.shape[0] == B and tuple(partial.shape[2:]) == (H, W, 4)
            and partial.stride()[1:] == (H * W * 4, W * 4, 4, 1))


def conv_c8_forward_split_raw(x8, packed, bias32, y8, partial, leaky_slope=0.0):
    """The merged narrow tail of a dense stack, first launch (upf_conv_forward_c8_split): ONE pass over the octet slice x8 computes
    a layer of C_main = 8 * y8.shape[1] output channels completely (bias, LeakyReLU, octets into y8) and, as the remaining rows of the
    packed operand (Cout = bias32.shape[0] <= 64 rows), the shared-input part of later layers as raw fp32 (bias included) into
    partial [B, Q, H, W, 4] (planes of channel quads: partial channel c is partial[:, c // 4, :, :, c % 4])."""
    B, n, H, W, _ = x8.shape
    Cout = bias32.shape[0]
    if not _c8_view_ok(x8) or not _c8_view_ok(y8) or tuple(y8.shape[0:1] + y8.shape[2:]) != (B, H, W, 8):
        raise UpflowHipError('conv_c8_split: x8 / y8 must be octet slices of contiguous C8 buffers of one size')
    cmain = 8 * y8.shape[1]
    if not _partial_ok(partial, B, H, W) or 4 * partial.shape[1] < (Cout - cmain + 3) // 4 * 4:
        raise UpflowHipError('conv_c8_split: partial must be fp32 [B,Q,H,W,4] (planes of channel quads, 4 Q >= the partial channels), got %s' % (tuple(partial.shape),))
    dev = x8.device
    if not (x8.is_cuda and y8.is_cuda and partial.is_cuda) or x8.dtype != y8.dtype:
        raise UpflowHipError('conv_c8_split: GPU tensors of one 16-bit dtype expected (there is no CPU fallback)')
    with torch.cuda.device(dev):
        _lib.call('upf_conv_forward_c8_split', _lib.ptr(x8), x8.stride(0), n, _lib.ptr(packed), _lib.ptr(bias32), _lib.ptr(y8), y8.stride(0), cmain,
                  _lib.ptr(partial), partial.stride(0), 4 * partial.shape[1], B, Cout, H, W, float(leaky_slope), _lib.dtype_code(x8), _lib.stream_ptr(dev))
    return y8


def conv_c8_forward_narrow_init_raw(x8, packed16, partial, offset, Cout, y, leaky_slope=0.0):
    """The merged narrow tail, a finishing launch (upf_conv_forward_c8_narrow_init): conv_c8_forward_narrow_raw whose accumulators start
    from partial channels [offset, offset + Cout) of `partial` (conv_c8_forward_split_raw) instead of from a bias."""
    B, n, H, W, _ = x8.shape
    y_is_c8 = y.dim() == 5
    if not _c8_view_ok(x8):
        raise UpflowHipError('conv_c8_narrow_init: x8 must be an octet slice of a contiguous C8 buffer')
    if y_is_c8:
        if not _c8_view_ok(y) or tuple(y.shape) != (B, (Cout + 7) // 8, H, W, 8):
            raise UpflowHipError('conv_c8_narrow_init: C8 output must be [%d,%d,%d,%d,8], got %s' % (B, (Cout + 7) // 8, H, W, tuple(y.shape)))
    elif tuple(y.shape) != (B, Cout, H, W) or y.stride()[1:] != (H * W, W, 1):
        raise UpflowHipError('conv_c8_narrow_init: NCHW output must be a [%d,%d,%d,%d] channel slice' % (B, Cout, H, W))
    if not _partial_ok(partial, B, H, W):
        raise UpflowHipError('conv_c8_narrow_init: partial must be fp32 [B,Q,H,W,4] (planes of channel quads)')
    dev = x8.device
    if not (x8.is_cuda and y.is_cuda and partial.is_cuda) or x8.dtype != y.dtype:
        raise UpflowHipError('conv_c8_narrow_init: GPU tensors of one 16-bit dtype expected (there is no CPU fallback)')
    with torch.cuda.device(dev):
        _lib.call('upf_conv_forward_c8_narrow_init', _lib.ptr(x8), x8.stride(0), n, _lib.ptr(packed16), _lib.ptr(partial), partial.stride(0), 4 * partial.shape[1],
                  int(offset), _lib.ptr(y), y.stride(0), int(y_is_c8), B, int(Cout), H, W, float(leaky_slope), _lib.dtype_code(x8), _lib.stream_ptr(dev))
    return y


def conv_pair_pack(w_a, w_b):
    """Packed operands of upf_conv_pair_forward (include/upflow_hip.h) for a 3x3 layer w_a [C1,Cin,3,3] (Cin <= 16, C1 = 16 | 32)
    followed by a 3x3 layer w_b [C2,C1,3,3] (C2 <= 32): MFMA lane order, built with torch indexing (the operands are a few KB)."""
    C1, Cin, C2 = w_a.shape[0], w_a.shape[1], w_b.shape[0]
    if tuple(w_a.shape[2:]) != (3, 3) or tuple(w_b.shape[2:]) != (3, 3) or w_b.shape[1] != C1 or Cin > 16 or C1 not in (16, 32) or C2 > 32:
        raise UpflowHipError('conv_pair_pack: 3x3 layers with Cin <= 16, C1 = 16 | 32, C2 <= 32 expected, got %s / %s' % (tuple(w_a.shape), tuple(w_b.shape)))
    dev, dt = w_a.device, w_a.dtype
    lane = torch.arange(64, device=dev)
    co, kg, j = (lane % 32).view(1, 64, 1), (lane // 32).view(1, 64, 1), torch.arange(8, device=dev).view(1, 1, 8)
    # layer A: zero-padded copy [32, 16, 10 taps] (tap 9 = the absent second tap of the last step)
    wa = torch.zeros((32, 16, 12), dtype=dt, device=dev)
    wa[:C1, :Cin, :9] = w_a.detach().reshape(C1, Cin, 9)
    if Cin <= 4:                                     # four taps per k-step: k-octet kg of step s = taps 4s + 2kg, 4s + 2kg + 1 x 4 channels
        s = torch.arange(3, device=dev).view(3, 1, 1)
        pa = wa[co.expand(3, 64, 8), (j % 4).expand(3, 64, 8), (4 * s + 2 * kg + j // 4).expand(3, 64, 8)]
    elif Cin <= 8:
        s = torch.arange(5, device=dev).view(5, 1, 1)
        pa = wa[co.expand(5, 64, 8), j.expand(5, 64, 8), (2 * s + kg).expand(5, 64, 8)]
    else:
        s = torch.arange(9, device=dev).view(9, 1, 1)
        pa = wa[co.expand(9, 64, 8), (8 * kg + j).expand(9, 64, 8), s.expand(9, 64, 8)]
    ksb = C1 // 16
    wbz = torch.zeros((32, C1, 9), dtype=dt, device=dev)
    wbz[:C2] = w_b.detach().reshape(C2, C1, 9)
    tap = torch.arange(9, device=dev).view(9, 1, 1, 1)
    ks = torch.arange(ksb, device=dev).view(1, ksb, 1, 1)
    shp = (9, ksb, 64, 8)
    pb = wbz[co.view(1, 1, 64, 1).expand(shp), (16 * ks + 8 * kg.view(1, 1, 64, 1) + j.view(1, 1, 1, 8)).expand(shp), tap.expand(shp)]
    return pa.contiguous(), pb.contiguous()


def conv_pair_forward_raw(x, packed_a, bias_a, slope_a, packed_b, bias_b, slope_b, y, strides=(1, 2)):
    """One launch of upf_conv_pair_forward: x [B,Cin,H,W] (a channel slice of a possibly row-pitched NCHW buffer, EVEN pitch) ->
    y: NCHW [B,C2,Ho,Wo] channel slice or (strides (1, 2)) octets [B,ceil(C2/8),Ho,Wo,8].  strides: (1, 2) or (2, 1)."""
    B, Cin, H, W = x.shape
    C1, C2 = bias_a.shape[0], bias_b.shape[0]
    Ho, Wo = conv3x3_out_hw(H, W, 2)
    xp = _pitch_or_raise(x, 'conv_pair: x')
    y_is_c8 = y.dim() == 5
    if y_is_c8:
        if not _c8_view_ok(y) or tuple(y.shape) != (B, (C2 + 7) // 8, Ho, Wo, 8):
            raise UpflowHipError('conv_pair: C8 output must be [%d,%d,%d,%d,8], got %s' % (B, (C2 + 7) // 8, Ho, Wo, tuple(y.shape)))
        yp = 0
    else:
        if tuple(y.shape) != (B, C2, Ho, Wo):
            raise UpflowHipError('conv_pair: NCHW output must be [%d,%d,%d,%d], got %s' % (B, C2, Ho, Wo, tuple(y.shape)))
        yp = _out_pitch_or_raise(y, 'conv_pair: y')
    dev = x.device
    if not (x.is_cuda and y.is_cuda) or x.dtype != y.dtype or x.dtype not in (torch.bfloat16, torch.float16) or packed_a.dtype != x.dtype:
        raise UpflowHipError('conv_pair: GPU tensors of one 16-bit dtype expected (there is no CPU fallback)')
    with torch.cuda.device(dev):
        _lib.call('upf_conv_pair_forward', _lib.ptr(x), x.stride(0), xp, Cin, _lib.ptr(packed_a), _lib.ptr(bias_a), float(slope_a), C1, int(strides[0]),
                  _lib.ptr(packed_b), _lib.ptr(bias_b), float(slope_b), C2, int(strides[1]), _lib.ptr(y), y.stride(0), yp, int(y_is_c8), B, H, W,
                  _lib.dtype_code(x), _lib.stream_ptr(dev))
    return y


def conv_pair_supported(x, conv_a, conv_b):
    """The fused pair applies: 16-bit GPU inference, two undilated 3x3 layers with 'same' padding and strides (1, 2) or (2, 1), Cin <= 16,
    C1 = 16 | 32, C2 <= 32, rows readable as pixel pairs (even pitch, 4-byte aligned)."""
    if torch.is_grad_enabled() or not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16) or x.dim() != 4:
        return False
    if (conv_a.stride, conv_b.stride) not in (((1, 1), (2, 2)), ((2, 2), (1, 1))):
        return False
    for c in (conv_a, conv_b):
        if c.kernel_size != (3, 3) or c.dilation != (1, 1) or c.padding != (1, 1) or c.groups != 1 or c.bias is None or c.weight.dtype != x.dtype:
            return False
    p = nchw_pitch(x)
    return (conv_a.in_channels <= 16 and conv_a.out_channels in (16, 32) and conv_b.in_channels == conv_a.out_channels and conv_b.out_channels <= 32
            and p is not None and p % 2 == 0 and x.data_ptr() % 4 == 0 and x.stride(0) % 2 == 0 and x.shape[3] >= 8)


def _c8_view_ok(t):
    B, n, H, W, e = t.shape
    return e == 8 and t.stride()[1:] == (H * W * 8, W * 8, 8, 1)


def conv_c8_supported(H, W, dtype, Cout, dilation, kernel_size, has_c8_in, has_tail, y_is_c8):
    """What upf_conv_forward_c8 takes (stride 1)."""
    if dtype not in (torch.bfloat16, torch.float16) or (W % 8 and has_tail):      # (an NCHW input part needs aligned rows: W % 8 == 0 or a pitch)
        return False
    if kernel_size == 1:
        return (not has_c8_in) and has_tail and y_is_c8 and Cout <= 32
    if dilation == 1:
        return has_c8_in or (has_tail and y_is_c8)
    return dilation in (2, 4, 8, 16) and has_c8_in and not has_tail and y_is_c8


def conv_c8_forward_raw(x8, x2, packed, bias32, y, dilation=1, leaky_slope=0.0, kernel_size=3, stride=1):
    """x8: C8 view [B, n_oct, H, W, 8] (an octet slice of a C8 buffer) or None; x2: NCHW channel slice [B, C2, H, W] or None;
    y: a C8 view [B, n_oct_out, H, W, 8] with Cout = its channel count given by bias32, or an NCHW channel slice."""
    ref = x8 if x8 is not None else x2
    B, H, W = ref.shape[0], ref.shape[2], ref.shape[3]
    Cout = bias32.shape[0]
    y_is_c8 = y.dim() == 5
    Ho, Wo = conv3x3_out_hw(H, W, stride)
    if x8 is not None and not _c8_view_ok(x8):
        raise UpflowHipError('conv_c8: x8 must be an octet slice of a contiguous C8 buffer')
    x2p = _pitch_or_raise(x2, 'conv_c8: x2') if x2 is not None else 0
    yp = 0
    if y_is_c8:
        if not _c8_view_ok(y) or tuple(y.shape) != (B, (Cout + 7) // 8, Ho, Wo, 8):
            raise UpflowHipError('conv_c8: C8 output must be [%d,%d,%d,%d,8], got %s' % (B, (Cout + 7) // 8, Ho, Wo, tuple(y.shape)))
    else:
        if tuple(y.shape) != (B, Cout, Ho, Wo):
            raise UpflowHipError('conv_c8: NCHW output must be a [%d,%d,%d,%d] channel slice' % (B, Cout, Ho, Wo))
        yp = _out_pitch_or_raise(y, 'conv_c8: y')
    dev = ref.device
    if y.dtype != ref.dtype:
        if not (x8 is None and x2 is not None and kernel_size == 1 and stride == 1 and y_is_c8 and Cout <= 32 and y.dtype in (torch.bfloat16, torch.float16)):
            raise UpflowHipError('conv_c8: an output type other than the operands\' is offered for the 1x1 NCHW -> C8 projection (Cout <= 32) only')
        with torch.cuda.device(dev):
            _lib.call('upf_conv1x1_forward_mixed', _lib.ptr(x2), x2.stride(0), x2p, _lib.ptr(packed), _lib.ptr(bias32), _lib.ptr(y), y.stride(0), 0, 1,
                      B, x2.shape[1], Cout, H, W, float(leaky_slope), _lib.dtype_code(x2), _lib.dtype_code(y), _lib.stream_ptr(dev))
        return y
    with torch.cuda.device(dev):
        _lib.call('upf_conv_forward_c8_pitched', _lib.ptr(x8), x8.stride(0) if x8 is not None else 0, x8.shape[1] if x8 is not None else 0,
                  _lib.ptr(x2), x2.stride(0) if x2 is not None else 0, x2p, x2.shape[1] if x2 is not None else 0,
                  _lib.ptr(packed), _lib.ptr(bias32), _lib.ptr(y), y.stride(0), yp, int(y_is_c8), B, Cout, H, W, int(kernel_size),
                  int(dilation), int(stride), float(leaky_slope), _lib.dtype_code(ref), _lib.stream_ptr(dev))
    return y


def conv1x1_c8_dual_raw(x2, packed, bias32, y_a, y_b, leaky_slope=0.0):
    """The 1x1 projection x2 [B,Cin,H,W] (NCHW, 16-byte aligned rows) -> octets, stored into BOTH y_a and y_b [B, ceil(Cout/8), H, W, 8]
    (upf_conv1x1_forward_c8_dual): one launch instead of two for a tensor that is the input of two dense stacks."""
    B, Cin, H, W = x2.shape
    Cout = bias32.shape[0]
    for y in (y_a, y_b):
        if y.dim() != 5 or not _c8_view_ok(y) or tuple(y.shape) != (B, (Cout + 7) // 8, H, W, 8) or y.dtype != y_a.dtype:
            raise UpflowHipError('conv1x1_c8_dual: outputs must be octet slices [%d,%d,%d,%d,8] of one type' % (B, (Cout + 7) // 8, H, W))
    xp = _pitch_or_raise(x2, 'conv1x1_c8_dual: x')
    dev = x2.device
    if not (x2.is_cuda and y_a.is_cuda and y_b.is_cuda) or x2.dtype not in (torch.bfloat16, torch.float16) or y_a.dtype not in (torch.bfloat16, torch.float16):
        raise UpflowHipError('conv1x1_c8_dual: 16-bit GPU tensors expected (there is no CPU fallback)')
    with torch.cuda.device(dev):
        _lib.call('upf_conv1x1_forward_c8_dual', _lib.ptr(x2), x2.stride(0), xp, _lib.ptr(packed), _lib.ptr(bias32), _lib.ptr(y_a), y_a.stride(0),
                  _lib.ptr(y_b), y_b.stride(0), B, Cin, Cout, H, W, float(leaky_slope), _lib.dtype_code(x2), _lib.dtype_code(y_a), _lib.stream_ptr(dev))
    return y_a


def conv_c8_set_option(name, value):
    prev = _lib.lib().upf_conv_c8_set_option(name.encode(), int(value))
    if prev == -2 ** 31:
        raise UpflowHipError('unknown C8 convolution option %r' % name)
    return prev


def conv_x3_set_option(name, value):
    """Launch heuristics of the split-precision convolution (include/upflow_hip.h: upf_conv_x3_set_option); returns the previous value."""
    prev = _lib.lib().upf_conv_x3_set_option(name.encode(), int(value))
    if prev == -2 ** 31:
        raise UpflowHipError('unknown split-precision convolution option %r' % name)
    return prev


# ------------------------------------------------------------------------------------------------
# soft census distance (photometric loss, utils/loss.py:50-91)
# ------------------------------------------------------------------------------------------------
class CensusFunction(Function):
    @staticmethod
    def forward(ctx, gray1, gray2, max_distance):
        gray1 = _f32(gray1).contiguous()
        gray2 = _f32(gray2).contiguous()
        if gray1.dim() != 4 or gray1.shape[1] != 1 or gray1.shape != gray2.shape:
            raise UpflowHipError('census: two [B,1,H,W] grey images expected, got %s / %s' % (tuple(gray1.shape), tuple(gray2.shape)))
        B, _, H, W = gray1.shape
        dev = _lib.check_gpu(gray1, gray2)
        dist = torch.empty_like(gray1)
        _lib.launch(dev, 'upf_census_forward', _lib.ptr(gray1), _lib.ptr(gray2), _lib.ptr(dist), B, H, W, int(max_distance))
        ctx.save_for_backward(gray1, gray2)
        ctx.max_distance = int(max_distance)
        return dist

    @staticmethod
    def backward(ctx, g):
        gray1, gray2 = ctx.saved_tensors
        B, _, H, W = gray1.shape
        g = _f32(g).contiguous()
        dev = _lib.check_gpu(gray1, gray2, g)
        g1 = torch.empty_like(gray1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(gray2) if ctx.needs_input_grad[1] else None
        if g1 is None and g2 is None:
            return None, None, None
        _lib.launch(dev, 'upf_census_backward', _lib.ptr(gray1), _lib.ptr(gray2), _lib.ptr(g), _lib.ptr(g1), _lib.ptr(g2), B, H, W,
                    ctx.max_distance)
        return g1, g2, None


def census_distance(gray1, gray2, max_distance=3):
    """Soft census (ternary) distance [B,1,H,W] of two grey images, one launch (csrc/misc.hip)."""
    return CensusFunction.apply(gray1, gray2, max_distance)


# ------------------------------------------------------------------------------------------------
# loss-side operators of the unsupervised training step (csrc/loss.hip, csrc/loss_variants.hip; fp32)
# ------------------------------------------------------------------------------------------------
def _lv_check(name, *tensors):
    """Strict operands: float32, contiguous, on one GPU (None is skipped); -> the device."""
    for t in tensors:
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise UpflowHipError('%s: float32 operands expected, got %s' % (name, t.dtype))
    return _lib.check_gpu(*tensors)               # (GPU, contiguous, one device)


def _partial_sums(dev, name, n, k, tensors, *scalars):
    """A deterministic reduction over n elements: the forward entry point `name(*tensors, partials, *scalars)` writes k partial
    sums per workgroup (upf_loss_partials(n) of them), which are added here in fixed order -> the k sums, on the device."""
    partials = torch.empty((_lib.lib().upf_loss_partials(n), k), dtype=torch.float32, device=dev)
    _lib.launch(dev, name, *[_lib.ptr(t) for t in tensors], _lib.ptr(partials), *scalars)
    return partials.sum(0)


def _grad_scalar(g):
    """The upstream gradient of a scalar output as the one-element fp32 device array that the backward kernels read."""
    return _f32(g).reshape(1).contiguous()


class BoundaryWarpFunction(Function):
    @staticmethod
    def forward(ctx, image, flow, start):
        image = _f32(image).contiguous()
        flow = _f32(flow).contiguous()
        B, C, Hi, Wi = image.shape
        if flow.dim() != 4 or flow.shape[0] != B or flow.shape[1] != 2:
            raise UpflowHipError('boundary_warp: image [B,C,Hi,Wi] and flow [B,2,h,w] expected, got %s / %s' % (tuple(image.shape), tuple(flow.shape)))
        start = _f32(start).to(flow.device).reshape(-1)
        if start.numel() == 2:
            start = start.repeat(B)
        if start.numel() != 2 * B:
            raise UpflowHipError('boundary_warp: start must hold (x, y) per batch item, got %d values for B=%d' % (start.numel(), B))
        start = start.contiguous()
        h, w = flow.shape[2:]
        dev = _lib.check_gpu(image, flow, start)
        out = torch.empty((B, C, h, w), dtype=torch.float32, device=flow.device)
        _lib.launch(dev, 'upf_boundary_warp_forward', _lib.ptr(image), _lib.ptr(flow), _lib.ptr(start), _lib.ptr(out), B, C, Hi, Wi, h, w)
        ctx.save_for_backward(image, flow, start)
        return out

    @staticmethod
    def backward(ctx, g):
        image, flow, start = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise UpflowHipError('boundary_warp: the gradient wrt the image is not implemented (frames are data)')
        B, C, Hi, Wi = image.shape
        h, w = flow.shape[2:]
        g = _f32(g).contiguous()
        dev = _lib.check_gpu(image, flow, g)
        gflow = torch.empty_like(flow)
        _lib.launch(dev, 'upf_boundary_warp_backward', _lib.ptr(image), _lib.ptr(flow), _lib.ptr(start), _lib.ptr(g), _lib.ptr(gflow),
                    B, C, Hi, Wi, h, w)
        return None, gflow, None


def boundary_warp(image, flow, start):
    """tools.boundary_dilated_warp.warp_im (utils/tools.py:351-499) — one gather launch; differentiable wrt the flow."""
    return BoundaryWarpFunction.apply(image, flow, start)


POINTWISE_KINDS = {'charbonnier': 0, 'L1': 1}          # UPF_LOSS_CHARBONNIER, UPF_LOSS_L1 (include/upflow_hip.h)


class PointwiseLossFunction(Function):
    """(sum over [B,C,H,W] of loss(x - y) * occ, sum of occ) for the kinds 'abs_robust' (upf_robust_loss_*), 'charbonnier' and 'L1'
    (upf_pointwise_loss_*): one kernel pair templated on the kind (csrc/loss.hip).  Strict: fp32 contiguous GPU operands."""

    @staticmethod
    def forward(ctx, x, y, occ, kind, q, eps):
        name = 'robust_loss' if kind == 'abs_robust' else 'pointwise_loss'
        if x.shape != y.shape or x.dim() != 4:
            raise UpflowHipError('%s: two [B,C,H,W] tensors expected, got %s / %s' % (name, tuple(x.shape), tuple(y.shape)))
        B, C, H, W = x.shape
        if occ is not None and tuple(occ.shape) != (B, 1, H, W):
            raise UpflowHipError('%s: occlusion mask must be [B,1,H,W], got %s' % (name, tuple(occ.shape)))
        dev = _lv_check(name, x, y, occ)
        # the two entry-point families differ in one argument: eps (abs_robust; the other kinds fix 1e-6) or the kind's code
        ctx.name = name
        ctx.scalars = (B, C, H * W, float(eps) if kind == 'abs_robust' else POINTWISE_KINDS[kind], float(q))
        sums = _partial_sums(dev, 'upf_%s_forward' % name, B * H * W, 2, (x, y, occ), *ctx.scalars)
        ctx.save_for_backward(x, y, occ)
        s_loss, s_occ = sums.unbind(0)                       # (mark and return the SAME view objects: ADVICE r2)
        ctx.mark_non_differentiable(s_occ)
        ctx.set_materialize_grads(False)                     # (no zero tensor for s_occ's gradient)
        return s_loss, s_occ

    @staticmethod
    def backward(ctx, g, _g_occ):
        if g is None:
            return (None,) * 6
        if ctx.needs_input_grad[2]:
            raise UpflowHipError('%s: the occlusion weights are treated as constants (hard masks); a mask that '
                                 'requires grad would silently get a zero gradient' % ctx.name)
        x, y, occ = ctx.saved_tensors
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        if gx is None and gy is None:
            return (None,) * 6
        coef = _grad_scalar(g)
        dev = _lib.check_gpu(x, y, coef)
        _lib.launch(dev, 'upf_%s_backward' % ctx.name, _lib.ptr(x), _lib.ptr(y), _lib.ptr(occ), _lib.ptr(coef), _lib.ptr(gx), _lib.ptr(gy),
                    *ctx.scalars)
        return gx, gy, None, None, None, None


def robust_loss_sums(x, y, occ=None, q=0.4, eps=0.01):
    """-> (sum over [B,C,H,W] of (|x - y| + eps)^q * occ, sum of occ): the 'abs_robust' term of
    network_tools.photo_loss_multi_type (model/upflow.py:265-288) as ONE deterministic reduction (differentiable wrt x, y)."""
    occ = None if occ is None else _f32(occ).contiguous()
    return PointwiseLossFunction.apply(_f32(x).contiguous(), _f32(y).contiguous(), occ, 'abs_robust', q, eps)


def grey(image):
    """[B,3,H,W] fp32 RGB -> [B,1,H,W]: 0.2989 r + 0.5870 g + 0.1140 b evaluated left to right (utils/loss.py:53-55), one launch."""
    image = _f32(image).contiguous()
    B, C, H, W = image.shape
    if C != 3:
        raise UpflowHipError('grey: an RGB image [B,3,H,W] expected, got %s' % (tuple(image.shape),))
    dev = _lib.check_gpu(image)
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=image.device)
    _lib.launch(dev, 'upf_grey_forward', _lib.ptr(image), _lib.ptr(out), B, H * W)
    return out


class MsdUpupFunction(Function):
    """One direction of the pyramid-distillation term, style 'upup' (model/upflow.py:461-487): weight * sum over the levels of
    abs_robust(upsample_flow(level flow -> label size), label, occ) — one pass over the label, one finishing launch, one backward
    launch for all levels (upf_msd_upup_forward / _backward).  apply(y, occ, weight, q, eps, *level_flows) -> scalar."""

    @staticmethod
    def forward(ctx, y, occ, weight, q, eps, *levels):
        y = _f32(y).contiguous()
        B, C, H, W = y.shape
        if C != 2 or not levels or len(levels) > 6:
            raise UpflowHipError('msd_upup: a [B,2,H,W] label and 1..6 level flows expected')
        xs = [_f32(x).contiguous() for x in levels]
        for x in xs:
            if x.dim() != 4 or x.shape[0] != B or x.shape[1] != 2:
                raise UpflowHipError('msd_upup: level flows must be [B,2,h,w], got %s' % (tuple(x.shape),))
        if occ is not None:
            occ = _f32(occ).contiguous()
            if tuple(occ.shape) != (B, 1, H, W):
                raise UpflowHipError('msd_upup: occlusion mask must be [B,1,H,W], got %s' % (tuple(occ.shape),))
            if occ.requires_grad:
                raise UpflowHipError('msd_upup: the occlusion weights are treated as constants (hard masks)')
        dev = _lib.check_gpu(y, occ, *xs)
        n = len(xs)
        nb = _lib.lib().upf_msd_upup_partials(B, H, W)
        partials = torch.empty((nb, 7), dtype=torch.float32, device=y.device)
        out2 = torch.empty((2,), dtype=torch.float32, device=y.device)
        xp = (_lib._vp * n)(*[x.data_ptr() for x in xs])
        hs = (_lib._c.c_int * n)(*[x.shape[2] for x in xs])
        ws = (_lib._c.c_int * n)(*[x.shape[3] for x in xs])
        _lib.launch(dev, 'upf_msd_upup_forward', xp, hs, ws, n, _lib.ptr(y), _lib.ptr(occ), _lib.ptr(partials), _lib.ptr(out2), B, H, W,
                    float(weight), float(eps), float(q))
        ctx.save_for_backward(y, occ, out2, *xs)
        ctx.cfg = (float(weight), float(q), float(eps))
        ctx.set_materialize_grads(False)
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        n = len(ctx.saved_tensors) - 3
        if g is None:
            return (None,) * (5 + n)
        y, occ, out2 = ctx.saved_tensors[:3]
        xs = ctx.saved_tensors[3:]
        weight, q, eps = ctx.cfg
        B, _, H, W = y.shape
        g = _grad_scalar(g)
        dev = _lib.check_gpu(y, g)
        gxs = [torch.empty_like(x) for x in xs]
        xp = (_lib._vp * n)(*[x.data_ptr() for x in xs])
        gp = (_lib._vp * n)(*[x.data_ptr() for x in gxs])
        hs = (_lib._c.c_int * n)(*[x.shape[2] for x in xs])
        ws = (_lib._c.c_int * n)(*[x.shape[3] for x in xs])
        _lib.launch(dev, 'upf_msd_upup_backward', xp, gp, hs, ws, n, _lib.ptr(y), _lib.ptr(occ), _lib.ptr(g), _lib.ptr(out2), B, H, W,
                    weight, eps, q)
        return (None, None, None, None, None) + tuple(gx if ctx.needs_input_grad[5 + i] else None for i, gx in enumerate(gxs))


def msd_upup_supported(y, levels):
    """The fused distillation term applies: GPU tensors, a [B,2,H,W] label, 1..6 level flows no larger than it and >= 2 wide."""
    return (y.is_cuda and y.dim() == 4 and y.shape[1] == 2 and 1 <= len(levels) <= 6 and y.shape[2] > 1 and y.shape[3] > 1
            and all(x.is_cuda and x.dim() == 4 and x.shape[1] == 2 and 2 <= x.shape[3] <= y.shape[3] and 1 <= x.shape[2] <= y.shape[2]
                    and (y.shape[3] - 1) / (x.shape[3] - 1) <= 250 for x in levels))


def msd_upup_loss(levels, y, occ=None, weight=1.0, q=0.4, eps=0.01):
    """weight * sum_l photo_loss_multi_type(upsample_flow(levels[l], y), y, occ, 'abs_robust') for ONE flow direction
    (model/upflow.py:461-487 with multi_scale_distillation_style 'upup'); differentiable wrt the level flows."""
    return MsdUpupFunction.apply(y, occ, weight, q, eps, *levels)


class SmoothEdgeFunction(Function):
    """Edge-aware smoothness of first (upf_smooth_edge1_*) or second (upf_smooth_edge2_*) order: one forward kernel templated on
    the order (csrc/loss_common.hpp), one gather backward per order.  Strict: fp32 contiguous GPU operands."""

    @staticmethod
    def forward(ctx, img, pred, order):
        name = 'smooth_edge%d' % order
        if img.dim() != 4 or pred.dim() != 4 or img.shape[0] != pred.shape[0] or img.shape[2:] != pred.shape[2:]:
            raise UpflowHipError('%s: img [B,Ci,H,W] and pred [B,Cp,H,W] expected, got %s / %s' % (name, tuple(img.shape), tuple(pred.shape)))
        B, Ci, H, W = img.shape
        Cp = pred.shape[1]
        if H <= order or W <= order:
            raise UpflowHipError('%s: at least %dx%d pixels' % (name, order + 1, order + 1))
        dev = _lv_check(name, img, pred)
        s = _partial_sums(dev, 'upf_%s_forward' % name, B * H * W, 2, (img, pred), B, Ci, Cp, H, W)
        ctx.save_for_backward(img, pred)
        ctx.name = name
        return s[0] / float(B * Cp * (H - order) * W) + s[1] / float(B * Cp * H * (W - order))

    @staticmethod
    def backward(ctx, g):
        img, pred = ctx.saved_tensors
        B, Ci, H, W = img.shape
        Cp = pred.shape[1]
        gup = _grad_scalar(g)
        dev = _lib.check_gpu(img, pred, gup)
        gp = torch.empty_like(pred)
        _lib.launch(dev, 'upf_%s_backward' % ctx.name, _lib.ptr(img), _lib.ptr(pred), _lib.ptr(gup), _lib.ptr(gp), B, Ci, Cp, H, W)
        return None, gp, None


def smooth_edge1(img, pred):
    """network_tools.edge_aware_smoothness_order1 (model/upflow.py:197-216) as one reduction launch + one gather backward."""
    return SmoothEdgeFunction.apply(_f32(img).contiguous(), _f32(pred).contiguous(), 1)


# ------------------------------------------------------------------------------------------------
# non-default loss variants (fp32): operands must already be fp32 contiguous NCHW on the GPU
# ------------------------------------------------------------------------------------------------
def smooth_edge2(img, pred):
    """network_tools.edge_aware_smoothness_order2 (model/upflow.py:220-243) as one reduction launch + one gather backward
    (differentiable wrt pred; the image is data)."""
    return SmoothEdgeFunction.apply(img, pred, 2)


class SmoothDeltaFunction(Function):
    @staticmethod
    def forward(ctx, flow, second_order):
        if flow.dim() != 4:
            raise UpflowHipError('smooth_delta: a [B,C,H,W] tensor expected, got %s' % (tuple(flow.shape),))
        B, C, H, W = flow.shape
        second_order = bool(second_order)
        m = 3 if second_order else 2
        if H < m or W < m:
            raise UpflowHipError('smooth_delta: at least %dx%d pixels' % (m, m))
        dev = _lv_check('smooth_delta', flow)
        k = 6 if second_order else 2
        s = _partial_sums(dev, 'upf_smooth_delta_forward', B * C * H * W, k, (flow,), B * C, H, W, int(second_order))
        n = float(B * C)
        counts = [n * H * (W - 1), n * (H - 1) * W]
        if second_order:
            counts += [n * H * (W - 2), n * (H - 1) * (W - 1), n * (H - 1) * (W - 1), n * (H - 2) * W]
        out = s[0] / counts[0]
        for i in range(1, k):                                   # the reference's order of the sum of means
            out = out + s[i] / counts[i]
        ctx.save_for_backward(flow)
        ctx.second_order = second_order
        return out

    @staticmethod
    def backward(ctx, g):
        flow, = ctx.saved_tensors
        B, C, H, W = flow.shape
        gup = _grad_scalar(g)
        dev = _lib.check_gpu(flow, gup)
        gf = torch.empty_like(flow)
        _lib.launch(dev, 'upf_smooth_delta_backward', _lib.ptr(flow), _lib.ptr(gup), _lib.ptr(gf), B * C, H, W, int(ctx.second_order))
        return gf, None


def smooth_delta(flow, second_order=False):
    """network_tools.flow_smooth_delta (model/upflow.py:245-263): mean |dx| + mean |dy| (+ the four second-difference means) as
    one reduction launch + one gather backward."""
    return SmoothDeltaFunction.apply(flow, second_order)


def pointwise_loss_sums(x, y, occ=None, kind='charbonnier', q=0.4):
    """-> (sum over [B,C,H,W] of loss(x - y) * occ, sum of occ) for the 'charbonnier' ((d^2 + 1e-6)^q) and 'L1' (|d + 1e-6|) arms of
    network_tools.photo_loss_multi_type (model/upflow.py:273-278, :284-287): ONE deterministic reduction, differentiable wrt x, y."""
    if kind not in POINTWISE_KINDS:
        raise UpflowHipError("pointwise_loss: kind must be 'charbonnier' or 'L1', got %r" % (kind,))
    return PointwiseLossFunction.apply(x, y, occ, kind, q, 0.0)


def _ssim_check(name, x, y, weight, c2, weight_epsilon):
    if x.shape != y.shape or x.dim() != 4:
        raise UpflowHipError('%s: two [B,C,H,W] tensors expected, got %s / %s' % (name, tuple(x.shape), tuple(y.shape)))
    B, C, H, W = x.shape
    if tuple(weight.shape) != (B, 1, H, W):
        raise UpflowHipError('%s: weight must be [B,1,H,W], got %s' % (name, tuple(weight.shape)))
    if H < 3 or W < 3:
        raise UpflowHipError('%s: at least 3x3 pixels (one window)' % name)
    if weight.requires_grad:
        raise UpflowHipError('%s: the gradient wrt the weight is not built (hard masks)' % name)
    if not (0.0 < float(c2) < float('inf')) or not (0.0 < float(weight_epsilon) < float('inf')):
        raise UpflowHipError('%s: c2 and weight_epsilon must be positive and finite (c1 = inf form only)' % name)
    return _lv_check(name, x, y, weight)


def _ssim_backward(ctx, gmap, coef_w, coef_u):
    x, y, weight = ctx.saved_tensors
    c2, eps = ctx.cfg
    B, C, H, W = x.shape
    gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
    gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
    if (gx is None and gy is None) or (gmap is None and coef_w is None and coef_u is None):
        return None, None
    dev = _lib.check_gpu(x, y, weight, gmap, coef_w, coef_u)
    _lib.launch(dev, 'upf_ssim_backward', _lib.ptr(x), _lib.ptr(y), _lib.ptr(weight), _lib.ptr(gmap), _lib.ptr(coef_w), _lib.ptr(coef_u),
                _lib.ptr(gx), _lib.ptr(gy), B, C, H, W, c2, eps)
    return gx, gy


class WeightedSsimFunction(Function):
    @staticmethod
    def forward(ctx, x, y, weight, c2, weight_epsilon):
        dev = _ssim_check('weighted_ssim', x, y, weight, c2, weight_epsilon)
        B, C, H, W = x.shape
        out = torch.empty((B, C, H - 2, W - 2), dtype=torch.float32, device=x.device)
        w_avg = torch.empty((B, 1, H - 2, W - 2), dtype=torch.float32, device=x.device)
        _lib.launch(dev, 'upf_ssim_forward', _lib.ptr(x), _lib.ptr(y), _lib.ptr(weight), _lib.ptr(out), _lib.ptr(w_avg), _lib.ptr(None),
                    B, C, H, W, float(c2), float(weight_epsilon))
        ctx.save_for_backward(x, y, weight)
        ctx.cfg = (float(c2), float(weight_epsilon))
        ctx.mark_non_differentiable(w_avg)
        ctx.set_materialize_grads(False)
        return out, w_avg

    @staticmethod
    def backward(ctx, gmap, _g_wavg):
        gmap = None if gmap is None else _f32(gmap).contiguous()
        gx, gy = _ssim_backward(ctx, gmap, None, None)
        return gx, gy, None, None, None


def weighted_ssim(x, y, weight, c2=9e-6, weight_epsilon=0.01):
    """network_tools.weighted_ssim (model/upflow.py:139-195) with c1 = inf -> (loss map [B,C,H-2,W-2], pooled weight [B,1,H-2,W-2]):
    one launch forward, one gather launch backward (differentiable wrt x and y; the weight is a constant)."""
    return WeightedSsimFunction.apply(x, y, weight, c2, weight_epsilon)


class SsimLossSumsFunction(Function):
    @staticmethod
    def forward(ctx, x, y, weight, c2, weight_epsilon):
        dev = _ssim_check('ssim_loss_sums', x, y, weight, c2, weight_epsilon)
        B, C, H, W = x.shape
        s_lw, s_w, s_l = _partial_sums(dev, 'upf_ssim_forward', B * (H - 2) * (W - 2), 3, (x, y, weight, None, None),
                                       B, C, H, W, float(c2), float(weight_epsilon)).unbind(0)
        ctx.save_for_backward(x, y, weight)
        ctx.cfg = (float(c2), float(weight_epsilon))
        ctx.mark_non_differentiable(s_w)
        ctx.set_materialize_grads(False)
        return s_lw, s_w, s_l

    @staticmethod
    def backward(ctx, g_lw, _g_w, g_l):
        coef_w = None if g_lw is None else _grad_scalar(g_lw)
        coef_u = None if g_l is None else _grad_scalar(g_l)
        gx, gy = _ssim_backward(ctx, None, coef_w, coef_u)
        return gx, gy, None, None, None


def ssim_loss_sums(x, y, weight, c2=9e-6, weight_epsilon=0.01):
    """-> (sum map * w_avg, sum w_avg, sum map) of weighted_ssim(x, y, weight): what photo_loss_multi_type's 'SSIM' arm
    (model/upflow.py:279-287) divides — the map is never written; one launch forward, one backward."""
    return SsimLossSumsFunction.apply(x, y, weight, c2, weight_epsilon)


def loss_variant_operands_ok(*tensors, min_hw=2):
    """The native loss variants apply: every tensor a float32 [B,C,H,W] on the GPU, at least min_hw x min_hw (the callers in
    model/upflow.py make them contiguous; the operators themselves reject a non-contiguous operand)."""
    return all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4
               and t.shape[2] >= min_hw and t.shape[3] >= min_hw for t in tensors if t is not None)


# ------------------------------------------------------------------------------------------------
# convolution under autograd on the matrix cores (training; csrc/conv3x3.hip + csrc/conv_wgrad.hip)
# ------------------------------------------------------------------------------------------------
_OPERANDS = OperandCache()      # every packed weight operand of the training path; forms: ('pack', dtype, mode), ('x3', dgrad),
#                                 ('stack', channel, width, dtype), ('stacks', slices, dtype)


def conv_pack_from_master(weight32, dtype, dgrad=False):
    """fp32 master weights [Cout,Cin,k,k] -> the MFMA kernel's packed 16-bit operand, for the forward convolution, (dgrad) for
    its data gradient (flipped, transposed kernel) or (dgrad = 2) for the data gradient of the space-to-depth form of a stride-2
    layer (a C-ABI form conv_train no longer takes: its structural zero weights spread a non-finite gradient element over a 6x6
    block, include/upflow_hip.h).  Cached per parameter VERSION (_OPERANDS): the decoder's layers are shared by the five pyramid levels, so a training
    step packs every layer once per direction instead of ten times (the optimiser's in-place update bumps the version, `.data`
    surgery moves the storage: both miss; train_caches_clear() drops everything)."""
    form = ('pack', dtype, int(dgrad))
    hit = _OPERANDS.get((weight32,), form)
    return hit if hit is not None else _OPERANDS.put((weight32,), form, _conv_pack_from_master(weight32, dtype, dgrad))


# The packed 16-bit weight copies (here and in model/pwc_modules._PackedConv*) and runtime.GraphedInference's staleness check are
# keyed on the parameters' autograd VERSION counters.  torch's FUSED optimizers (torch.optim.Adam(fused=True), ...) update the
# parameters in one multi-tensor kernel WITHOUT advancing them: a training loop that uses one would keep multiplying by the weights
# of its first step (round 4, found by the Trainer's own tests).  register_version_hook(optimizer) installs a post-step hook ON THAT
# OPTIMIZER that advances the versions of its parameters — no kernel, a few microseconds of host time per step.  train.Trainer
# registers it for its own optimizer; a custom loop around a fused optimizer must call it once.  (Round 4 installed a process-global
# hook at import time, which also touched the optimizers of unrelated models: ADVICE r4.)
def _advance_versions_after_step(optimizer, args, kwargs):
    torch.autograd.graph.increment_version([p for g in optimizer.param_groups for p in g['params']])


def register_version_hook(optimizer):
    """Advance the autograd version counters of `optimizer`'s parameters after each of its steps if it is a fused optimizer
    (see above); idempotent; returns the hook handle (None: not fused, nothing to do)."""
    if not optimizer.defaults.get('fused'):
        return None
    handle = getattr(optimizer, '_upf_version_hook', None)
    if handle is None:
        handle = optimizer.register_step_post_hook(_advance_versions_after_step)
        optimizer._upf_version_hook = handle
    return handle


def _carve(sizes, dtype, device):
    """-> (pool, views): ONE allocation and a 16-byte-aligned view of >= n elements of a 16-bit `dtype` for every n in sizes."""
    sizes = [(n + 7) // 8 * 8 for n in sizes]
    pool = torch.empty((sum(sizes),), dtype=dtype, device=device)
    return pool, list(pool.split(sizes))


def _packed_elems(Cout, Cin, k, mode):
    """Elements of the 16-bit operand conv_pack_from_master(w [Cout,Cin,k,k], dtype, mode) makes."""
    if mode == 2:
        return _lib.lib().upf_conv_packed_bytes(Cout, 4 * Cin, 3) // 2
    return _lib.lib().upf_conv_packed_bytes(Cout if mode else Cin, Cin if mode else Cout, k) // 2


# ---- every layer's operands in one launch ---------------------------------------------------------------------------------
# A training step re-packs ~60 operands (forward / data-gradient form of every layer) after the optimiser has changed the
# fp32 master weights: 60 launches of 3-5 us.  The per-layer packers above REMEMBER what was asked of each parameter
# (_OPERANDS.forms_seen); conv_prepack(weights) — called by shared_conv_grads at the start of a forward — then makes all of them
# for the current parameter versions in ONE launch (upf_conv_pack_weights_f32_multi) and the per-layer calls find them cached.
def conv_prepack(weights):
    """Pack, in one launch, every operand form the per-layer packers have been asked for so far (forward, data gradient;
    the space-to-depth data-gradient form too, if a caller asked for it) of the given fp32 master weights at their CURRENT versions; fills the same cache."""
    import ctypes
    by_dev = {}
    for w in weights:
        if not w.is_cuda or w.dtype != torch.float32 or not w.is_contiguous():
            continue
        for form in _OPERANDS.forms_seen(w):
            if form[0] == 'pack' and _OPERANDS.get((w,), form) is None:
                by_dev.setdefault((w.device, form[1]), []).append((w, form))
    for (dev, dtype), js in by_dev.items():
        if len(js) < 2:
            continue                                            # (the per-layer packer does a single one just as well)
        elems = [_packed_elems(w.shape[0], w.shape[1], w.shape[2], form[2]) for w, form in js]
        pool, outs = _carve(elems, dtype, dev)
        n = len(js)
        wp = (ctypes.c_void_p * n)(*[w.data_ptr() for w, _ in js])
        op = (ctypes.c_void_p * n)(*[t.data_ptr() for t in outs])
        ci = (ctypes.c_int * n)(*[w.shape[1] for w, _ in js])
        co = (ctypes.c_int * n)(*[w.shape[0] for w, _ in js])
        ks = (ctypes.c_int * n)(*[w.shape[2] for w, _ in js])
        dg = (ctypes.c_int * n)(*[form[2] for _, form in js])
        with torch.cuda.device(dev):
            _lib.call('upf_conv_pack_weights_f32_multi', wp, op, ci, co, ks, dg, n, _lib.dtype_code(pool), _lib.stream_ptr(dev))
        for (w, form), t, ne in zip(js, outs, elems):
            _OPERANDS.put((w,), form, t[:ne])


def _train_cache_tensors():
    """Every device tensor the training-path caches hold right now (packed operands, the zero-bias buffers)."""
    return _OPERANDS.tensors() + list(_ZERO_BIAS.values())


def train_caches_mark():
    """Snapshot taken right BEFORE a hipGraph capture of a training step: the cached tensors that exist — the OBJECTS, held for as
    long as the mark lives (OperandCache, 3)."""
    return {id(t): t for t in _train_cache_tensors()}


def train_caches_after_capture(mark):
    """Called right AFTER a capture attempt (train.Trainer._capture): the operands made during the capture are dropped from the
    cache, those from before it stay, and the full list of pre-capture tensors is RETURNED so that the trainer keeps them alive
    as long as its graph (OperandCache, 4).  The zero-bias buffers are never dropped."""
    _OPERANDS.keep_only(mark)
    return list(mark.values())


def train_caches_clear():
    """Drop every packed / derived weight operand of the training path.  NOT the zero-bias buffers: their addresses may be baked
    into a captured training graph, and nothing else holds them; a live captured trainer holds its own references to the operands
    it read (train_caches_after_capture), so clearing here cannot invalidate a graph."""
    _OPERANDS.clear()


conv_pack_cache_clear = train_caches_clear


def _conv_pack_from_master(weight32, dtype, dgrad=False):
    w = weight32.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    Cout, Cin, k, _ = w.shape
    dev = _lib.check_gpu(w)
    packed = torch.empty((_packed_elems(Cout, Cin, k, int(dgrad)),), dtype=dtype, device=w.device)
    with torch.cuda.device(dev):
        _lib.call('upf_conv_pack_weights_f32', _lib.ptr(w), _lib.ptr(packed), Cin, Cout, k, _lib.dtype_code(packed), int(dgrad), _lib.stream_ptr(dev))
    return packed


def conv_train_supported(x, weight, stride, dilation):
    """The autograd convolution on the matrix cores applies (forward at least): 16-bit NCHW input, fp32 master weights,
    1x1 or 3x3, stride 1 (dilation <= 16) or stride 2 (dilation 1), rows of >= 8 pixels."""
    if not (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and x.dim() == 4):
        return False
    Cout, Cin, k, k2 = weight.shape
    return bool(k == k2 and k in (1, 3) and x.shape[1] == Cin and conv3x3_supported(x, Cout, dilation, stride, k))


def conv_wgrad_supported(x, weight, stride, dilation):
    Cout, Cin, k, _ = weight.shape
    return bool(_lib.lib().upf_conv_wgrad_supported(Cin, Cout, x.shape[2], x.shape[3], k, dilation if k == 3 else 1, stride, _lib.dtype_code(x)))


def _is_slice(t):
    """[B,C,H,W] channel slice of a contiguous NCHW buffer (only the batch stride is free)."""
    return t.dim() == 4 and t.stride()[1:] == (t.shape[2] * t.shape[3], t.shape[3], 1)


def act_grad(src, y=None, slope=0.0, add=None, dst=None, want_bias=False):
    """dst = (src + add) * (y > 0 ? 1 : slope) over [B,C,H,W] channel slices (add, y optional; dst None: a new tensor,
    dst False: nothing stored) and, from the same pass, the first stage of the bias gradient ([C,32] fp32 partial sums;
    `conv_bias_grad_finish`).  -> (dst, partial)"""
    B, C, H, W = src.shape
    for t in (src, add, y, dst):
        if t is not None and t is not False and (not _is_slice(t) or tuple(t.shape) != (B, C, H, W) or t.dtype != src.dtype):
            raise UpflowHipError('act_grad: operands must be [B,C,H,W] channel slices of one 16-bit dtype and shape')
    if dst is None:
        dst = torch.empty((B, C, H, W), dtype=src.dtype, device=src.device)
    part = torch.empty((C, 32), dtype=torch.float32, device=src.device) if want_bias else None
    dev = src.device
    if not src.is_cuda:
        raise UpflowHipError('act_grad: GPU tensors expected (there is no CPU fallback)')
    st = lambda t: t.stride(0) if (t is not None and t is not False) else 0
    pt = lambda t: _lib.ptr(t if t is not False else None)
    with torch.cuda.device(dev):
        _lib.call('upf_act_grad', _lib.ptr(src), st(src), pt(add), st(add), pt(y), st(y), pt(dst), st(dst), _lib.ptr(part),
                  B, C, H * W, float(slope), _lib.dtype_code(src), _lib.stream_ptr(dev))
    return (dst if dst is not False else None), part


def conv_bias_grad_finish(parts, Cout):
    """Second stage of the bias gradient over the first-stage sums of 1..n uses (fixed order)."""
    gb = torch.empty((Cout,), dtype=torch.float32, device=parts[0].device)
    dev = parts[0].device
    total = None
    with torch.cuda.device(dev):
        for i in range(0, len(parts), 8):
            chunk = parts[i:i + 8]
            arr = (_lib._vp * len(chunk))(*[p.data_ptr() for p in chunk])
            out = gb if i == 0 else torch.empty_like(gb)
            _lib.call('upf_conv_bias_grad_finish', arr, len(chunk), _lib.ptr(out), Cout, _lib.stream_ptr(dev))
            total = out if total is None else total + out
    return total


def _fill_wgrad_levels(pairs):
    """ctypes array of upf_wgrad_level for the uses [(x, g), ...]; the callers check the shapes."""
    arr = (_lib.WgradLevel * len(pairs))()
    for a, (x, g) in zip(arr, pairs):
        a.x, a.x_batch_stride, a.grad_pre, a.g_batch_stride = x.data_ptr(), x.stride(0), g.data_ptr(), g.stride(0)
        a.B, a.H, a.W = x.shape[0], x.shape[2], x.shape[3]
    return arr


def _wgrad_levels(chunk, Cin, Cout):
    """The same, checked: x / g channel slices of the right shapes."""
    for x, g in chunk:
        if not (_is_slice(x) and _is_slice(g)) or x.shape[1] != Cin or g.shape[1] != Cout or x.shape[0] != g.shape[0] or x.shape[2:] != g.shape[2:]:
            raise UpflowHipError('conv_wgrad_multi: x / g must be [B,Cin,H,W] / [B,Cout,H,W] channel slices')
    return _fill_wgrad_levels(chunk)


def conv_wgrad_multi(uses, Cin, Cout, k, dilation, bias_parts=None):
    """fp32 [Cout,Cin,k,k] weight gradient over several uses [(x, g), ...] of one convolution (x: [B,Cin,H,W] slices,
    g: [B,Cout,H,W] slices of the gradient entering the pre-activation; sizes may differ per use — the pyramid levels):
    one K dimension, shared K-split launches and one ordered reduction (upf_conv_wgrad_multi).
    bias_parts (1..8 first-stage [Cout,32] buffers of act_grad, with at most 6 uses): the bias gradient is finished by the SAME
    reduction launch (upf_conv_wgrad_multi_bias) and the result is (grad_w, grad_b)."""
    dev = uses[0][0].device
    d = dilation if k == 3 else 1
    if bias_parts is not None and not (1 <= len(bias_parts) <= 8 and len(uses) <= 6):
        raise UpflowHipError('conv_wgrad_multi: the fused bias finish takes 1..8 partial buffers and one chunk of levels')
    total, gb = None, None
    with torch.cuda.device(dev):
        for i in range(0, len(uses), 6):
            chunk = uses[i:i + 6]
            arr = _wgrad_levels(chunk, Cin, Cout)
            nbytes = _lib.lib().upf_conv_wgrad_multi_workspace_bytes(arr, len(chunk), Cin, Cout, k, d)
            if nbytes < 0:
                raise UpflowHipError('conv_wgrad_multi: bad level list')
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            gw = torch.empty((Cout, Cin, k, k), dtype=torch.float32, device=dev)
            if bias_parts is not None:
                gb = torch.empty((Cout,), dtype=torch.float32, device=dev)
                parr = (_lib._vp * len(bias_parts))(*[p.data_ptr() for p in bias_parts])
                _lib.call('upf_conv_wgrad_multi_bias', arr, len(chunk), _lib.ptr(gw), _lib.ptr(ws), Cin, Cout, k, d, parr, len(bias_parts), _lib.ptr(gb),
                          _lib.dtype_code(chunk[0][0]), _lib.stream_ptr(dev))
            else:
                _lib.call('upf_conv_wgrad_multi', arr, len(chunk), _lib.ptr(gw), _lib.ptr(ws), Cin, Cout, k, d, _lib.dtype_code(chunk[0][0]), _lib.stream_ptr(dev))
            total = gw if total is None else total + gw
    return (total, gb) if bias_parts is not None else total


# ---- parameter gradients of SHARED convolutions: one contraction per step -----------------------------------------------
# The decoder (flow estimator, context network, SGU estimator) is applied at every pyramid level with the same weights
# (model/upflow.py:535-573).  Autograd would compute a weight gradient per use and add them; here every use only records
# its (x, g) pair and its bias partial sums in the parameter's sink, and a gate node between the parameter and its uses —
# which autograd runs after ALL uses — does the one multi-level contraction.
class _TailGroup(object):
    """The NARROW TAIL of a dense stack — conv_last, conv5, ... while their output channels add up to <= 64 — as ONE weight-gradient
    contraction.  The layers of a stack read nested channel suffixes of one buffer and their pre-activation gradients are adjacent
    slices of P (DenseStackTrainFunction), so  g = P[:, :sum Cout], x = the last layer's input (the whole buffer)  is a layer with
    <= 64 output channels whose gradient holds every member's as a block: dW_k = dW[co_k : co_k + Cout_k, Cin - Cin_k :].  The
    weight-gradient kernel works on 64 co x 64 ci blocks, and a launch with 2 ... 32 live output channels costs what one with 64 does
    (its time is the staging of X): the SGU estimator's four tail layers (3 + 8 + 16 + 32 channels, 70 + 70 + 70 + 58 us) and the
    flow estimator's two (2 + 32 channels, 110 + 121 us) become one launch each (round 5)."""

    def __init__(self, members):
        self.members = members                       # [(sink, co_offset, Cout, Cin)], the last layer first
        self.cout = sum(m[2] for m in members)
        self.cin = members[0][3]
        self.uses, self.result, self.pending = [], None, 0
        self.sig = None

    def take(self, sink):
        if self.result is None:
            self.result = conv_wgrad_multi(self.uses, self.cin, self.cout, 3, 1)
            self.uses, self.pending = [], len(self.members)
        for (m, co, cout, cin) in self.members:
            if m is sink:
                gw = self.result[co:co + cout, self.cin - cin:].contiguous()
                break
        else:
            raise UpflowHipError('_TailGroup: not a member')
        self.pending -= 1
        if self.pending == 0:
            self.result = None
        return gw


class _ParamSink(object):
    def __init__(self, weight, bias, dilation):
        self.weight, self.bias, self.dilation = weight, bias, int(dilation)
        self.uses, self.bias_parts = [], []
        self.group = None                            # _TailGroup: this layer's weight gradient is a block of the group's

    def finish(self):
        Cout, Cin, k, _ = self.weight.shape
        if self.group is not None and (self.group.uses or self.group.result is not None):
            gw = self.group.take(self)
            if self.uses:                            # (uses beyond the group's six levels kept their own contraction)
                gw = gw + conv_wgrad_multi(self.uses, Cin, Cout, k, self.dilation)
            gb = conv_bias_grad_finish(self.bias_parts, Cout) if self.bias_parts else None
            self.uses, self.bias_parts = [], []
            return gw, gb
        if self.uses and self.bias_parts and len(self.uses) <= 6 and len(self.bias_parts) <= 8:
            gw, gb = conv_wgrad_multi(self.uses, Cin, Cout, k, self.dilation, bias_parts=self.bias_parts)     # (one reduction launch for both)
        else:
            gw = conv_wgrad_multi(self.uses, Cin, Cout, k, self.dilation) if self.uses else None
            gb = conv_bias_grad_finish(self.bias_parts, Cout) if self.bias_parts else None
        self.uses, self.bias_parts = [], []
        return gw, gb


class _GateFunction(Function):
    @staticmethod
    def forward(ctx, sink, weight, bias):
        ctx.sink = sink
        ctx.set_materialize_grads(False)
        return weight.view_as(weight), (bias.view_as(bias) if bias is not None else None)

    @staticmethod
    def backward(ctx, gw_in, gb_in):
        gw, gb = ctx.sink.finish()                   # (gradients that a use could not defer arrive as gw_in / gb_in)
        if gw_in is not None:
            gw = gw_in if gw is None else gw + gw_in
        if gb_in is not None:
            gb = gb_in if gb is None else gb + gb_in
        return None, gw, gb


_GATES = {}


class shared_conv_grads(object):
    """with shared_conv_grads(conv_modules): every ops.conv_train / DenseStackTrainFunction use of these nn.Conv2d
    parameters inside the block defers its parameter gradients to one multi-use contraction (see _ParamSink)."""

    def __init__(self, convs):
        self.convs = [c for c in convs if c.weight.requires_grad]
        self.keys = []

    def __enter__(self):
        if torch.is_grad_enabled():
            if not getattr(shared_conv_grads, 'no_prepack', False):
                conv_prepack([c.weight for c in self.convs if c.weight.is_cuda])      # one launch for every layer's operands
            for c in self.convs:
                if id(c.weight) in _GATES or not c.weight.is_cuda:
                    continue
                sink = _ParamSink(c.weight, c.bias, c.dilation[0])
                wa, ba = _GateFunction.apply(sink, c.weight, c.bias)
                _GATES[id(c.weight)] = (wa, ba, sink)
                self.keys.append(id(c.weight))
        return self

    def __exit__(self, *exc):
        for k in self.keys:
            _GATES.pop(k, None)
        self.keys = []
        return False


def _gated(weight, bias):
    """-> (weight, bias, sink) to hand to an autograd Function: the gate's aliases inside shared_conv_grads."""
    hit = _GATES.get(id(weight))
    return hit if hit is not None else (weight, bias, None)


_ZERO_BIAS = {}


def _zero_bias(device, n):
    """A read-only fp32 zero vector (the bias operand of the data-gradient convolutions), one allocation per device."""
    z = _ZERO_BIAS.get(device)
    if z is None or z.numel() < n:
        z = _ZERO_BIAS[device] = torch.zeros(max(4096, n), dtype=torch.float32, device=device)
    return z[:n]


# ---- stride-2 layers (feature pyramid, SGU guidance) through the stride-1 gradient kernels --------------------------------
# y[i] = sum_k w[k] x[2i + k - 1] reads rows 2i-1, 2i, 2i+1 = (row i-1, phase 1), (row i, phase 0), (row i, phase 1) of the
# space-to-depth input xs[(c, p, q), i, j] = x[c, 2i+p, 2j+q] (F.pixel_unshuffle): a STRIDE-1 3x3 convolution of xs whose
# kernel w4[co, (ci,p,q), a, b] is w[co, ci, ky, kx] at (p, a) = _S2D(ky), (q, b) = _S2D(kx) and zero elsewhere.  So the
# weight gradient is the stride-1 weight gradient w.r.t. (xs, g) gathered at those positions (inside the split-K reduction,
# upf_conv_wgrad_s2d).  The data gradient is the TRANSPOSED form: the stride-1 data gradient (flipped, transposed w) of grad_pre spread
# over the even pixels of a zero grid — the same flops as the stride-1 data gradient with w4 (upf_conv_pack_weights_f32(dgrad = 2),
# shuffled back by upf_space_to_depth2), which rounds 1-6 used, but its zeros are DATA: w4's structural zero WEIGHTS turned one
# non-finite gradient element into a 6x6 block of NaN where the layer's footprint is 3x3.  4x the flops of the minimum on layers that
# hold 2 % of the step's flops — against PyTorch-ROCm's fp32 gradient kernels, their casts and NCHW<->NHWC transposes.
def space_to_depth2(t, inverse=False):
    """xs[n, c*4 + p*2 + q, i, j] = x[n, c, 2i+p, 2j+q] (= F.pixel_unshuffle(x, 2)); inverse: F.pixel_shuffle(xs, 2)."""
    t = t.contiguous()
    B, C, H, W = t.shape
    if inverse:
        C, H, W = C // 4, H * 2, W * 2
    out = torch.empty((B, C, H, W) if inverse else (B, 4 * C, H // 2, W // 2), dtype=t.dtype, device=t.device)
    dev = _lib.check_gpu(t)
    with torch.cuda.device(dev):
        _lib.call('upf_space_to_depth2', _lib.ptr(t), _lib.ptr(out), B, C, H, W, int(bool(inverse)), _lib.dtype_code(t), _lib.stream_ptr(dev))
    return out


def conv_wgrad_s2d(xs, g, Cin, Cout):
    """Weight gradient [Cout,Cin,3,3] of a stride-2 3x3 layer from its space-to-depth input xs [B,4*Cin,H/2,W/2] and the
    gradient g [B,Cout,H/2,W/2] entering its pre-activation (upf_conv_wgrad_s2d)."""
    dev = _lib.check_gpu(xs, g)
    arr = _fill_wgrad_levels([(xs, g)])
    nbytes = _lib.lib().upf_conv_wgrad_multi_workspace_bytes(arr, 1, 4 * Cin, Cout, 3, 1)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    gw = torch.empty((Cout, Cin, 3, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call('upf_conv_wgrad_s2d', arr, 1, _lib.ptr(gw), _lib.ptr(ws), Cin, Cout, _lib.dtype_code(xs), _lib.stream_ptr(dev))
    return gw


def _s2d_ok(x, weight, stride, dilation):
    Cout, Cin, k, _ = weight.shape
    H, W = x.shape[2:]
    return (stride == 2 and k == 3 and dilation == 1 and H % 2 == 0 and W % 2 == 0 and W // 2 >= 8 and x.dtype in (torch.bfloat16, torch.float16)
            and bool(_lib.lib().upf_conv_wgrad_supported(4 * Cin, Cout, H // 2, W // 2, 3, 1, 1, _lib.dtype_code(x))))


class ConvTrainFunction(Function):
    """y = LeakyReLU_slope(conv2d(x, weight, bias, padding = dilation * (k-1)/2, dilation, stride)) with 16-bit activations,
    fp32 master weights / bias and fp32 parameter gradients.  Forward on the MFMA kernel of csrc/conv3x3.hip; backward:
    the data gradient of a stride-1 layer is the same kernel on the flipped, transposed weights, the weight gradient is
    csrc/conv_wgrad.hip (stride 1, W >= 8), the LeakyReLU gradient and the first stage of the bias gradient one launch
    (upf_act_grad).  A stride-2 layer of even size (_s2d_ok) goes through the same kernels: weight gradient of its space-to-depth
    input (upf_conv_wgrad_s2d), data gradient in the transposed form (grad_pre on the even pixels of a zero grid, then the
    stride-1 data gradient); only what is left (stride-2 layers of odd size) takes PyTorch-ROCm's gradient kernels on fp32 copies.  Inside
    `shared_conv_grads` the parameter gradients are deferred to the parameter's sink (one contraction over all uses).
    Replaces nn.Conv2d + nn.LeakyReLU (model/pwc_modules.py:10-49) in training."""

    @staticmethod
    def forward(ctx, x, weight, bias, dilation, slope, stride, sink):
        x = x.contiguous()
        master = sink.weight if sink is not None else weight
        Cout, Cin, k, _ = weight.shape
        B, _, H, W = x.shape
        _lib.check_gpu(x, weight)
        Ho, Wo = conv3x3_out_hw(H, W, stride)
        y = torch.empty((B, Cout, Ho, Wo), dtype=x.dtype, device=x.device)
        b32 = bias.detach().float().contiguous() if bias is not None else torch.zeros(Cout, device=x.device)
        conv3x3_forward_raw(x, conv_pack_from_master(master, x.dtype), b32, y, dilation, slope, stride, k)
        ctx.save_for_backward(x, weight, y if slope != 0.0 else None)
        ctx.cfg = (int(dilation), float(slope), bias is not None, int(stride))
        ctx.sink = sink
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        dilation, slope, has_bias, stride = ctx.cfg
        sink = ctx.sink
        master = sink.weight if sink is not None else weight
        Cout, Cin, k, _ = weight.shape
        gy = gy.to(x.dtype).contiguous()
        _lib.check_gpu(x, gy)
        pad = dilation * (k - 1) // 2
        want_b = has_bias and ctx.needs_input_grad[2]
        if y is None:
            g, part = gy, (act_grad(gy, dst=False, want_bias=True)[1] if want_b else None)
        else:
            g, part = act_grad(gy, y, slope, want_bias=want_b)
        gx = gw = gb = None
        if _s2d_ok(x, weight, stride, dilation):
            # stride-2 layer through the stride-1 gradient kernels (see _s2d_ok): both gradients on the
            # matrix-core kernels instead of PyTorch-ROCm's fp32 kernels + casts + layout transposes
            B, _, H, W = x.shape
            if ctx.needs_input_grad[0]:
                # the transposed form (see above): zeros as data, not as weights (tests/test_hip_conv_exact.py, non-finite operands)
                up = torch.zeros((B, Cout, H, W), dtype=x.dtype, device=x.device)
                up[:, :, ::2, ::2] = g
                gx = torch.empty_like(x)
                conv3x3_forward_raw(up, conv_pack_from_master(master, x.dtype, dgrad=True), _zero_bias(x.device, Cin), gx, 1, 0.0, 1, 3)
            if ctx.needs_input_grad[1]:
                gw = conv_wgrad_s2d(space_to_depth2(x), g, Cin, Cout)
            if want_b:
                if sink is not None:
                    sink.bias_parts.append(part)
                else:
                    gb = conv_bias_grad_finish([part], Cout)
            return gx, gw, gb, None, None, None, None
        if ctx.needs_input_grad[0]:
            if stride == 1:
                gx = torch.empty_like(x)
                conv3x3_forward_raw(g, conv_pack_from_master(master, x.dtype, dgrad=True), _zero_bias(x.device, Cin), gx, dilation, 0.0, 1, k)
            else:
                gx = torch.nn.grad.conv2d_input(x.shape, weight.detach(), g.float(), stride=stride, padding=pad, dilation=dilation).to(x.dtype)
        if ctx.needs_input_grad[1]:
            if conv_wgrad_supported(x, weight, stride, dilation):
                if sink is not None:
                    sink.uses.append((x, g))
                else:
                    gw = conv_wgrad_multi([(x, g)], Cin, Cout, k, dilation)
            else:
                gw = torch.nn.grad.conv2d_weight(x.float(), weight.shape, g.float(), stride=stride, padding=pad, dilation=dilation)
        if want_b:
            if sink is not None:
                sink.bias_parts.append(part)
            else:
                gb = conv_bias_grad_finish([part], Cout)
        return gx, gw, gb, None, None, None, None


def conv_train(x, weight, bias, dilation=1, slope=0.0, stride=1):
    w, b, sink = _gated(weight, bias)
    return ConvTrainFunction.apply(x, w, b, dilation, slope, stride, sink)


# ---- the fp32 training step on the matrix cores: split-precision convolutions under autograd (csrc/conv_x3_bwd.hip) -------------
def conv_x3_pack_from_master(weight32, dgrad=False):
    """fp32 master weights [Cout,Cin,k,k] -> the split-precision kernel's packed fp16 hi / lo operand, for the forward convolution
    or (dgrad) for the data gradient of a stride-1 layer (flipped, transposed kernel).  Cached per parameter VERSION like
    conv_pack_from_master, in the same cache (_OPERANDS; train_caches_clear)."""
    form = ('x3', bool(dgrad))
    hit = _OPERANDS.get((weight32,), form)
    if hit is not None:
        return hit
    w = weight32.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        raise UpflowHipError('conv_x3_train: contiguous fp32 master weights expected')
    Cout, Cin, k, k2 = w.shape
    if k != k2 or k not in (1, 3):
        raise UpflowHipError('conv_x3_train: 3x3 or 1x1 kernels only')
    dev = _lib.check_gpu(w)
    nbytes = _lib.lib().upf_conv_x3_packed_bytes(Cout if dgrad else Cin, Cin if dgrad else Cout, k)
    packed = torch.empty((nbytes // 2,), dtype=torch.float16, device=w.device)
    with torch.cuda.device(dev):
        _lib.call('upf_conv_x3_pack_weights_dgrad' if dgrad else 'upf_conv_x3_pack_weights', _lib.ptr(w), _lib.ptr(packed), Cin, Cout, k,
                  _lib.stream_ptr(dev))
    return _OPERANDS.put((weight32,), form, packed)


def act_grad_x3(gy, y=None, slope=0.0, want_bias=False):
    """fp32 [B,C,H,W] channel slices: gs = gy * (y > 0 ? 1 : slope) * 2^s (y None: no activation), 2^s the power of two that puts
    max |gs| into [2^13, 2^14), taken on the device (upf_act_grad_x3).  -> (gs, scale slot [4] = {max bits, 2^s, 2^-s, 0},
    first-stage bias sums [C,32] of gs or None)."""
    B, C, H, W = gy.shape
    for t in (gy, y):
        if t is not None and (not _is_slice(t) or tuple(t.shape) != (B, C, H, W) or t.dtype != torch.float32):
            raise UpflowHipError('act_grad_x3: operands must be fp32 [B,C,H,W] channel slices of one shape')
    dev = _lib.check_gpu(gy, y, contiguous=False)
    gs = torch.empty((B, C, H, W), dtype=torch.float32, device=gy.device)
    slot = torch.empty((4,), dtype=torch.float32, device=gy.device)
    part = torch.empty((C, 32), dtype=torch.float32, device=gy.device) if want_bias else None
    with torch.cuda.device(dev):
        _lib.call('upf_act_grad_x3', _lib.ptr(gy), gy.stride(0), _lib.ptr(y), y.stride(0) if y is not None else 0, _lib.ptr(gs), gs.stride(0),
                  _lib.ptr(part), _lib.ptr(slot), B, C, H * W, float(slope), _lib.stream_ptr(dev))
    return gs, slot, part


def conv_x3_dgrad(gs, slot, weight32, x_shape, dilation=1, stride=1):
    """Data gradient [B,Cin,H,W] (fp32) of the split-precision convolution from the SCALED pre-activation gradient (act_grad_x3).
    Stride 1 writes the gradient's 2^-s into the header of the cached, shared packed dgrad operand of `weight32` just before the
    convolution reads it: all data gradients of one parameter must be enqueued on ONE stream (a captured step: one capture
    stream, no parallel branches that share a weight).  The Trainer and autograd's single backward stream satisfy this."""
    Cout, Cin, k, _ = weight32.shape
    B, _, H, W = x_shape
    dev = _lib.check_gpu(gs, slot, weight32)
    gx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=gs.device)
    w = weight32.detach()
    packed = conv_x3_pack_from_master(weight32, dgrad=True) if stride == 1 else None
    zb = _zero_bias(gs.device, Cin) if stride == 1 else None
    with torch.cuda.device(dev):
        _lib.call('upf_conv_x3_dgrad', _lib.ptr(gs), gs.stride(0), _lib.ptr(slot), _lib.ptr(w), _lib.ptr(packed), _lib.ptr(zb), _lib.ptr(gx),
                  gx.stride(0), B, Cin, Cout, H, W, k, int(dilation) if k == 3 else 1, int(stride), _lib.stream_ptr(dev))
    return gx


def conv_x3_wgrad(uses, Cin, Cout, k, dilation=1, stride=1, want_bias=False):
    """fp32 weight gradient [Cout,Cin,k,k] over 1..6 uses [(x, gs, slot, bias_part), ...] of one convolution (x: [B,Cin,H,W] fp32
    slices, gs / slot / bias_part from act_grad_x3): K = the pixels of all uses, deterministic split-K, and — want_bias — the bias
    gradient [Cout] from the same reduction launch (upf_conv_x3_wgrad).  A use whose slot is None holds an UN-SCALED grad_pre (taken as
    it is, no 2^-s: for O(1) gradients only — the split's absolute floor applies); its bias_part, if any, holds sums of that
    un-scaled grad_pre.  -> (grad_w, grad_b or None)"""
    import ctypes
    if not 1 <= len(uses) <= 6:
        raise UpflowHipError('conv_x3_wgrad: 1..6 uses')
    dev = uses[0][0].device
    d = int(dilation) if k == 3 else 1
    for x, g, slot, part in uses:
        B, _, H, W = x.shape
        Ho, Wo = conv3x3_out_hw(H, W, stride)
        if (not _is_slice(x) or not _is_slice(g) or x.shape[1] != Cin or tuple(g.shape) != (B, Cout, Ho, Wo)
                or x.dtype != torch.float32 or g.dtype != torch.float32):
            raise UpflowHipError('conv_x3_wgrad: x [B,%d,H,W] and g [B,%d,Ho,Wo] fp32 channel slices expected' % (Cin, Cout))
        _lib.check_gpu(x, g, slot, part, contiguous=False)
    arr = _fill_wgrad_levels([u[:2] for u in uses])
    nbytes = ctypes.c_longlong(0)
    _lib.call('upf_conv_x3_wgrad_workspace_bytes', arr, len(uses), Cin, Cout, k, d, int(stride), ctypes.byref(nbytes))
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    gw = torch.empty((Cout, Cin, k, k), dtype=torch.float32, device=dev)
    gb = torch.empty((Cout,), dtype=torch.float32, device=dev) if want_bias else None
    slots = None if all(u[2] is None for u in uses) else (ctypes.c_void_p * len(uses))(*[u[2].data_ptr() if u[2] is not None else None for u in uses])
    parts = (ctypes.c_void_p * len(uses))(*[u[3].data_ptr() for u in uses]) if want_bias else None
    with torch.cuda.device(dev):
        _lib.call('upf_conv_x3_wgrad', arr, slots, len(uses), _lib.ptr(gw), _lib.ptr(ws), Cin, Cout, k, d, int(stride), parts, _lib.ptr(gb),
                  _lib.stream_ptr(dev))
    return gw, gb


class ConvX3TrainFunction(Function):
    """y = LeakyReLU_slope(conv2d(x, weight, bias, padding = dilation * (k-1)/2, dilation, stride)) with fp32 activations, fp32
    master weights and fp32 gradients, every product on the fp16 matrix cores in split precision (three products per operand
    pair): forward csrc/conv_x3.hip, backward csrc/conv_x3_bwd.hip — the gradient entering the pre-activation is scaled by a
    per-tensor power of two taken from its device-side maximum (act_grad_x3) and un-scaled exactly by its consumers.  No
    PyTorch-ROCm convolution, no host synchronisation, bit-reproducible.  slope 0 = no activation.  3x3 (dilation 1..16 at
    stride 1, dilation 1 at stride 2) or 1x1 at stride 1; any H, W >= 1."""

    @staticmethod
    def forward(ctx, x, weight, bias, dilation, slope, stride):
        if not _is_slice(x):
            x = x.contiguous()
        Cout, Cin, k, _ = weight.shape
        B, _, H, W = x.shape
        _lib.check_gpu(x, weight, contiguous=False)
        if x.dtype != torch.float32 or weight.dtype != torch.float32:
            raise UpflowHipError('conv_x3_train: fp32 activations and fp32 weights expected')
        if not (k in (1, 3) and 1 <= dilation <= 16 and (stride == 1 or (stride == 2 and dilation == 1 and k == 3)) and x.shape[1] == Cin):
            raise UpflowHipError('conv_x3_train: unsupported geometry (k=%d dilation=%d stride=%d)' % (k, dilation, stride))
        Ho, Wo = conv3x3_out_hw(H, W, stride)
        y = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=x.device)
        b32 = bias.detach().contiguous() if bias is not None else _zero_bias(x.device, Cout)
        conv3x3_forward_raw(x, conv_x3_pack_from_master(weight), b32, y, dilation, slope, stride, k)
        ctx.save_for_backward(x, weight, y if slope != 0.0 else None)
        ctx.cfg = (int(dilation), float(slope), bias is not None, int(stride))
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        dilation, slope, has_bias, stride = ctx.cfg
        Cout, Cin, k, _ = weight.shape
        if gy.dtype != torch.float32 or not _is_slice(gy):
            gy = gy.float().contiguous()
        want_b = has_bias and ctx.needs_input_grad[2]
        gs, slot, part = act_grad_x3(gy, y, slope, want_bias=want_b)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = conv_x3_dgrad(gs, slot, weight, x.shape, dilation, stride)
        if ctx.needs_input_grad[1] or want_b:
            gw, gb = conv_x3_wgrad([(x, gs, slot, part)], Cin, Cout, k, dilation, stride, want_bias=want_b)
            if not ctx.needs_input_grad[1]:
                gw = None
        return gx, gw, gb, None, None, None


def conv_x3_train(x, weight, bias, dilation=1, slope=0.0, stride=1):
    return ConvX3TrainFunction.apply(x, weight, bias, int(dilation), float(slope), int(stride))


# ---- a whole dense stack (conv1..conv5 + conv_last) under autograd, in ONE buffer ---------------------------------------
def _stacked_dgrad_pack(masters, lo, hi_of, lo_k, f_k, dtype):
    """Packed data-gradient operand for the buffer channels [lo_k, lo_k + f_k) with respect to the pre-activation gradients
    of the layers `masters` (ordered like the gradient buffer: last layer first): the rows of each layer's kernel that
    read those channels, stacked along the (transposed) input dimension.  Cached per parameter versions."""
    owners, form = tuple(masters), ('stack', lo_k, f_k, dtype)
    hit = _OPERANDS.get(owners, form)
    if hit is not None:
        return hit
    with torch.no_grad():
        parts = [w.detach()[:, lo_k - h:lo_k - h + f_k] for w, h in zip(masters, hi_of)]
        stacked = parts[0].contiguous() if len(parts) == 1 else torch.cat(parts, dim=0)
        packed = _conv_pack_from_master(stacked.float(), dtype, dgrad=True)
    return _OPERANDS.put(owners, form, packed)


def _stack_dgrad_packs(masters, hi, slices, dtype):
    """Every data-gradient operand of a dense stack in ONE launch (upf_conv_pack_stacked_dgrad).  masters: the layers' fp32
    kernels in gradient-buffer order (last layer first), hi[j] the first buffer channel layer j reads; slices: [(first buffer
    channel, width, number of consumers = a prefix of masters)].  -> one packed operand per slice, bit-identical to
    _stacked_dgrad_pack's.  Cached per parameter versions (the same operands serve every pyramid level of a step)."""
    import ctypes
    owners, form = tuple(masters), ('stacks', tuple(slices), dtype)
    hit = _OPERANDS.get(owners, form)
    if hit is not None:
        return hit
    dev = _lib.check_gpu(*masters)
    nl, ns = len(masters), len(slices)
    for w in masters:
        if w.dtype != torch.float32 or not w.is_contiguous() or w.shape[2:] != (3, 3):
            raise UpflowHipError('dense stack: contiguous fp32 3x3 master kernels expected')
    pool, outs = _carve([_lib.lib().upf_conv_packed_bytes(sum(w.shape[0] for w in masters[:npos]), width, 3) // 2 for (c0, width, npos) in slices],
                        dtype, masters[0].device)
    wp = (ctypes.c_void_p * nl)(*[w.data_ptr() for w in masters])
    ci = (ctypes.c_int * nl)(*[w.shape[1] for w in masters])
    co = (ctypes.c_int * nl)(*[w.shape[0] for w in masters])
    hh = (ctypes.c_int * nl)(*[int(h) for h in hi])
    op = (ctypes.c_void_p * ns)(*[t.data_ptr() for t in outs])
    sc = (ctypes.c_int * ns)(*[int(c[0]) for c in slices])
    sw = (ctypes.c_int * ns)(*[int(c[1]) for c in slices])
    sn = (ctypes.c_int * ns)(*[int(c[2]) for c in slices])
    with torch.cuda.device(dev):
        _lib.call('upf_conv_pack_stacked_dgrad', wp, ci, co, hh, nl, op, sc, sw, sn, ns, _lib.dtype_code(pool), _lib.stream_ptr(dev))
    return _OPERANDS.put(owners, form, outs, alloc=pool)


class DenseStackTrainFunction(Function):
    """The dense estimator stacks (FlowEstimatorDense / the SGU mask estimator: `x = cat([conv_k(x), x])` five times, then
    conv_last; model/pwc_modules.py:250-286) under autograd without a single concatenation, in the buffer layout of the
    inference path:
        buf = [conv5 | conv4 | conv3 | conv2 | conv1 | inputs... | flow tail]
    forward: every layer reads a channel suffix of buf and writes its slice.  backward: the gradients entering the
    pre-activations live in a second buffer P = [g_last | g5 | g4 | g3 | g2 | g1]; the gradient of buffer slice k is ONE
    data-gradient convolution of the PREFIX of P that is known by then (the layers after k) with their stacked kernels —
    the sum over consumers happens in the fp32 accumulators of the matrix cores instead of in 16-bit tensor adds — followed
    by one pass (upf_act_grad) that adds the gradient arriving from outside the stack, applies the LeakyReLU mask and takes
    the bias sums.  Weight gradients: (buf suffix, P slice) pairs, deferred to the parameter sinks inside
    shared_conv_grads.  `flow_tail`: buf[:, nt:] = flow_tail + out (the refined flow the context network reads next to
    the features, model/upflow.py:566-570).
    apply(cfg, *inputs, [flow_tail], w1, b1, ..., w5, b5, w_last, b_last) -> (buf, out)"""

    @staticmethod
    def forward(ctx, cfg, *tensors):
        nin, f, slope, sinks, has_tail = cfg['n_inputs'], tuple(cfg['f']), float(cfg['slope']), cfg['sinks'], cfg['flow_tail']
        inputs = tensors[:nin]
        tail = tensors[nin] if has_tail else None
        params = tensors[nin + (1 if has_tail else 0):]
        nl = len(f) + 1
        weights, biases = params[0::2], params[1::2]
        masters = [s.weight if s is not None else w for s, w in zip(sinks, weights)]
        dt, dev = inputs[0].dtype, inputs[0].device
        B, _, H, W = inputs[0].shape
        cin = [t.shape[1] for t in inputs]
        ch_in, nt = sum(cin), sum(cin) + sum(f)
        oc = weights[-1].shape[0]
        tailc = tail.shape[1] if has_tail else 0
        buf = torch.empty((B, nt + tailc, H, W), dtype=dt, device=dev)
        o = nt - ch_in
        for t in inputs:
            buf[:, o:o + t.shape[1]].copy_(t)
            o += t.shape[1]
        hi = nt - ch_in
        for k in range(len(f)):
            b32 = biases[k].detach().float().contiguous()
            conv3x3_forward_raw(buf[:, hi:nt], conv_pack_from_master(masters[k], dt), b32, buf[:, hi - f[k]:hi], 1, slope, 1, 3)
            hi -= f[k]
        out = torch.empty((B, oc, H, W), dtype=dt, device=dev)
        conv3x3_forward_raw(buf[:, :nt], conv_pack_from_master(masters[-1], dt), biases[-1].detach().float().contiguous(), out, 1, 0.0, 1, 3)
        if has_tail:
            flow_update(tail, out, out=buf[:, nt:])
        ctx.save_for_backward(buf, *weights)
        ctx.cfg = (nin, f, slope, has_tail, cin, [t.dtype for t in inputs], tail.dtype if has_tail else None, oc)
        ctx.sinks = sinks
        ctx.set_materialize_grads(False)
        return buf, out

    @staticmethod
    def backward(ctx, g_buf, g_out):
        buf = ctx.saved_tensors[0]
        weights = ctx.saved_tensors[1:]
        nin, f, slope, has_tail, cin, in_dtypes, tail_dtype, oc = ctx.cfg
        sinks = ctx.sinks
        masters = [s.weight if s is not None else w for s, w in zip(sinks, weights)]
        dt, dev = buf.dtype, buf.device
        B, _, H, W = buf.shape
        ch_in, nf = sum(cin), len(f)
        nt = ch_in + sum(f)
        if g_buf is not None:
            g_buf = g_buf.to(dt)
            if not _is_slice(g_buf):
                g_buf = g_buf.contiguous()
        # buffer slot of layer k (k = 0..nf-1 = conv1..conv5): [lo[k], lo[k] + f[k]); its input: [lo[k] + f[k], nt)
        lo = [sum(f[k + 1:]) for k in range(nf)]
        pch = oc + sum(f)
        P = torch.empty((B, pch, H, W), dtype=dt, device=dev)
        parts = [None] * (nf + 1)
        # the last layer's output gradient (+ what arrives through the flow tail)
        if g_out is None:
            g_out = torch.zeros((B, oc, H, W), dtype=dt, device=dev)
        g_tail = g_buf[:, nt:] if (has_tail and g_buf is not None) else None
        _, parts[nf] = act_grad(g_out.to(dt).contiguous(), None, 0.0, add=g_tail, dst=P[:, :oc], want_bias=True)
        # layers in P order: last, conv5, ..., conv1;  hi_of = first buffer channel each one reads
        order = [nf] + list(range(nf - 1, -1, -1))
        hi_of = {nf: 0}
        for k in range(nf):
            hi_of[k] = lo[k] + f[k]
        zero = _zero_bias(dev, max(max(f), ch_in))
        filled = oc
        # the mask / residual pass of each layer inside its data-gradient convolution's epilogue (upf_conv_forward_gated; the
        # separate passes cost 1.1 ms of a 9.5 ms config-3 step), the bias sums of all layers by ONE pass over P afterwards
        gated = not (getattr(DenseStackTrainFunction, 'no_gated_dgrad', False) or os.environ.get('UPF_NO_GATED_DGRAD'))
        # every data-gradient operand of the stack from one launch (the first level of a step packs, the others hit the cache)
        x0 = nt - ch_in
        one_pack = len(order) <= 8 and not (getattr(DenseStackTrainFunction, 'no_stack_pack', False) or os.environ.get('UPF_NO_STACK_PACK'))
        if one_pack:
            with torch.no_grad():
                packs = _stack_dgrad_packs([masters[j] for j in order], [hi_of[j] for j in order],
                                           [(lo[k], f[k], pos) for pos, k in enumerate(order[1:], start=1)] + [(x0, ch_in, len(order))], dt)
        for pos, k in enumerate(order[1:], start=1):
            ms = [masters[j] for j in order[:pos]]
            packed = packs[pos - 1] if one_pack else _stacked_dgrad_pack(ms, lo, [hi_of[j] for j in order[:pos]], lo[k], f[k], dt)
            dst = P[:, filled:filled + f[k]]
            add_k = g_buf[:, lo[k]:lo[k] + f[k]] if g_buf is not None else None
            if gated:
                conv3x3_forward_gated_raw(P[:, :filled], packed, zero, dst, add_k, buf[:, lo[k]:lo[k] + f[k]], slope)
            else:
                conv3x3_forward_raw(P[:, :filled], packed, zero, dst, 1, 0.0, 1, 3)
                _, parts[k] = act_grad(dst, buf[:, lo[k]:lo[k] + f[k]], slope, add=add_k, dst=dst, want_bias=True)
            filled += f[k]
        if gated:
            _, part_all = act_grad(P[:, oc:], dst=False, want_bias=True)
            o = 0
            for k in order[1:]:
                parts[k] = part_all[o:o + f[k]]
                o += f[k]
        # gradient of the input slot
        grads_in = [None] * nin
        g_tail_in = None
        if any(ctx.needs_input_grad[1:1 + nin]):
            packed = packs[-1] if one_pack else _stacked_dgrad_pack([masters[j] for j in order], lo, [hi_of[j] for j in order], x0, ch_in, dt)
            gx = torch.empty((B, ch_in, H, W), dtype=dt, device=dev)
            summed = gated and g_buf is not None     # the 16-bit tensor add below, in the convolution's epilogue
            if summed:
                conv3x3_forward_gated_raw(P, packed, zero, gx, g_buf[:, x0:x0 + ch_in], None, 1.0)
            else:
                conv3x3_forward_raw(P, packed, zero, gx, 1, 0.0, 1, 3)
            o = 0
            for i in range(nin):
                if ctx.needs_input_grad[1 + i]:
                    gi = gx[:, o:o + cin[i]]
                    if not summed:                   # (summed: the channel slice itself — the consumers take slices)
                        gi = (gi + g_buf[:, x0 + o:x0 + o + cin[i]]) if g_buf is not None else gi.contiguous()
                    grads_in[i] = gi.to(in_dtypes[i])
                o += cin[i]
        if has_tail and ctx.needs_input_grad[1 + nin]:
            g_tail_in = g_tail.to(tail_dtype) if g_tail is not None else None
        # parameter gradients: x = the buffer suffix a layer read, g = its slice of P
        gparams = []
        poff = {nf: 0}
        acc = oc
        for k in range(nf - 1, -1, -1):
            poff[k] = acc
            acc += f[k]
        # the narrow tail (conv_last, conv5, ...: output channels adding up to <= 64) as one contraction: _TailGroup
        iw_of = lambda k: 1 + nin + (1 if has_tail else 0) + 2 * k
        tail, csum = [], 0
        for k in [nf] + list(range(nf - 1, -1, -1)):
            ck = oc if k == nf else f[k]
            if sinks[k] is None or not ctx.needs_input_grad[iw_of(k)] or csum + ck > 64:
                break
            tail.append(k); csum += ck
        grouped = set()
        if len(tail) >= 2 and not getattr(DenseStackTrainFunction, 'no_tail_group', False):
            grp = sinks[nf].group
            # (the sinks — and with them the group — are made anew by every forward, ops.shared_conv_grads.__enter__; within one backward
            # every level must describe the same tail: a group whose members or offsets differ — the set of trainable tail layers
            # changed between two uses — is replaced, not fed a P slice of another width: ADVICE r5)
            sig = tuple((id(sinks[k]), poff[k]) for k in tail)
            if grp is None or grp.sig != sig:
                if grp is not None and (grp.uses or grp.result is not None):
                    raise UpflowHipError('dense stack: the trainable narrow tail changed between two uses of one backward pass')
                grp = _TailGroup([(sinks[k], poff[k], (oc if k == nf else f[k]), nt - hi_of[k]) for k in tail])
                grp.sig = sig
                for k in tail:
                    sinks[k].group = grp
            if len(grp.uses) < 6:
                grp.uses.append((buf[:, :nt], P[:, :csum]))
                grouped = set(tail)
        for k in range(nf + 1):
            xk = buf[:, hi_of[k]:nt]
            gk = P[:, poff[k]:poff[k] + (oc if k == nf else f[k])]
            Cout, Cin = weights[k].shape[0], weights[k].shape[1]
            iw = 1 + nin + (1 if has_tail else 0) + 2 * k
            gw = gb = None
            if sinks[k] is not None:
                if ctx.needs_input_grad[iw] and k not in grouped:
                    sinks[k].uses.append((xk, gk))
                if ctx.needs_input_grad[iw + 1]:
                    sinks[k].bias_parts.append(parts[k])
            else:
                if ctx.needs_input_grad[iw]:
                    gw = conv_wgrad_multi([(xk, gk)], Cin, Cout, 3, 1)
                if ctx.needs_input_grad[iw + 1]:
                    gb = conv_bias_grad_finish([parts[k]], Cout)
            gparams += [gw, gb]
        return (None,) + tuple(grads_in) + ((g_tail_in,) if has_tail else ()) + tuple(gparams)


def dense_stack_train_supported(inputs, convs):
    """16-bit GPU inputs under autograd, 3x3 stride-1 undilated layers with bias, rows of >= 8 pixels (every layer then has
    its forward, data-gradient and weight-gradient kernels)."""
    x = inputs[0]
    if not (torch.is_grad_enabled() and x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and x.dim() == 4 and x.shape[3] >= 8):
        return False
    for c in convs:
        if not (c.kernel_size == (3, 3) and c.stride == (1, 1) and c.dilation == (1, 1) and c.padding == (1, 1) and c.groups == 1
                and c.bias is not None and c.weight.dtype == torch.float32 and c.weight.is_cuda):
            return False
    return True


def dense_stack_train(inputs, convs, slope, flow_tail=None):
    """inputs: the tensors whose concatenation is the stack's input ([B,C_i,H,W], 16-bit or fp32 — cast on the way into
    the buffer); convs: the nn.Conv2d modules conv1..conv5, conv_last.  -> (buf [B, sum(f) + sum(C_i) (+ tail), H, W], out)"""
    gated = [_gated(c.weight, c.bias) for c in convs]
    cfg = dict(n_inputs=len(inputs), f=[c.out_channels for c in convs[:-1]], slope=slope, sinks=[g[2] for g in gated],
               flow_tail=flow_tail is not None)
    params = []
    for w, b, _ in gated:
        params += [w, b]
    args = list(inputs) + ([flow_tail] if flow_tail is not None else []) + params
    return DenseStackTrainFunction.apply(cfg, *args)


# ---- optimiser step and loss scaling on the device (csrc/optim.hip) ---------------------------------------------------------
# The step of optim.NativeAdam: a non-finite check over all gradients, Adam (amsgrad, L2) with the loss scale divided out, and
# the scale's state machine — launches on the current stream only, so the training step stays one hipGraph.  The tensors'
# addresses travel by value in the kernel arguments (the gradients of a captured step are allocated DURING the capture, and a
# host-to-device copy of a pointer table cannot be captured): at most 4 KB per launch, so the planner below splits the tensor
# list over as many launches as it needs.
MT_TENSORS, MT_BLOCKS, MT_CHUNK = _lib.MT_TENSORS, _lib.MT_BLOCKS, _lib.MT_CHUNK
MT_KERNARG_LIMIT = 4096
_MT_LISTS = ('param', 'grad', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')


def mt_plan(sizes, max_tensors=MT_TENSORS, max_blocks=MT_BLOCKS, chunk=MT_CHUNK):
    """Assign the tensors of `sizes` (element counts) to multi-tensor launches: -> [(tensors, blocks)] per launch, `tensors` the
    indices into `sizes` the launch's table holds (at most max_tensors) and `blocks` its workgroups (at most max_blocks) as
    (slot in `tensors`, chunk): workgroup (s, c) takes elements [c * chunk, min((c + 1) * chunk, size)) of tensor tensors[s].
    Every element of every tensor belongs to exactly one workgroup of one launch; a tensor of more chunks than a launch has
    workgroups left continues in the next launch; empty tensors get none.  Pure host arithmetic."""
    launches, tensors, blocks = [], [], []
    for ti, n in enumerate(sizes):
        n = int(n)
        if n < 0 or n >= 2 ** 31:
            raise UpflowHipError('mt_plan: tensor %d has %d elements (0 .. 2^31 - 1)' % (ti, n))
        nchunks, c = (n + chunk - 1) // chunk, 0
        while c < nchunks:
            if len(blocks) == max_blocks or (len(tensors) == max_tensors and tensors[-1] != ti):
                launches.append((tensors, blocks))
                tensors, blocks = [], []
            if not tensors or tensors[-1] != ti:
                tensors.append(ti)
            take = min(nchunks - c, max_blocks - len(blocks))
            blocks += [(len(tensors) - 1, cc) for cc in range(c, c + take)]
            c += take
    if blocks:
        launches.append((tensors, blocks))
    return launches


def mt_kernarg_bytes(clipped=False):
    """Bytes of the largest argument block of the multi-tensor kernels (the Adam launch: the table, four double
    hyper-parameters, four pointers; clipped=True: the clipped Adam launch, the larger of the two — one more pointer, the clip
    coefficient)."""
    import ctypes
    return ctypes.sizeof(_lib.MtLaunch) + 4 * 8 + (5 if clipped else 4) * 8


def mt_partials(sizes):
    """The number of workgroups — one fp64 partial each in grads_sumsq_check — that mt_plan gives a tensor list: the sum of
    ceil(n / MT_CHUNK).  Pure host arithmetic."""
    return sum(len(blocks) for _, blocks in mt_plan(sizes))


class MtTables():
    """The launch tables (upf_mt_launch) of one tensor list: built once from the sizes, the addresses filled per list with
    set() — the parameters and moments when the optimiser state is made, the gradients every step."""

    def __init__(self, sizes):
        self.sizes = [int(n) for n in sizes]
        self.launches = []
        for tensors, blocks in mt_plan(self.sizes):
            L = _lib.MtLaunch()
            L.n_tensors, L.n_blocks = len(tensors), len(blocks)
            for s, ti in enumerate(tensors):
                L.numel[s] = self.sizes[ti]
            for b, (s, c) in enumerate(blocks):
                L.block_tensor[b], L.block_chunk[b] = s, c
            self.launches.append((L, tensors))
        self.device = None
        self.filled = set()
        self.n_blocks = sum(L.n_blocks for L, _ in self.launches)     # (all launches: the partials of grads_sumsq_check)

    def set(self, which, tensors):
        """which: 'param' | 'grad' | 'exp_avg' | 'exp_avg_sq' | 'max_exp_avg_sq'; tensors: fp32, contiguous, on one GPU, of
        the sizes the tables were planned for (any 4-byte alignment: DDP's gradients are views into bucket storage)."""
        if which not in _MT_LISTS or len(tensors) != len(self.sizes):
            raise UpflowHipError('MtTables.set: %r with %d tensors (planned: %d)' % (which, len(tensors), len(self.sizes)))
        for t, n in zip(tensors, self.sizes):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n or t.is_sparse:
                raise UpflowHipError('MtTables.set(%r): every tensor must be a dense contiguous fp32 GPU tensor of the planned size '
                                     '(got %s %s %s, planned %d elements); there is no CPU path' % (which, t.device, t.dtype, tuple(t.shape), n))
            if self.device is None:
                self.device = t.device
            elif t.device != self.device:
                raise UpflowHipError('operands on different devices: %s vs %s' % (self.device, t.device))
        for L, idx in self.launches:
            arr = getattr(L, which)
            for s, ti in enumerate(idx):
                arr[s] = tensors[ti].data_ptr()
        self.filled.add(which)


def _mt_scalar(t, dtype, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.numel() >= 1 and t.is_contiguous()):
        raise UpflowHipError('%s must be a %s GPU tensor' % (name, dtype))
    return _lib.ptr(t)


def grads_nonfinite_check(tables, flag):
    """flag (int32 device scalar) = 1 if any gradient element of `tables` is NaN or +-inf; never cleared here."""
    import ctypes
    if 'grad' not in tables.filled:
        raise UpflowHipError('grads_nonfinite_check: the gradients were not set')
    f = _mt_scalar(flag, torch.int32, 'flag')
    for L, _ in tables.launches:
        _lib.call('upf_grads_nonfinite_check', ctypes.byref(L), f, _lib.stream_ptr(tables.device))


def grads_sumsq_check(tables, partials, flag):
    """grads_nonfinite_check plus the sum of squares of the gradients (still multiplied by the loss scale), in double: every
    launch of `tables` writes one partial per workgroup at its own running offset into `partials`, an fp64 device vector of at
    least tables.n_blocks elements (a view into a longer vector when a step has several tables); fixed order, no atomics.
    -> the number of partials written."""
    import ctypes
    if 'grad' not in tables.filled:
        raise UpflowHipError('grads_sumsq_check: the gradients were not set')
    f = _mt_scalar(flag, torch.int32, 'flag')
    base = _mt_scalar(partials, torch.float64, 'partials')
    if partials.numel() < tables.n_blocks:
        raise UpflowHipError('grads_sumsq_check: %d partials for %d workgroups' % (partials.numel(), tables.n_blocks))
    if partials.device != tables.device:
        raise UpflowHipError('operands on different devices: %s vs %s' % (tables.device, partials.device))
    off = 0
    for L, _ in tables.launches:
        _lib.call('upf_grads_sumsq_check', ctypes.byref(L), ctypes.c_void_p(base.value + 8 * off), f, _lib.stream_ptr(tables.device))
        off += L.n_blocks
    return off


def grad_norm_clip_coef(partials, loss_scale, max_norm, norm_out, coef_out):
    """One workgroup: norm_out = (float)(sqrt(sum of `partials`, in index order) / loss_scale) — the L2 norm of the un-scaled
    gradients before clipping — and coef_out = (float)min(max_norm / (norm_out + 1e-6), 1) in double; max_norm=inf: exactly 1.
    partials fp64, the others fp32 device scalars.  A non-finite gradient makes norm_out non-finite and coef_out unspecified."""
    args = (_mt_scalar(partials, torch.float64, 'partials'), int(partials.numel()), _mt_scalar(loss_scale, torch.float32, 'loss_scale'),
            float(max_norm), _mt_scalar(norm_out, torch.float32, 'norm_out'), _mt_scalar(coef_out, torch.float32, 'coef_out'))
    _lib.check_gpu(partials, loss_scale, norm_out, coef_out)
    _lib.call('upf_grad_norm_clip_coef', *args, _lib.stream_ptr(partials.device))


def adam_amsgrad_step(tables, lr, step, loss_scale, flag, beta1, beta2, eps, weight_decay, clip_coef=None):
    """torch.optim.Adam(amsgrad=True) with L2 weight decay on the tensors of `tables`, in place; lr, step (the count BEFORE
    this step; not advanced here), loss_scale (fp32) and flag (int32) are device scalars; flag != 0: nothing is written.
    clip_coef: None, or an fp32 device scalar the un-scaled gradient is multiplied by as it is read (the gradient tensors are not
    modified); read only when flag == 0."""
    import ctypes
    if tables.filled != set(_MT_LISTS):
        raise UpflowHipError('adam_amsgrad_step: lists not set: %s' % sorted(set(_MT_LISTS) - tables.filled))
    args = (_mt_scalar(lr, torch.float32, 'lr'), _mt_scalar(step, torch.float32, 'step'),
            _mt_scalar(loss_scale, torch.float32, 'loss_scale'))
    if clip_coef is not None:
        name, args = 'upf_adam_amsgrad_step_clipped', args + (_mt_scalar(clip_coef, torch.float32, 'clip_coef'),)
    else:
        name = 'upf_adam_amsgrad_step'
    args = args + (_mt_scalar(flag, torch.int32, 'flag'),)
    for L, _ in tables.launches:
        _lib.call(name, ctypes.byref(L), *args, float(beta1), float(beta2), float(eps), float(weight_decay),
                  _lib.stream_ptr(tables.device))


def loss_scale_update(loss_scale, growth_tracker, skipped_steps, flag, steps, growth_factor, backoff_factor, growth_interval):
    """The end of a step (one thread): see upf_loss_scale_update.  steps: the fp32 device vector of the parameter groups' step
    counters, advanced by one on a step that was not skipped; growth_interval <= 0: a fixed scale."""
    _lib.check_gpu(loss_scale, growth_tracker, skipped_steps, flag, steps)
    _lib.call('upf_loss_scale_update', _mt_scalar(loss_scale, torch.float32, 'loss_scale'),
              _mt_scalar(growth_tracker, torch.int32, 'growth_tracker'), _mt_scalar(skipped_steps, torch.int32, 'skipped_steps'),
              _mt_scalar(flag, torch.int32, 'flag'), _mt_scalar(steps, torch.float32, 'steps'), int(steps.numel()),
              float(growth_factor), float(backoff_factor), int(growth_interval), _lib.stream_ptr(loss_scale.device))


# ---- batch assembly from uint8 frames (csrc/ingest.hip) -----------------------------------------------------------------------
def _ingest_constants(normalize):
    """(mean0, mean1, mean2, stddev) of the host data path — img_func is the one source of truth; normalize=False: 0, 0, 0, 1."""
    if not normalize:
        return 0.0, 0.0, 0.0, 1.0
    from .dataset.kitti_dataset import img_func
    return float(img_func.MEAN[0]), float(img_func.MEAN[1]), float(img_func.MEAN[2]), float(img_func.STDDEV)


def _u8_frames(name, t, like=None):
    if not (torch.is_tensor(t) and t.dtype == torch.uint8 and t.dim() == 4 and t.shape[3] == 3):
        raise UpflowHipError('%s: uint8 frames [B,H,W,3] expected, got %s' % (name, (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t)))
    if like is not None and t.shape != like.shape:
        raise UpflowHipError('%s: the two frame sets differ in shape: %s vs %s' % (name, tuple(like.shape), tuple(t.shape)))
    return t


def check_aug(aug, H, W, crop_size):
    """Host-side range check of a CPU `aug` [B,3] = (x, y, flip): 0 <= x <= W-pw, 0 <= y <= H-ph, else ValueError (nothing is
    clamped silently; a DEVICE aug cannot be looked at without a synchronisation — the kernel clamps it)."""
    ph, pw = int(crop_size[0]), int(crop_size[1])
    if not (0 < ph <= H and 0 < pw <= W):
        raise ValueError('crop_size %r does not fit the %d x %d frames' % (tuple(crop_size), H, W))
    if aug.dim() != 2 or aug.shape[1] != 3 or aug.dtype not in (torch.int32, torch.int64):
        raise ValueError('aug: an integer tensor [B,3] = (x, y, flip) expected, got %s %s' % (tuple(aug.shape), aug.dtype))
    if not aug.is_cuda and aug.numel():
        x, y = aug[:, 0], aug[:, 1]
        if int(x.min()) < 0 or int(x.max()) > W - pw or int(y.min()) < 0 or int(y.max()) > H - ph:
            raise ValueError('aug: crop origin outside 0 <= x <= %d, 0 <= y <= %d (x in [%d, %d], y in [%d, %d])'
                             % (W - pw, H - ph, int(x.min()), int(x.max()), int(y.min()), int(y.max())))


def _frames_u8_assemble(name, f1, f2, aug, ph, pw, normalize, want_start):
    dev = _lib.check_gpu(f1, f2, aug)
    B, H, W, _ = f1.shape
    if aug is not None and (aug.dtype != torch.int32 or tuple(aug.shape) != (B, 3)):
        raise UpflowHipError('%s: aug must be int32 [%d,3], got %s %s' % (name, B, tuple(aug.shape), aug.dtype))
    if not (0 <= ph <= H and 0 <= pw <= W and (ph > 0) == (pw > 0)):
        raise UpflowHipError('%s: crop %d x %d does not fit the %d x %d frames' % (name, ph, pw, H, W))
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=f1.device)   # noqa: E731
    raw1, raw2 = new(B, 3, H, W), (new(B, 3, H, W) if f2 is not None else None)
    crop1 = new(B, 3, ph, pw) if ph else None
    crop2 = new(B, 3, ph, pw) if ph and f2 is not None else None
    start = new(B, 2, 1, 1) if want_start else None
    _lib.launch(dev, 'upf_frames_u8_assemble', _lib.ptr(f1), _lib.ptr(f2), _lib.ptr(aug), _lib.ptr(raw1), _lib.ptr(raw2),
                _lib.ptr(crop1), _lib.ptr(crop2), _lib.ptr(start), B, H, W, ph, pw, *_ingest_constants(normalize))
    return raw1, raw2, crop1, crop2, start


def frames_from_u8(u8, flip=None, normalize=True):
    """uint8 frames [B,H,W,3] -> fp32 [B,3,H,W], the bits of img_func.get_process_img_only_img + np_2_tensor
    (dataset/kitti_dataset.py:62-80): (u8 - MEAN) / STDDEV in float64 rounded once to fp32, transposed; one launch.
    flip: optional int32 device tensor [B], != 0 mirrors that item horizontally."""
    _u8_frames('frames_from_u8', u8)
    _lib.check_gpu(u8, flip)
    aug = None
    if flip is not None:
        if flip.dtype != torch.int32 or tuple(flip.shape) != (u8.shape[0],):
            raise UpflowHipError('frames_from_u8: flip must be int32 [%d], got %s %s' % (u8.shape[0], tuple(flip.shape), flip.dtype))
        aug = torch.zeros((u8.shape[0], 3), dtype=torch.int32, device=u8.device)
        aug[:, 2] = flip
    return _frames_u8_assemble('frames_from_u8', u8, None, aug, 0, 0, normalize, False)[0]


def assemble_train_batch(frames1_u8, frames2_u8, aug, crop_size, normalize=True):
    """The training batch of kitti_data_with_start_point (dataset/kitti_dataset.py:268-342; train.synthetic_train_batch has the
    same keys) from uint8 frames [B,H,W,3] and aug int32 [B,3] = (x, y, flip), in ONE launch that reads aug on the device:
    {'im1', 'im2': the crops [B,3,ph,pw]; 'im1_raw', 'im2_raw' [B,3,H,W]; 'start' [B,2,1,1] = (x, y)}, bit for bit the host path's
    tensors.  A CPU aug is range-checked here (ValueError) and uploaded; a device aug is clamped by the kernel."""
    _u8_frames('assemble_train_batch', frames1_u8)
    _u8_frames('assemble_train_batch', frames2_u8, like=frames1_u8)
    ph, pw = int(crop_size[0]), int(crop_size[1])
    check_aug(aug, frames1_u8.shape[1], frames1_u8.shape[2], (ph, pw))
    _lib.check_gpu(frames1_u8, frames2_u8)
    aug = aug.to(device=frames1_u8.device, dtype=torch.int32, non_blocking=True).contiguous()
    raw1, raw2, crop1, crop2, start = _frames_u8_assemble('assemble_train_batch', frames1_u8, frames2_u8, aug, ph, pw, normalize, True)
    return {'im1': crop1, 'im2': crop2, 'im1_raw': raw1, 'im2_raw': raw2, 'start': start}


def _flip_or_raise(name, flip, B):
    if flip is not None and (not torch.is_tensor(flip) or flip.dtype != torch.int32 or tuple(flip.shape) != (B,)):
        raise UpflowHipError('%s: flip must be an int32 tensor [%d], got %s' % (name, B, (tuple(flip.shape), flip.dtype) if torch.is_tensor(flip) else type(flip)))
    return flip


def stack_frames_u8(frames1_u8, frames2_u8, dtype, dec_dtype=None, pitched=True, normalize=True, flip=None, out=None, out_dec=None):
    """The network's stacked input straight from uint8 frames [B,H,W,3]: X [2B,3,H,W] of `dtype`, items n < B = frames1_u8[n],
    items n + B = frames2_u8[n] (UPFlow_net._forward_stacked), every value the bits of frames_from_u8(...).to(dtype) — in ONE
    launch that reads each source byte once (upf_frames_u8_stack16).  dec_dtype (the decoder's type where to_inference gave it
    another 16-bit type than the pyramid's): a second tensor Xd of that type from the same launch -> (X, Xd); None or `dtype`:
    X alone.  Outputs are ops.empty_nchw(pitched=pitched) tensors unless `out` / `out_dec` are given ([2B,3,H,W] of the type,
    contiguous rows or rows padded as ops.empty_nchw pads them).  flip: optional int32 device tensor [B], != 0 mirrors that item
    of both frame sets.  dtype = torch.float32 (the parity mode): upf_frames_u8_assemble writes the two halves of a contiguous X."""
    who = 'stack_frames_u8'
    _u8_frames(who, frames1_u8)
    _u8_frames(who, frames2_u8, like=frames1_u8)
    B, H, W, _ = frames1_u8.shape
    dev = _lib.check_gpu(frames1_u8, frames2_u8, _flip_or_raise(who, flip, B))
    if dtype not in _lib._DTYPES or (dec_dtype is not None and dec_dtype not in _lib._DTYPES):
        raise UpflowHipError('%s: float32 / float16 / bfloat16 outputs only, got %s / %s' % (who, dtype, dec_dtype))
    dual = dec_dtype is not None and dec_dtype != dtype
    if dual and torch.float32 in (dtype, dec_dtype):
        raise UpflowHipError('%s: a second output type is for two 16-bit types (got %s and %s)' % (who, dtype, dec_dtype))
    if out_dec is not None and not dual:
        raise UpflowHipError('%s: out_dec given without a dec_dtype that differs from dtype' % who)
    shape = (2 * B, 3, H, W)
    outs = []
    for name, t, dt in (('out', out, dtype), ('out_dec', out_dec, dec_dtype))[:2 if dual else 1]:
        if t is None:
            t = empty_nchw(shape, dt, dev, pitched=pitched)
        elif not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or t.device != dev:
            raise UpflowHipError('%s: `%s` must be a %s tensor %s on %s' % (who, name, dt, shape, dev))
        outs.append((t, _out_pitch_or_raise(t, '%s: `%s`' % (who, name))))
    consts = _ingest_constants(normalize)
    X, px = outs[0]
    if dtype == torch.float32:
        if not X.is_contiguous():
            raise UpflowHipError('%s: a float32 `out` must be contiguous' % who)
        aug = None
        if flip is not None:
            aug = torch.zeros((B, 3), dtype=torch.int32, device=dev)
            aug[:, 2] = flip
        _lib.launch(dev, 'upf_frames_u8_assemble', _lib.ptr(frames1_u8), _lib.ptr(frames2_u8), _lib.ptr(aug), _lib.ptr(X[:B]), _lib.ptr(X[B:]),
                    None, None, None, B, H, W, 0, 0, *consts)
        return X
    Xd, pd = outs[1] if dual else (None, 0)
    _lib.launch(dev, 'upf_frames_u8_stack16', _lib.ptr(frames1_u8), _lib.ptr(frames2_u8), _lib.ptr(flip),
                _lib.ptr(X), _lib.dtype_code(X), px, X.stride(0), _lib.ptr(Xd), _lib.dtype_code(Xd) if dual else 0, pd, Xd.stride(0) if dual else 0,
                B, H, W, *consts)
    return (X, Xd) if dual else X


# ---- KITTI scoring from the uint16 ground truth (csrc/score.hip) ------------------------------------------------------------------
SCORE_ROW = 12          # doubles per result row: EPE all, F1 %, EPE noc, EPE occluded-only, the seven sums, the batch size


def kitti_score(pred, gt_occ_u16, gt_noc_u16, out=None):
    """The four KITTI numbers of one batch (Evaluation_bench's flow_error_avg x 3 and outlier_pct) and the sums behind them as ONE
    float64 [12] device row (include/upflow_hip.h, upf_kitti_score), from pred fp32 [B,2,H,W] and the payload of the two flow
    PNGs, uint16 [B,H,W,3] as flow_io.read_png returns it: two launches on the current stream, no host synchronisation,
    bit-reproducible.  out: a float64 [12] device tensor to write, e.g. row `index` of a [N,12] table; else a new tensor."""
    who = 'kitti_score'
    for name, t, dt in (('pred', pred, torch.float32), ('gt_occ_u16', gt_occ_u16, torch.uint16), ('gt_noc_u16', gt_noc_u16, torch.uint16)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 4:
            raise UpflowHipError('%s: `%s` must be a 4-d %s tensor, got %s' % (who, name, dt, (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t)))
    B, C, H, W = pred.shape
    if C != 2 or min(B, H, W) < 1:
        raise UpflowHipError('%s: pred [B,2,H,W] expected, got %s' % (who, tuple(pred.shape)))
    for name, t in (('gt_occ_u16', gt_occ_u16), ('gt_noc_u16', gt_noc_u16)):
        if tuple(t.shape) != (B, H, W, 3):
            raise UpflowHipError('%s: `%s` must be [%d,%d,%d,3] (R, G, B of the KITTI flow PNG), got %s' % (who, name, B, H, W, tuple(t.shape)))
    dev = _lib.check_gpu(pred, gt_occ_u16, gt_noc_u16, out)
    if out is None:
        out = torch.empty((SCORE_ROW,), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or tuple(out.shape) != (SCORE_ROW,):
        raise UpflowHipError('%s: `out` must be a float64 [%d] tensor, got %s %s' % (who, SCORE_ROW, tuple(out.shape), out.dtype))
    import ctypes
    nbytes = ctypes.c_longlong(0)
    _lib.call('upf_kitti_score_workspace_bytes', B, H, W, ctypes.byref(nbytes))
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    _lib.launch(dev, 'upf_kitti_score', _lib.ptr(pred), _lib.ptr(gt_occ_u16), _lib.ptr(gt_noc_u16), _lib.ptr(ws), _lib.ptr(out), B, H, W)
    return out


# ---- evaluation results: KITTI PNG samples, Middlebury colours, .flo body (csrc/export.hip) ---------------------------------------
_EXPORT_OUT = {'kitti': (torch.uint16, 3), 'color': (torch.uint8, 3), 'flo': (torch.float32, 2)}      # name -> dtype, last dim
_export_ws = {}                                                                                        # (device, stream, B, H, W) -> uint8 tensor


def flow_export_workspace(device, B, H, W):
    """The cached workspace ops.flow_export uses for [B,2,H,W] predictions on `device`: one per device and shape — and per
    current stream, since the calls of one stream use it one after the other and those of two streams would not."""
    import ctypes
    device = torch.device(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, B, H, W)
    ws = _export_ws.get(key)
    if ws is None:
        nbytes = ctypes.c_longlong(0)
        _lib.call('upf_flow_export_workspace_bytes', B, H, W, ctypes.byref(nbytes))
        ws = _export_ws[key] = torch.empty((nbytes.value,), dtype=torch.uint8, device=device)
    return ws


def flow_export(pred, valid=None, kitti=False, color=False, flo=False, max_rad=None, out=None):
    """The payloads of the files an evaluation run saves, from pred fp32 [B,2,H,W] on the device (include/upflow_hip.h,
    upf_flow_export) -> dict of device tensors, one per requested output:
        'kitti'  uint16 [B,H,W,3]   the samples of the KITTI flow PNG (flow_io.write_kitti_png_u16 writes them); B channel = valid
        'color'  uint8  [B,H,W,3]   tools.flow_to_image of every item
        'flo'    fp32   [B,H,W,2]   the body of a .flo file (flow_io.write_flo_payload)
    valid: fp32 [B,1,H,W] or None (1 everywhere).  max_rad: the colour scale in px for every item; None / <= 0: each item's own
    largest radius, as the reference (one more launch).  out: dict of preallocated contiguous tensors to write (slices of larger
    tensors included); its keys count as requested.  One or two launches on the current stream, no host synchronisation."""
    who = 'flow_export'
    if not torch.is_tensor(pred) or pred.dtype != torch.float32 or pred.dim() != 4:
        raise UpflowHipError('%s: `pred` must be a 4-d float32 tensor, got %s' % (who, (tuple(pred.shape), pred.dtype) if torch.is_tensor(pred) else type(pred)))
    B, C, H, W = pred.shape
    if C != 2 or min(B, H, W) < 1:
        raise UpflowHipError('%s: pred [B,2,H,W] expected, got %s' % (who, tuple(pred.shape)))
    if valid is not None and (not torch.is_tensor(valid) or valid.dtype != torch.float32 or tuple(valid.shape) != (B, 1, H, W)):
        raise UpflowHipError('%s: `valid` must be a float32 [%d,1,%d,%d] tensor, got %s' % (who, B, H, W, (tuple(valid.shape), valid.dtype) if torch.is_tensor(valid) else type(valid)))
    out = dict(out) if out else {}
    unknown = set(out) - set(_EXPORT_OUT)
    if unknown:
        raise UpflowHipError('%s: `out` has unknown keys %s (kitti, color, flo)' % (who, sorted(unknown)))
    wanted = [name for name, flag in (('kitti', kitti), ('color', color), ('flo', flo)) if flag or out.get(name) is not None]
    if not wanted:
        raise UpflowHipError('%s: no output requested (kitti, color, flo)' % who)
    dev = _lib.check_gpu(pred, valid, *[out[name] for name in wanted if torch.is_tensor(out.get(name))])
    res = {}
    for name in wanted:
        dt, last = _EXPORT_OUT[name]
        t = out.get(name)
        if t is None:
            t = torch.empty((B, H, W, last), dtype=dt, device=dev)
        elif not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != (B, H, W, last):
            raise UpflowHipError('%s: out[%r] must be a %s [%d,%d,%d,%d] tensor, got %s' % (who, name, dt, B, H, W, last, (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t)))
        res[name] = t
    max_rad = 0.0 if max_rad is None else float(max_rad)
    ws = flow_export_workspace(dev, B, H, W) if 'color' in res and not max_rad > 0.0 else None
    _lib.launch(dev, 'upf_flow_export', _lib.ptr(pred), _lib.ptr(valid), _lib.ptr(res.get('kitti')), _lib.ptr(res.get('color')),
                _lib.ptr(res.get('flo')), max_rad, _lib.ptr(ws), B, H, W)
    return res


# ---- PNG compression: filter, Huffman code, zlib stream (csrc/png.hip) -------------------------------------------------------------
_PNG_DEPTH = {torch.uint8: 8, torch.uint16: 16}
_png_ws = {}                                                  # (device, stream, B, H, W, C, depth) -> (uint8 workspace, cap)


def png_encode_workspace(device, B, H, W, C, depth):
    """(workspace, cap) of ops.png_encode for [B,H,W,C] images of `depth` bits on `device`: cached per device, current stream and
    shape, as flow_export_workspace is; cap is the pitch of the stream slots (include/upflow_hip.h, upf_png_encode)."""
    import ctypes
    device = torch.device(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, B, H, W, C, depth)
    got = _png_ws.get(key)
    if got is None:
        nbytes, cap = ctypes.c_longlong(0), ctypes.c_longlong(0)
        _lib.call('upf_png_encode_workspace_bytes', B, H, W, C, depth, ctypes.byref(nbytes), ctypes.byref(cap))
        got = _png_ws[key] = (torch.empty((nbytes.value,), dtype=torch.uint8, device=device), cap.value)
    return got


def png_encode(img, out=None):
    """The zlib stream of every image's PNG — the body of its IDAT chunk, flow_io.write_png_stream adds the rest of the file — from
    img uint8 / uint16 [B,H,W,C], C in 1..4, on the device: ops.flow_export's 'kitti' and 'color' as they are (include/upflow_hip.h,
    upf_png_encode) -> (streams uint8 [B,cap], lengths int32 [B]); image b's stream is streams[b, :lengths[b]], a negative length
    says that it did not fit (cap rules that out).  out: a contiguous uint8 [B,cap] tensor to write (a slice of a larger one
    included), or a pair of it and an int32 [B] tensor.  Three launches on the current stream, no host synchronisation."""
    who = 'png_encode'
    if not torch.is_tensor(img) or img.dtype not in _PNG_DEPTH or img.dim() != 4:
        raise UpflowHipError('%s: `img` must be a 4-d uint8 / uint16 tensor [B,H,W,C], got %s' % (who, (tuple(img.shape), img.dtype) if torch.is_tensor(img) else type(img)))
    B, H, W, C = img.shape
    if not 1 <= C <= 4 or min(B, H, W) < 1:
        raise UpflowHipError('%s: img [B,H,W,C] with C in 1..4 expected, got %s' % (who, tuple(img.shape)))
    streams, lengths = out if isinstance(out, (tuple, list)) else (out, None)
    dev = _lib.check_gpu(img, streams, lengths)
    depth = _PNG_DEPTH[img.dtype]
    ws, cap = png_encode_workspace(dev, B, H, W, C, depth)
    if streams is None:
        streams = torch.empty((B, cap), dtype=torch.uint8, device=dev)
    elif streams.dtype != torch.uint8 or tuple(streams.shape) != (B, cap):
        raise UpflowHipError('%s: `out` must be a uint8 [%d,%d] tensor, got %s %s' % (who, B, cap, tuple(streams.shape), streams.dtype))
    if lengths is None:
        lengths = torch.empty((B,), dtype=torch.int32, device=dev)
    elif lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,):
        raise UpflowHipError('%s: the lengths must be an int32 [%d] tensor, got %s %s' % (who, B, tuple(lengths.shape), lengths.dtype))
    _lib.launch(dev, 'upf_png_encode', _lib.ptr(img), _lib.ptr(streams), _lib.ptr(lengths), _lib.ptr(ws), B, H, W, C, depth)
    return streams, lengths


# ---- KITTI error maps from the uint16 ground truth (csrc/errmap.hip) ---------------------------------------------------------------
ERROR_DILATE_MAX = 4
_errmap_ws = {}                                               # (device, stream, B, H, W, dilate) -> uint8 tensor, or None (no bytes needed)


def flow_error_image_workspace(device, B, H, W, dilate):
    """The cached workspace ops.flow_error_image uses for [B,2,H,W] predictions on `device`, per device, current stream and shape as
    flow_export_workspace is — or None where upf_flow_error_image_workspace_bytes answers 0 bytes."""
    import ctypes
    device = torch.device(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, B, H, W, dilate)
    if key not in _errmap_ws:
        nbytes = ctypes.c_longlong(0)
        _lib.call('upf_flow_error_image_workspace_bytes', B, H, W, dilate, ctypes.byref(nbytes))
        _errmap_ws[key] = torch.empty((nbytes.value,), dtype=torch.uint8, device=device) if nbytes.value > 0 else None
    return _errmap_ws[key]


def flow_error_image(pred, gt_occ_u16, gt_noc_u16, log_colors=True, dilate=0, out=None):
    """The KITTI devkit's error map of every item (tools.lib_to_show_flow.flow_error_image_np; include/upflow_hip.h,
    upf_flow_error_image) -> uint8 [B,H,W,3] on the device, R, G, B: the payload flow_io.write_png and ops.png_encode take as it
    is.  pred fp32 [B,2,H,W]; gt_occ_u16 / gt_noc_u16: the payload of the two flow PNGs, uint16 [B,H,W,3], as ops.kitti_score takes
    them.  log_colors: the devkit's ten-bin map (occluded pixels at half brightness), else min(error, 5) / 5 as brightness (red
    where occluded); pixels without ground truth are black.  dilate = r in 0..4: every pixel without ground truth takes the colour of
    the last valid pixel (in raster order) within r pixels — KITTI's ground truth is sparse.  out: a contiguous uint8 [B,H,W,3]
    tensor to write (a slice of a larger one included).  One launch on the current stream, no host synchronisation."""
    who = 'flow_error_image'
    for name, t, dt in (('pred', pred, torch.float32), ('gt_occ_u16', gt_occ_u16, torch.uint16), ('gt_noc_u16', gt_noc_u16, torch.uint16)):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 4:
            raise UpflowHipError('%s: `%s` must be a 4-d %s tensor, got %s' % (who, name, dt, (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t)))
    B, C, H, W = pred.shape
    if C != 2 or min(B, H, W) < 1:
        raise UpflowHipError('%s: pred [B,2,H,W] expected, got %s' % (who, tuple(pred.shape)))
    for name, t in (('gt_occ_u16', gt_occ_u16), ('gt_noc_u16', gt_noc_u16)):
        if tuple(t.shape) != (B, H, W, 3):
            raise UpflowHipError('%s: `%s` must be [%d,%d,%d,3] (R, G, B of the KITTI flow PNG), got %s' % (who, name, B, H, W, tuple(t.shape)))
    if isinstance(dilate, bool) or not isinstance(dilate, int) or not 0 <= dilate <= ERROR_DILATE_MAX:
        raise UpflowHipError('%s: `dilate` must be an integer in 0..%d, got %r' % (who, ERROR_DILATE_MAX, dilate))
    dev = _lib.check_gpu(pred, gt_occ_u16, gt_noc_u16, out)
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, 3):
        raise UpflowHipError('%s: `out` must be a uint8 [%d,%d,%d,3] tensor, got %s %s' % (who, B, H, W, tuple(out.shape), out.dtype))
    ws = flow_error_image_workspace(dev, B, H, W, dilate)
    _lib.launch(dev, 'upf_flow_error_image', _lib.ptr(pred), _lib.ptr(gt_occ_u16), _lib.ptr(gt_noc_u16), _lib.ptr(out),
                1 if log_colors else 0, dilate, _lib.ptr(ws), B, H, W)
    return out
