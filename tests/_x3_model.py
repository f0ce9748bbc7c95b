"""A plain-torch model of what the split-precision training kernels (csrc/conv_x3_bwd.hip) REPRESENT, and the input generators
that tests/test_hip_conv_x3_bwd_ops.py (GPU) and tests/test_x3_train_cpu.py (the model, no GPU) share.

The model: operands a = hi + lo with hi = fp16(a), lo = fp16(a - hi); the lo * lo product dropped; the three remaining products
summed in fp64 (F.conv2d / torch.nn.grad on the halves); the per-tensor power of two of x3_scale_of (conv_x3_common.hpp) from the
fp32 bit pattern of the maximum, and exact per-level un-scaling.  It has NO accumulation rounding: it is the best any correct
kernel of this design can do, so a bound the model alone breaks is a wrong bound (or a wrong input), not a kernel bug."""
import struct

import torch
import torch.nn.functional as F

BAR_ABS, BAR_REL = 3.0e-6, 2.5            # the project's fp32-class bar: err <= max(3.0e-6, 2.5 * err32)  (test_hip_conv_x3_train.py)


def bar(err32):
    return max(BAR_ABS, BAR_REL * err32)


def rel(got, want):
    return float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1e-300)


# ---- the model ----------------------------------------------------------------------------------------------------------
def scale_of(absmax):
    """x3_scale_of: the power of two that puts `absmax` (a non-negative fp32 value) into [2^13, 2^14); 1 for zero, inf, NaN (and
    anything above 3.0e38); the exponent of the scale clamped to +-100; a subnormal maximum counts as exponent -127."""
    bits = struct.unpack('<I', struct.pack('<f', float(absmax)))[0]
    m = struct.unpack('<f', struct.pack('<I', bits))[0]
    if not (m > 0.0) or m > struct.unpack('<f', struct.pack('<f', 3.0e38))[0]:     # (the kernel compares with 3.0e38f)
        return 1.0
    e = ((bits >> 23) & 0xff) - 127
    return 2.0 ** max(-100, min(100, 13 - e))


def split(v):
    """fp32 tensor -> (hi, lo) as fp64 tensors holding fp16 values."""
    v = v.float()
    hi = v.half().float()
    lo = (v - hi).half().float()
    return hi.double(), lo.double()


def act_grad(gy, mask=None, slope=0.0):
    """upf_act_grad_x3: (grad_pre [fp32], scaled copy gs [fp32], 2^s).  mask: bool tensor `y > 0` (None: no activation).  NaN
    elements do not define the scale."""
    gpre = gy.float() if mask is None else gy.float() * torch.where(mask, torch.ones((), dtype=torch.float32, device=gy.device),
                                                                    torch.full((), float(slope), dtype=torch.float32, device=gy.device))
    a = gpre.abs()
    a = torch.where(a == a, a, torch.zeros_like(a))
    sc = scale_of(float(a.max())) if a.numel() else 1.0
    return gpre, gpre * sc, sc


def _geom(k, d, s):
    return dict(stride=s, padding=d * (k - 1) // 2, dilation=d)


def wgrad(levels, w_shape, d, s, scaled=True):
    """upf_conv_x3_wgrad over levels [(x, grad_pre), ...]: (grad_w, grad_b) in fp64.  scaled = False: the NULL-slot mode, grad_pre is
    split as it is."""
    k = w_shape[-1]
    gw = torch.zeros(w_shape, dtype=torch.float64, device=levels[0][0].device)
    gb = torch.zeros(w_shape[0], dtype=torch.float64, device=gw.device)
    for x, gpre in levels:
        _, gs, sc = act_grad(gpre) if scaled else (None, gpre.float(), 1.0)
        ah, al = split(gs)
        bh, bl = split(x)
        part = sum(torch.nn.grad.conv2d_weight(b, w_shape, a, **_geom(k, d, s)) for a, b in ((ah, bh), (al, bh), (ah, bl)))
        gw += part / sc
        gb += gs.double().sum((0, 2, 3)) / sc
    return gw, gb


def dgrad(gpre, w, x_shape, d, s):
    """upf_conv_x3_dgrad in fp64: stride 1 = the split convolution of gs with the packed (scaled, split) weights; stride 2 = the plain
    fp32-operand kernel (no split)."""
    k = w.shape[-1]
    _, gs, sc = act_grad(gpre)
    if s == 2:
        return torch.nn.grad.conv2d_input(x_shape, w.double(), gs.double(), **_geom(k, d, s)) / sc
    scw = scale_of(float(w.abs().max()))
    wh, wl = split(w.float() * scw)
    gh, gl = split(gs)
    tot = sum(torch.nn.grad.conv2d_input(x_shape, a, b, **_geom(k, d, s)) for a, b in ((wh, gh), (wl, gh), (wh, gl)))
    return tot / scw / sc


def truth(x, w, gpre, d, s):
    """fp64 gradients (gx, gw, gb) of the linear convolution of the same fp32 operands."""
    k = w.shape[-1]
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(x64, w64, None, **_geom(k, d, s)).backward(gpre.double())
    return x64.grad, w64.grad, gpre.double().sum((0, 2, 3))


def torch32(x, w, gpre, d, s):
    """torch's own fp32 gradient kernels on the same operands: the error to compare against."""
    k = w.shape[-1]
    return (torch.nn.grad.conv2d_input(x.shape, w, gpre, **_geom(k, d, s)), torch.nn.grad.conv2d_weight(x, w.shape, gpre, **_geom(k, d, s)),
            gpre.sum((0, 2, 3)))


def out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


# ---- A1: the multi-level weight gradient ---------------------------------------------------------------------------------
A1_CONVS = {'c115': (115, 128, 3, 1, 1), 'c35': (35, 2, 3, 1, 1), 'p196': (196, 32, 1, 1, 1), 's2': (16, 32, 3, 1, 2), 'd4': (96, 64, 3, 4, 1),
            'c5': (5, 3, 3, 1, 1)}
# (B, H, W) per level.  K chunks of 32 pixels; the plan gives every slice cps = max(4, ceil(all chunks / 256)) chunks:
#   pyramid  stride 1: 1, 4, 13, 52, 208 chunks (cps 4: 13 is no multiple; the 2x7 level has fewer chunks than cps)
#   pixels   one chunk each, one valid pixel in it
#   six      unequal B, six levels
#   big      stride 1: 832, 312, 17 chunks -> cps 5, no level a multiple of it
#   odd_s2   odd sizes (for stride 2: 7x14 and 3x4 outputs)
A1_LEVELS = {'pyramid': [(2, 2, 7), (2, 4, 13), (2, 8, 26), (2, 16, 52), (2, 32, 104)],
             'pixels': [(1, 1, 1)] * 3,
             'six': [(1, 3, 5), (3, 2, 9), (2, 7, 11), (1, 16, 33), (4, 1, 3), (2, 9, 4)],
             'big': [(2, 64, 208), (3, 32, 104), (1, 17, 31)],
             'odd_s2': [(1, 13, 27), (2, 5, 7)]}
A1_CASES = [('c115', 'pyramid'), ('c115', 'pixels'), ('c35', 'six'), ('c35', 'pyramid'), ('p196', 'pyramid'), ('p196', 'six'),
            ('s2', 'odd_s2'), ('s2', 'big'), ('s2', 'pyramid'), ('d4', 'pyramid'), ('d4', 'pixels'), ('c5', 'big'), ('c5', 'six'),
            ('c5', 'odd_s2')]
A1_SLOPE = 0.1


def a1_inputs(conv, levels):
    """-> [(x, gy, y or None)] at unit magnitude (CPU fp32).  Odd levels have an activation (slope A1_SLOPE, y gives the mask)."""
    Cin, Cout, k, d, s = A1_CONVS[conv]
    g = torch.Generator().manual_seed(1000 + 7 * sorted(A1_CONVS).index(conv) + sorted(A1_LEVELS).index(levels))
    out = []
    for l, (B, H, W) in enumerate(A1_LEVELS[levels]):
        ho, wo = out_hw(H, W, s)
        x = torch.randn(B, Cin, H, W, generator=g)
        gy = torch.randn(B, Cout, ho, wo, generator=g)
        y = torch.randn(B, Cout, ho, wo, generator=g) if l % 2 else None
        out.append((x, gy, y))
    return out


def a1_magnitudes(nlevels, rot):
    """Level l's grad_y is multiplied by 2^(-7 * ((l - rot) mod nlevels)): every level is the dominant one in one rotation, so a
    reduction that un-scales ANY level with another level's slot is off by a power of 2^7 in a result that level dominates."""
    return [2.0 ** (-7 * ((l - rot) % nlevels)) for l in range(nlevels)]


def a1_grad_pre(gy, y, mag):
    g = gy * mag
    return g if y is None else g * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, A1_SLOPE))


# ---- A4: activation magnitude in the weight gradient ---------------------------------------------------------------------
A4_MAGS = (1e-4, 1e-2, 30.0, 3000.0)
A4_SLOPE = 0.1


def a4_inputs(mag, s):
    """Layer (2, 64, 48, 16, 40), k = 3: x = x0 * mag and b = b0 * mag for FIXED x0, b0: the sign pattern of the pre-activation is
    that of conv(x0) + b0 up to rounding.  -> x, w, b, gy."""
    g = torch.Generator().manual_seed(7 + s)
    x0 = torch.randn(2, 64, 16, 40, generator=g)
    w = torch.randn(48, 64, 3, 3, generator=g) * 0.05
    b0 = torch.randn(48, generator=g)
    ho, wo = out_hw(16, 40, s)
    gy = torch.randn(2, 48, ho, wo, generator=g)
    return x0 * mag, w, b0 * mag, gy


def a4_floor(gpre):
    """Every activation off by the subnormal half-spacing 2^-25, same sign (the form of test_conv_x3_operand_magnitudes' floor)."""
    return 2.0 ** -25 * float(gpre.double().abs().sum((0, 2, 3)).max())


# ---- A5: dynamic range inside grad_y ---------------------------------------------------------------------------------------
A5_LAYERS = [(2, 32, 32, 24, 40, 3, 1, 1), (2, 16, 32, 32, 64, 3, 1, 2)]
A5_R = (8, 14, 18, 24, 32)
A5_VARIANTS = ('right_half', 'sample1', 'upper_channels')
A5_SLOPE = 0.1


def a5_inputs(layer, variant, r):
    """-> x, w, b, gy with one part of gy multiplied by 2^-r."""
    B, Cin, Cout, H, W, k, d, s = layer
    g = torch.Generator().manual_seed(sum(layer))
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5
    b = torch.randn(Cout, generator=g)
    ho, wo = out_hw(H, W, s)
    gy = torch.randn(B, Cout, ho, wo, generator=g)
    f = 2.0 ** -r
    if variant == 'right_half':
        gy[:, :, :, wo // 2:] *= f
    elif variant == 'sample1':
        gy[1] *= f
    else:
        gy[:, Cout // 2:] *= f
    return x, w, b, gy


def a5_gx_part(layer, variant):
    """The slice of gx that only attenuated gradient elements reach: for the right half, the columns more than one kernel radius
    (in input pixels) right of the seam."""
    B, Cin, Cout, H, W, k, d, s = layer
    if variant == 'right_half':
        wo = out_hw(H, W, s)[1]
        return (slice(None), slice(None), slice(None), slice(s * (wo // 2) + 2, None))
    if variant == 'sample1':
        return (slice(1, 2),)
    return None


def a5_floors(x, w, gpre):
    """Elements of gs below 2^-3 (max |gs| in [2^13, 2^14)) carry up to 2^-25 of absolute error: 2^-38 of max |grad_pre|.
    -> (floor of gx at stride 1, floor of grad_w rows)."""
    m = float(gpre.abs().max())
    return (2.0 ** -38 * m * float(w.double().abs().sum((0, 2, 3)).max()), 2.0 ** -38 * m * float(x.double().abs().sum((0, 2, 3)).max()))


def a5_check(name, got, ref32, want, floor, r, label=''):
    """Part-wise bound of A5: |got - want|max <= max(bar * max |want|, floor), the floor only beyond r = 14.  Prints ours beside
    torch fp32 (ref32 may be None: the model's tests)."""
    top = max(float(want.abs().max()), 1e-300)
    err = float((got.double() - want).abs().max())
    err32 = float((ref32.double() - want).abs().max()) / top if ref32 is not None else 0.0
    print('%s r=%d %s: err %.2e of the part\'s max (torch fp32: %.2e), floor %.2e of it' % (label, r, name, err / top, err32, floor / top))
    bound = bar(err32) * top
    if r > 14:
        bound = max(bound, floor)
    assert err <= bound, (label, name, r, err / top, err32, floor / top)
    return err / top, err32
