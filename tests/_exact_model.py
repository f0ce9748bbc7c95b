"""Exactly representable operands for the 16-bit convolution kernels (csrc/conv3x3.hip, conv_kernel.hpp, conv_c8.hip, conv_pair.hip,
conv_wgrad.hip), their fp64 reference, the guard that makes bit equality a fair demand, and the NaN arena the operands live in.
Shared by tests/test_hip_conv_exact.py (GPU) and tests/test_exact_model_cpu.py (the conditions, no GPU).  Plain torch, no GPU import.

The idea: every operand sits on a grid (an integer multiple of a power of two, few significant bits).  Every product is then a
multiple of the QUANTUM (the product of the two grid steps) and so is every partial sum, in any order.  If the sum of the ABSOLUTE
products, in quanta, stays below 2^24, every partial sum of every summation order is an integer below 2^24 times the quantum: exact
in fp32.  fp32 accumulation is then exact whatever the K order, K split, matrix-instruction shape, level order or reduction tree —
the result of a correct kernel is fully determined: ONE round-to-nearest-even of the exact value for a 16-bit output, the exact
value for an fp32 output.  `guard` checks that condition on the operands and the reference alone.

Activation convention (the project's): slope 0 means NO activation (ops.ConvTrainFunction.forward saves y only `if slope != 0.0`;
conv_kernel.hpp epilogue_store: "slope = 1 -> identity", which is what the host passes for 0), any other slope is
y = pre > 0 ? pre : slope * pre.  The exact matrix uses slope 0.125 (a power of two: slope * pre is exact)."""
import functools
import zlib

import torch
import torch.nn.functional as F

LIMIT = float(2 ** 24)
SLOPE = 0.125

# (grid step, largest magnitude) per operand.  bf16 keeps 8 significant bits, fp16 11: the fp16 grids are finer so that its
# outputs still need rounding (tests/test_exact_model_cpu.py checks the share of ties / rounded values for both).
GRIDS = {torch.bfloat16: {'x': (1.0, 3.0), 'w': (0.25, 1.0), 'b': (0.125, 2.0), 'gy': (0.25, 2.0)},
         torch.float16: {'x': (0.25, 2.0), 'w': (2.0 ** -7, 0.5), 'b': (2.0 ** -9, 2.0), 'gy': (0.125, 1.0)}}
DTYPES = (torch.bfloat16, torch.float16)
DTYPE_NAMES = {torch.bfloat16: 'bf16', torch.float16: 'fp16'}


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def grid(shape, step, amax, gen, nonzero=False):
    """Random multiples of `step` in [-amax, amax] (fp32, CPU); nonzero: no exact zeros."""
    n = int(round(amax / step))
    if nonzero:
        k = torch.randint(1, n + 1, shape, generator=gen) * (2 * torch.randint(0, 2, shape, generator=gen) - 1)
    else:
        k = torch.randint(-n, n + 1, shape, generator=gen)
    return (k.double() * step).float()


def out_hw(H, W, s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def geom(k, d, s):
    return dict(stride=s, padding=d * (k - 1) // 2, dilation=d)


class Layer(object):
    """One layer geometry: B, Cin, Cout, H, W, k, d (dilation), s (stride)."""

    def __init__(self, name, B, Cin, Cout, H, W, k=3, d=1, s=1):
        self.name, self.B, self.Cin, self.Cout, self.H, self.W, self.k, self.d, self.s = name, B, Cin, Cout, H, W, k, d, s

    def __repr__(self):
        return self.name

    @property
    def out_hw(self):
        return out_hw(self.H, self.W, self.s)


def operands(layer, dtype, nonzero=False, gy_pow2=0, gy_grid=None, salt=0):
    """-> dict x, w, b, gy (fp32 CPU tensors on the grids of `dtype`: x, w, gy exactly representable in it) and `steps`.
    gy_pow2: gy (and its step) times 2^gy_pow2; gy_grid: another (step, amax) for gy.
    Unless `nonzero`, output channel Cout // 2 has zero weights and a zero bias: its pre-activations are EXACT zeros (the finer the
    grid, the rarer a sum lands on zero by itself), so the mask convention at zero — `y > 0`, zeros take the slope — shapes every
    gradient of the layer."""
    G = GRIDS[dtype]
    gen = torch.Generator().manual_seed(seed_of(layer.name, DTYPE_NAMES[dtype], nonzero, salt))
    ho, wo = layer.out_hw
    gstep, gmax = gy_grid if gy_grid is not None else G['gy']
    o = {'x': grid((layer.B, layer.Cin, layer.H, layer.W), G['x'][0], G['x'][1], gen, nonzero),
         'w': grid((layer.Cout, layer.Cin, layer.k, layer.k), G['w'][0], G['w'][1], gen, nonzero),
         'b': grid((layer.Cout,), G['b'][0], G['b'][1], gen, nonzero),
         'gy': grid((layer.B, layer.Cout, ho, wo), gstep, gmax, gen, nonzero) * 2.0 ** gy_pow2}
    o['steps'] = {'x': G['x'][0], 'w': G['w'][0], 'b': G['b'][0], 'gy': gstep * 2.0 ** gy_pow2}
    if not nonzero:
        o['w'][layer.Cout // 2] = 0
        o['b'][layer.Cout // 2] = 0
    for n in ('x', 'w', 'gy'):
        assert torch.equal(o[n].to(dtype).float(), o[n]), n
    return o


# ---- the fp64 reference -----------------------------------------------------------------------------------------------------
def act(pre, slope):
    return torch.where(pre > 0, pre, slope * pre) if slope else pre


def act_mask(pre, slope):
    """The factor of the activation's gradient: 1 where pre > 0, slope elsewhere (exact zeros and NaN take the slope)."""
    return torch.where(pre > 0, torch.ones((), dtype=pre.dtype), torch.full((), float(slope), dtype=pre.dtype))


def forward_ref(x, w, b, k, d, s, slope=0.0):
    """-> (pre, y) in fp64."""
    pre = F.conv2d(x.double(), w.double(), None if b is None else b.double(), **geom(k, d, s))
    return pre, act(pre, slope)


def layer_ref(x, w, b, gy, k, d, s, slope=0.0):
    """One training layer in fp64, in this order: pre-activation; y; gpre = gy * (pre > 0 ? 1 : slope); data, weight and bias
    gradients.  -> dict pre, y, gpre, gx, gw, gb."""
    pre, y = forward_ref(x, w, b, k, d, s, slope)
    gpre = gy.double() * act_mask(pre, slope) if slope else gy.double()
    return {'pre': pre, 'y': y, 'gpre': gpre, 'gx': torch.nn.grad.conv2d_input(x.shape, w.double(), gpre, **geom(k, d, s)),
            'gw': wgrad_ref([(x, gpre)], w.shape, d, s), 'gb': gpre.sum((0, 2, 3))}


def wgrad_ref(uses, w_shape, d, s=1):
    """fp64 weight gradient over the uses [(x, gpre), ...] of one convolution: the sum over uses."""
    k = w_shape[-1]
    return sum(torch.nn.grad.conv2d_weight(x.double(), w_shape, g.double(), **geom(k, d, s)) for x, g in uses)


# ---- the exactness guard ------------------------------------------------------------------------------------------------------
def on_grid(t, step):
    q = t.double() / step
    f = torch.isfinite(q)
    return bool((q[f] == q[f].round()).all())


def guard(what, abs_sum, quantum, *checks):
    """abs_sum: the contraction evaluated on absolute values (fp64); quantum: the product of the operands' grid steps (the smaller
    one if an addend has its own).  Raises unless every operand in `checks` [(tensor, step)] is on its grid and
    max(abs_sum) / quantum < 2^24.  -> that maximum in quanta.  Takes nothing from the code under test."""
    for t, step in checks:
        assert on_grid(t, step), '%s: an operand is off its grid (step %g)' % (what, step)
    top = float(abs_sum.max()) / quantum if abs_sum.numel() else 0.0
    assert top < LIMIT, '%s: %.3g quanta of absolute products, exactness needs < 2^24 = %.3g' % (what, top, LIMIT)
    return top


def guard_forward(x, w, b, k, d, s, steps, what='forward'):
    a = F.conv2d(x.double().abs(), w.double().abs(), None if b is None else b.double().abs(), **geom(k, d, s))
    q = steps['x'] * steps['w']
    checks = [(x, steps['x']), (w, steps['w'])]
    if b is not None:
        q = min(q, steps['b'])
        checks.append((b, steps['b']))
    return guard(what, a, q, *checks)


def guard_dgrad(gpre, w, x_shape, k, d, s, step_g, step_w, what='data gradient'):
    a = torch.nn.grad.conv2d_input(x_shape, w.double().abs(), gpre.double().abs(), **geom(k, d, s))
    return guard(what, a, step_g * step_w, (gpre, step_g), (w, step_w))


def guard_wgrad(uses, w_shape, d, s, step_x, step_g, what='weight gradient'):
    a = wgrad_ref([(x.abs(), g.abs()) for x, g in uses], w_shape, d, s)
    return guard(what, a, step_x * step_g, *([(x, step_x) for x, _ in uses] + [(g, step_g) for _, g in uses]))


def guard_bias(gpres, step_g, what='bias gradient'):
    a = sum(g.double().abs().sum((0, 2, 3)) for g in gpres)
    return guard(what, a, step_g, *[(g, step_g) for g in gpres])


def guard_layer(o, ref, k, d, s, slope):
    """Every contraction of one training layer (operands `o`, reference `ref` = layer_ref of them).  -> the maxima in quanta."""
    st = o['steps']
    sg = st['gy'] * (slope if slope else 1.0)
    finite = lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))
    x, gpre = finite(o['x']), finite(ref['gpre'])
    return {'y': guard_forward(x, o['w'], o.get('b'), k, d, s, st),
            'gx': guard_dgrad(gpre, o['w'], o['x'].shape, k, d, s, sg, st['w']),
            'gw': guard_wgrad([(x, gpre)], o['w'].shape, d, s, st['x'], sg),
            'gb': guard_bias([gpre], sg)}


# ---- rounding, by bit pattern of the fp32 value ---------------------------------------------------------------------------------
def _dropped_bits(v32, dtype):
    """(bits the 16-bit format drops from the fp32 pattern, their count, elements in the 16-bit format's normal range)."""
    bits = v32.contiguous().view(torch.int32)
    a = v32.abs()
    if dtype == torch.bfloat16:
        return bits & 0xffff, 16, torch.isfinite(v32) & (a >= 2.0 ** -126)
    return bits & 0x1fff, 13, (a >= 2.0 ** -14) & (a < 65520.0)


def is_tie(v32, dtype):
    low, n, normal = _dropped_bits(v32, dtype)
    return normal & (low == (1 << (n - 1)))


def needs_rounding(v32, dtype):
    low, n, normal = _dropped_bits(v32, dtype)
    return normal & (low != 0)


# ---- layouts ----------------------------------------------------------------------------------------------------------------
def to_c8(x):
    """NCHW -> channel octets [B, ceil(C/8), H, W, 8]; the channels that pad the last octet are ZEROS (the layout's contract)."""
    B, C, H, W = x.shape
    n = (C + 7) // 8
    if n * 8 != C:
        x = torch.cat([x, x.new_zeros(B, n * 8 - C, H, W)], 1)
    return x.view(B, n, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def from_c8(x8, C=None):
    B, n, H, W, _ = x8.shape
    x = x8.permute(0, 1, 4, 2, 3).reshape(B, n * 8, H, W)
    return x if C is None else x[:, :C]


# ---- the poison arena -------------------------------------------------------------------------------------------------------
class Arena(object):
    """ONE 16-bit allocation filled with NaN from which operands and outputs are carved: channel slices of NCHW blocks, octet slices
    of C8 blocks, each with `before` / `after` >= 1 foreign planes (octets) around it and >= 4 KiB of NaN before the first and
    after the last byte of every block.  Whatever a kernel reads outside its operands is NaN; whatever it writes outside its
    output shows in `untouched`."""
    MARGIN = 2048                                     # elements = 4 KiB

    def __init__(self, dtype, device, elems=1 << 22):
        assert dtype in DTYPES
        self.dtype, self.device = dtype, torch.device(device)
        self.buf = torch.full((elems,), float('nan'), dtype=dtype, device=self.device)
        self.cur = 0

    def _take(self, n, lead, align):
        """n elements for a block whose view starts `lead` elements in; the view start is a multiple of `align` elements."""
        start = self.cur + self.MARGIN
        start += (-(start + lead)) % align
        assert start + n + self.MARGIN <= self.buf.numel(), 'arena too small'
        self.cur = start + n
        return self.buf[start:start + n]

    def nchw(self, B, C, H, W, before=1, after=1, pitch=None, align=1, fill=None):
        """[B,C,H,W] channel slice of a [B, before + C + after, H, pitch] block (pitch > W: rows with NaN pitch columns)."""
        assert before >= 1 and after >= 1
        p = W if pitch is None else pitch
        planes = before + C + after
        blk = self._take(B * planes * H * p, before * H * p, align).view(B, planes, H, p)
        v = blk[:, before:before + C, :, :W]
        if fill is not None:
            v.copy_(fill.to(self.dtype))
        return v

    def c8(self, B, C, H, W, before=1, after=1, fill=None):
        """[B, ceil(C/8), H, W, 8] octet slice of a [B, before + n + after, H, W, 8] block (16-byte aligned); fill: an NCHW
        tensor of C channels — the channels that pad the last octet become zeros."""
        assert before >= 1 and after >= 1
        n = (C + 7) // 8
        blk = self._take(B * (before + n + after) * H * W * 8, 0, 8).view(B, before + n + after, H, W, 8)
        v = blk[:, before:before + n]
        if fill is not None:
            v.copy_(to_c8(fill.to(self.dtype)))
        return v

    def snapshot(self):
        return self.buf.view(torch.int16).clone()

    def untouched(self, snap, *written):
        """True if the arena equals the snapshot bit for bit (int16 view) everywhere outside the views in `written`."""
        mask = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.device)
        for v in written:
            mask.as_strided(v.size(), v.stride(), v.storage_offset() - self.buf.storage_offset()).fill_(True)
        now = self.buf.view(torch.int16)
        return bool(((now == snap) | mask).all())


# ---- the cases (shared with the CPU conditions) ----------------------------------------------------------------------------------
# Channel geometries that select kernel variants today: Cin 3 / 16 / 33 / 115 / 196 / 243 / 565, Cout 2 / 3 / 32 / 33 / 96 / 128 / 196,
# dilations 1 ... 16, 1x1, stride 2 at even (space-to-depth path) and odd (torch fallback) sizes; widths from {8, 13, 26, 40, 52, 64},
# one case at 64x208 (the 16-row tiles).
TRAIN = [Layer('c565', 2, 565, 128, 8, 26), Layer('c115', 2, 115, 128, 16, 52), Layer('d16', 1, 96, 64, 33, 52, d=16),
         Layer('p196', 2, 196, 32, 4, 13, k=1), Layer('big', 2, 32, 32, 64, 208), Layer('c243', 1, 243, 96, 5, 40),
         Layer('d2', 1, 33, 33, 9, 26, d=2), Layer('d4', 1, 16, 196, 12, 13, d=4), Layer('d8', 1, 115, 96, 17, 40, d=8),
         Layer('n3', 3, 3, 2, 7, 8), Layer('c33_3', 1, 33, 3, 6, 64), Layer('p16', 1, 16, 33, 9, 40, k=1),
         Layer('s2e', 2, 16, 32, 16, 52, s=2), Layer('s2n', 1, 3, 16, 32, 64, s=2), Layer('s2o', 2, 16, 32, 17, 27, s=2)]
TRAIN_BY_NAME = {l.name: l for l in TRAIN}
# the launch matrix (slope, bias, which gradients) runs on these; every other layer runs slope 0.125, bias, all gradients
MATRIX_LAYERS = ('c115', 'd2', 'p196', 's2e', 's2o')
NONFINITE_LAYERS = [Layer('nf_c', 1, 33, 32, 9, 26), Layer('nf_d4', 1, 16, 33, 12, 13, d=4), Layer('nf_p', 2, 196, 32, 4, 13, k=1),
                    Layer('nf_s2', 1, 16, 32, 16, 52, s=2)]
SCALE_LAYERS = ('c115', 'd2', 's2e')
SCALE_K = {torch.bfloat16: (-40, -8, 8), torch.float16: (-6, 4)}
# fp16: a coarser, larger grad_y grid for the scaling cases — the smallest non-zero data gradient is one quantum (gy step * slope *
# w step = 2^-8), which times 2^-6 is still a normal fp16 number; the largest times 2^4 stays below 65504
SCALE_GY = {torch.bfloat16: None, torch.float16: (4.0, 32.0)}
FP16_OVERFLOW = ('c115', 13)                          # (layer, gy_pow2): data gradients beyond 65504 next to finite ones
FP16_SUBNORMAL = ('c33_3', (8 * 2.0 ** -24, 1016 * 2.0 ** -24))       # (layer, gy grid): multiples of 2^-21 below 2^-14; times the slope: of 2^-24

# multi-use weight gradients: conv (Cin, Cout, k, d) x levels [(B, H, W)]; 7 uses = two launches; aligned and ragged widths mixed
WG_CONVS = {'w115': (115, 128, 3, 1), 'w196p': (196, 32, 1, 1), 'w96d8': (96, 64, 3, 8), 'w16n': (16, 32, 3, 1), 'w3n': (3, 16, 3, 1),
            'w33': (33, 3, 3, 2)}
WG_LEVELS = {1: [(2, 8, 26)], 2: [(2, 16, 40), (1, 9, 13)], 6: [(1, 4, 13), (2, 8, 26), (1, 16, 52), (1, 8, 64), (3, 5, 8), (1, 12, 40)],
             7: [(1, 4, 13), (2, 8, 26), (1, 16, 52), (1, 8, 64), (3, 5, 8), (1, 12, 40), (2, 33, 13)]}
WG_CASES = [('w115', 1), ('w115', 2), ('w115', 6), ('w115', 7), ('w196p', 6), ('w96d8', 7), ('w16n', 2), ('w16n', 6), ('w3n', 7), ('w33', 6)]


def wgrad_operands(conv, nuses, dtype):
    """-> ([(x, gpre)] fp32 CPU, steps) for WG_CASES."""
    Cin, Cout, k, d = WG_CONVS[conv]
    G = GRIDS[dtype]
    gen = torch.Generator().manual_seed(seed_of(conv, nuses, DTYPE_NAMES[dtype]))
    uses = [(grid((B, Cin, H, W), G['x'][0], G['x'][1], gen), grid((B, Cout, H, W), G['gy'][0], G['gy'][1], gen)) for B, H, W in WG_LEVELS[nuses]]
    return uses, {'x': G['x'][0], 'gy': G['gy'][0]}


# inference forward through conv3x3_forward_raw: (layer, slope); one 0.1 case (not exactly representable: see slope01_ref)
FWD = [Layer('f115', 2, 115, 128, 6, 26), Layer('f565', 1, 565, 96, 8, 13), Layer('f243', 1, 243, 2, 12, 40), Layer('f16', 1, 16, 196, 9, 64),
       Layer('f33d2', 1, 33, 33, 24, 52, d=2), Layer('f96d16', 1, 96, 64, 33, 40, d=16), Layer('f128d8', 1, 196, 96, 17, 26, d=8),
       Layer('f32d4', 1, 32, 32, 13, 40, d=4), Layer('fbig', 1, 32, 32, 64, 208), Layer('f3s2', 2, 3, 16, 32, 64, s=2),
       Layer('f33s2', 1, 33, 128, 13, 26, s=2), Layer('f196p', 2, 196, 32, 4, 13, k=1), Layer('f16p', 1, 16, 3, 7, 40, k=1)]
FWD_BY_NAME = {l.name: l for l in FWD}


def slope01_ref(pre64, dtype):
    """The one slope-0.1 case per kernel family.  conv_kernel.hpp epilogue_store applies the activation to the fp32 accumulator
    BEFORE the 16-bit conversion (`v0 = fmaxf(v0, v0 * slope)`): the exact fp32 pre-activation, times float32(0.1) in fp32 where it
    is not positive, then one RNE to the dtype."""
    pre32 = pre64.float()
    assert torch.equal(pre32.double(), pre64)
    return torch.maximum(pre32, pre32 * torch.tensor(0.1, dtype=torch.float32)).to(dtype)


# octet-layout forward (conv_c8_forward_raw): name -> (B, octet channels, NCHW tail channels, Cout, H, W, d, y is octets)
C8 = {'o32t83': (1, 32, 83, 128, 8, 16, 1, True), 'o40t7': (2, 40, 7, 33, 7, 8, 1, True), 'o184': (1, 184, 0, 3, 9, 16, 1, False),
      'o64': (1, 64, 0, 32, 9, 24, 1, True), 'o60': (1, 60, 0, 32, 5, 13, 1, False), 'o128d2': (1, 128, 0, 96, 12, 16, 2, True),
      'o96d16': (1, 96, 0, 64, 33, 40, 16, True), 'o480t83': (1, 480, 83, 2, 8, 16, 1, False)}
C8_NARROW = {'n184_3': (1, 184, 3, 17, 40, False), 'n60_16': (2, 60, 16, 9, 13, True), 'n32_2': (2, 32, 2, 33, 8, False), 'n72_5': (1, 72, 5, 16, 64, True)}
# conv_pair_forward_raw: (B, Cin, C1, C2, H, W, strides, y is octets); first-layer weights on a coarse, small grid so that the
# second layer's REAL input (the 16-bit rounding of the first layer's output) keeps the guard
PAIR = {'p3_16_32': (2, 3, 16, 32, 16, 40, (1, 2), True), 'p3_16_32n': (1, 3, 16, 32, 13, 26, (1, 2), False), 'p16_32_32': (1, 16, 32, 32, 12, 64, (2, 1), False),
        'p8_16_3': (1, 8, 16, 3, 9, 40, (2, 1), False)}
PAIR_WA = (0.25, 0.5)
PAIR_BA = (0.125, 2.0)                                # (a fine first bias would make the second layer's quantum too small for fp16)


def layer_of_c8(name):
    B, C8c, C2, Cout, H, W, d, _ = C8[name]
    return Layer(name, B, C8c + C2, Cout, H, W, d=d)


def layer_of_narrow(name):
    B, Cin, Cout, H, W, _ = C8_NARROW[name]
    return Layer(name, B, Cin, Cout, H, W)


def pair_operands(name, dtype):
    """-> x, wa, ba, wb, bb (fp32 CPU, on grids), steps."""
    B, Cin, C1, C2, H, W, strides, _ = PAIR[name]
    G = GRIDS[dtype]
    gen = torch.Generator().manual_seed(seed_of(name, DTYPE_NAMES[dtype]))
    o = {'x': grid((B, Cin, H, W), G['x'][0], G['x'][1], gen), 'wa': grid((C1, Cin, 3, 3), PAIR_WA[0], PAIR_WA[1], gen),
         'ba': grid((C1,), PAIR_BA[0], PAIR_BA[1], gen), 'wb': grid((C2, C1, 3, 3), G['w'][0], G['w'][1], gen), 'bb': grid((C2,), G['b'][0], G['b'][1], gen)}
    o['steps'] = {'x': G['x'][0], 'wa': PAIR_WA[0], 'ba': PAIR_BA[0], 'wb': G['w'][0], 'bb': G['b'][0]}
    return o


def pair_ref(o, strides, slope_a, slope_b, dtype):
    """The two-layer composition: the intermediate layer ROUNDED to the 16-bit dtype (what two launches would store).
    -> (mid [dtype, as fp32], its grid step, second pre-activation fp64, y fp64); guards both layers."""
    st = o['steps']
    guard_forward(o['x'], o['wa'], o['ba'], 3, 1, strides[0], {'x': st['x'], 'w': st['wa'], 'b': st['ba']}, 'pair: first layer')
    pre_a, ya = forward_ref(o['x'], o['wa'], o['ba'], 3, 1, strides[0], slope_a)
    mid = ya.to(dtype).float()
    # the rounded intermediate is still a multiple of the first layer's quantum (times the slope): rounding only drops low bits
    step_mid = min(st['x'] * st['wa'], st['ba']) * (slope_a if slope_a else 1.0)
    guard_forward(mid, o['wb'], o['bb'], 3, 1, strides[1], {'x': step_mid, 'w': st['wb'], 'b': st['bb']}, 'pair: second layer')
    pre_b, yb = forward_ref(mid, o['wb'], o['bb'], 3, 1, strides[1], slope_b)
    return mid, step_mid, pre_b, yb


ALL_LAYERS = dict([(l.name, l) for l in TRAIN + NONFINITE_LAYERS + FWD] + [(n, layer_of_c8(n)) for n in C8] + [(n, layer_of_narrow(n)) for n in C8_NARROW])


@functools.lru_cache(maxsize=None)
def train_case(name, dtype, slope=SLOPE, bias=True, nonzero=False, gy_pow2=0, gy_grid=None):
    """Operands, fp64 reference and guard of one training layer, computed once and shared (nobody writes to them).
    -> (layer, operands, reference, guard maxima)."""
    layer = ALL_LAYERS[name]
    o = operands(layer, dtype, nonzero, gy_pow2, gy_grid)
    if not bias:
        o['b'] = None
    ref = layer_ref(o['x'], o['w'], o['b'], o['gy'], layer.k, layer.d, layer.s, slope)
    return layer, o, ref, guard_layer(o, ref, layer.k, layer.d, layer.s, slope)


@functools.lru_cache(maxsize=None)
def forward_case(name, dtype, slope=SLOPE):
    """-> (layer, operands, pre fp64, y fp64) of one inference layer, guarded."""
    layer = ALL_LAYERS[name]
    o = operands(layer, dtype)
    guard_forward(o['x'], o['w'], o['b'], layer.k, layer.d, layer.s, o['steps'])
    pre, y = forward_ref(o['x'], o['w'], o['b'], layer.k, layer.d, layer.s, slope)
    return layer, o, pre, y


# ---- the smaller families: gated data-gradient epilogue, act_grad, merged narrow tail, 1x1 -> octets ---------------------------------
GATED = [Layer('g2', 2, 2, 32, 16, 64), Layer('g34', 2, 34, 64, 9, 32), Layer('g130', 2, 130, 96, 16, 52), Layer('g226', 2, 226, 64, 8, 13),
         Layer('g450', 1, 450, 128, 4, 13), Layer('g7', 1, 7, 3, 9, 40), Layer('g40', 1, 40, 32, 33, 64)]
ACT_SHAPES = [(2, 32, 16, 52), (1, 7, 5, 9), (3, 2, 4, 13), (1, 33, 9, 64)]
TAIL = [(1, 64, 16, 3, 9, 24), (2, 40, 16, 8, 17, 13), (1, 96, 96, 2, 8, 64)]       # B, Cin, C main, C later, H, W
DUAL = [(2, 196, 32, 4, 13), (1, 33, 20, 9, 40), (1, 16, 8, 33, 64)]                # B, Cin, Cout, H, W
SHARED_LEVELS = [(2, 4, 13), (1, 8, 26), (2, 16, 52)]                               # one 33 -> 32 convolution at three levels


def gated_case(layer, dtype):
    """-> operands of the layer, add, act (a fifth of the gate's values exact zeros), the convolution in fp64 (guarded)."""
    o = operands(layer, dtype)
    G = GRIDS[dtype]
    gen = torch.Generator().manual_seed(seed_of('gate', layer.name, DTYPE_NAMES[dtype]))
    shape = (layer.B, layer.Cout, layer.H, layer.W)
    add, actv = grid(shape, G['gy'][0], G['gy'][1], gen), grid(shape, 1.0, 2.0, gen)
    guard_forward(o['x'], o['w'], o['b'], 3, 1, 1, o['steps'])
    return o, add, actv, forward_ref(o['x'], o['w'], o['b'], 3, 1, 1)[0]


def act_case(shape, dtype):
    """-> src, add, y (a fifth exact zeros) for ops.act_grad; guards the bias sums of all four (add, y) combinations times 9."""
    G = GRIDS[dtype]
    gen = torch.Generator().manual_seed(seed_of('act', shape, DTYPE_NAMES[dtype]))
    src, add = (grid(shape, G['gy'][0], G['gy'][1], gen) for _ in range(2))
    yv = grid(shape, 1.0, 2.0, gen)
    assert int((yv == 0).sum()) >= 20
    assert 9 * guard_bias([src.double().abs() + add.double().abs()], G['gy'][0] * SLOPE) < LIMIT
    return src, add, yv


def bias_parts_case(shape, dtype, n=9):
    """-> n DIFFERENT gradient tensors for the bias reductions (a finish that mis-indexes its partial buffers gives another sum);
    their total bias sum guarded."""
    G = GRIDS[dtype]
    gen = torch.Generator().manual_seed(seed_of('parts', shape, DTYPE_NAMES[dtype]))
    ts = [grid(shape, G['gy'][0], G['gy'][1], gen) for _ in range(n)]
    guard_bias(ts, G['gy'][0])
    return ts


def tail_case(geom, dtype):
    """The merged narrow tail of a dense stack: a main layer (Cin -> Cm) and a later layer that reads [main's output | main's
    input] (Cm + Cin -> Cj), both 3x3 with the activation.  -> dict x, wm, bm, wj, bj, ym (fp64), yj (fp64): yj from the main
    layer's output ROUNDED to the dtype (what the finishing launch reads); both layers guarded.  The main layer's weights and
    bias and the later layer's weights sit on coarse grids so that the second quantum stays large enough for fp16."""
    B, Cin, Cm, Cj, H, W = geom
    G = GRIDS[dtype]
    gen = torch.Generator().manual_seed(seed_of('tail', geom, DTYPE_NAMES[dtype]))
    c = {'x': grid((B, Cin, H, W), G['x'][0], G['x'][1], gen), 'wm': grid((Cm, Cin, 3, 3), PAIR_WA[0], PAIR_WA[1], gen), 'bm': grid((Cm,), PAIR_BA[0], PAIR_BA[1], gen),
         'wj': grid((Cj, Cm + Cin, 3, 3), PAIR_WA[0], PAIR_WA[1], gen), 'bj': grid((Cj,), G['b'][0], G['b'][1], gen)}
    st_m = {'x': G['x'][0], 'w': PAIR_WA[0], 'b': PAIR_BA[0]}
    guard_forward(c['x'], c['wm'], c['bm'], 3, 1, 1, st_m, 'tail: main layer')
    c['ym'] = forward_ref(c['x'], c['wm'], c['bm'], 3, 1, 1, SLOPE)[1]
    mid = c['ym'].to(dtype).float()
    step_mid = min(st_m['x'] * st_m['w'], st_m['b']) * SLOPE
    xin = torch.cat([mid, c['x']], 1)
    guard_forward(xin, c['wj'], c['bj'], 3, 1, 1, {'x': min(step_mid, G['x'][0]), 'w': PAIR_WA[0], 'b': G['b'][0]}, 'tail: later layer')
    c['prej'], c['yj'] = forward_ref(xin, c['wj'], c['bj'], 3, 1, 1, SLOPE)
    c['prem'] = forward_ref(c['x'], c['wm'], c['bm'], 3, 1, 1)[0]
    return c


def dual_case(geom, dtype):
    """-> (layer, operands, y fp64) of a 1x1 projection, guarded."""
    layer = Layer('dual%d' % geom[1], *geom, k=1)
    o = operands(layer, dtype)
    guard_forward(o['x'], o['w'], o['b'], 1, 1, 1, o['steps'])
    return layer, o, forward_ref(o['x'], o['w'], o['b'], 1, 1, 1, SLOPE)[1]


def shared_case(dtype):
    """One convolution (33 -> 32, 3x3) at SHARED_LEVELS: -> (levels, per-level operands with the SAME w and b, per-level references);
    every contraction guarded, the weight and bias gradients over the sum of the uses."""
    levels = [Layer('sh%d' % i, B, 33, 32, H, W) for i, (B, H, W) in enumerate(SHARED_LEVELS)]
    os_ = [operands(l, dtype) for l in levels]
    refs = []
    for o in os_:
        o['w'], o['b'] = os_[0]['w'], os_[0]['b']
        r = layer_ref(o['x'], o['w'], o['b'], o['gy'], 3, 1, 1, SLOPE)
        guard_forward(o['x'], o['w'], o['b'], 3, 1, 1, o['steps'])
        guard_dgrad(r['gpre'], o['w'], o['x'].shape, 3, 1, 1, o['steps']['gy'] * SLOPE, o['steps']['w'])
        refs.append(r)
    st = os_[0]['steps']
    guard_wgrad([(o['x'], r['gpre']) for o, r in zip(os_, refs)], os_[0]['w'].shape, 1, 1, st['x'], st['gy'] * SLOPE)
    guard_bias([r['gpre'] for r in refs], st['gy'] * SLOPE)
    return levels, os_, refs
