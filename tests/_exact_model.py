"""Exactly representable operands for the 16-bit convolution kernels (csrc/conv3x3.hip, conv_kernel.hpp, conv_c8.hip, conv_pair.hip,
conv_wgrad.hip), their fp64 reference, the guard that makes bit equality a fair demand, and the NaN arena the operands live in.
Shared by tests/test_hip_conv_exact.py (GPU) and tests/test_exact_model_cpu.py (the conditions, no GPU).  Plain torch, no GPU import.
The last section does the same for the cost-volume kernels (csrc/corr81_*.hip; tests/test_hip_corr_exact.py).

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

    def block(self, B, C, H, W, misalign=0, fill=None):
        """A CONTIGUOUS [B,C,H,W] block (what the cost-volume entry points take; `nchw` is contiguous only for B = 1) whose first
        element lies `misalign` elements past a 16-byte boundary; 4 KiB of NaN around it like every block."""
        unit = 16 // self.buf.element_size()
        assert 0 <= misalign < unit
        n = B * C * H * W
        v = self._take(n + misalign, 0, unit)[misalign:].view(B, C, H, W)
        assert v.is_contiguous() and v.data_ptr() % 16 == misalign * self.buf.element_size()
        if fill is not None:
            v.copy_(fill.to(self.dtype))
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


class Arena32(Arena):
    """The same arena in fp32 (the cost volume's parity mode): margins of 2048 elements = 8 KiB, bits compared as int32."""

    def __init__(self, device, elems=1 << 20):
        self.dtype, self.device = torch.float32, torch.device(device)
        self.buf = torch.full((elems,), float('nan'), dtype=torch.float32, device=self.device)
        self.cur = 0

    def snapshot(self):
        return self.buf.view(torch.int32).clone()

    def untouched(self, snap, *written):
        mask = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.device)
        for v in written:
            mask.as_strided(v.size(), v.stride(), v.storage_offset() - self.buf.storage_offset()).fill_(True)
        return bool(((self.buf.view(torch.int32) == snap) | mask).all())


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


# ---- the cost volume (csrc/corr81_fwd.hip with its three kernel headers, corr81_bwd.hip) ---------------------------------------------
# A plain sum of products of two 16-bit tensors, one scale by 1/C (1/(k*k*C) in the general-parameter kernel), one optional
# LeakyReLU.  Shared by tests/test_hip_corr_exact.py (GPU) and tests/test_exact_model_cpu.py.  Grids: (step, largest magnitude) of
# the features 'f' and of grad_out 'g'; grad_out * 0.125 stays representable (bf16: multiples of 1/32 up to 1/4, fp16: of 2^-7), so the
# gradient the autograd function masks with slope 0.125 is exact.  fp32 runs use the same grids.
CORR_GRIDS = {torch.bfloat16: {'f': (0.125, 2.0), 'g': (0.25, 2.0)}, torch.float16: {'f': (2.0 ** -5, 2.0), 'g': (2.0 ** -4, 2.0)}}
CORR_R, CORR_D, CORR_ND = 4, 9, 81

# Shapes (B, C, H, W), sized on the dispatch code (launch_fwd / try_allc / allc_pick in csrc/corr81_fwd.hip, upf_corr81_backward in
# csrc/corr81_bwd.hip): H = 9 / 5 / 6 is no multiple of a tile height (8, 4, 2), W = 40 / 35 crosses the 32- and 16-pixel tiles.
CORR_C = (5, 32, 96, 196, 208)
CORR_ALLC = [(2 if C == 32 else 1, C, 9, W) for W in (40, 35) for C in CORR_C]                # aligned and ragged rows; one B = 2 each
CORR_SMALL = [(1, 5, 6, 20), (1, 32, 5, 13), (2, 5, 5, 4)]
CORR_OLD = [(1, 5, 9, 40), (2, 32, 9, 40), (1, 33, 9, 40), (1, 96, 9, 40), (1, 33, 9, 35), (1, 33, 6, 20)]     # old_path: MFMA single / multi chunk, chunked
CORR_DEEP = [(1, 212, 9, 40), (1, 256, 9, 40), (1, 212, 9, 35), (1, 256, 9, 35)]               # C > 208: nothing all-channels fits
CORR_SHORT = [(1, 5, 5, 1), (2, 33, 5, 3)]                                                   # rows shorter than a staging quad
CORR_BIG = (8, 48, 40, 128)                                                                  # the smallest grid of >= 160 8x32 tiles with C > 40
CORR_F32 = [(2, 32, 9, 40), (1, 5, 9, 35), (1, 196, 6, 20), (1, 33, 5, 13), (1, 5, 5, 1), (1, 212, 5, 8)]
CORR_FWD = list(dict.fromkeys(CORR_ALLC + CORR_SMALL + CORR_OLD + CORR_DEEP + CORR_SHORT + [CORR_BIG] + CORR_F32))
CORR_BWD_ALIGNED = [(1, 5, 17, 68), (2, 33, 6, 12), (1, 8, 6, 12)]                           # W % 4 == 0; 64-pixel and 16-row tiles crossed; C % 4 != 0
CORR_BWD_RAGGED = [(1, 5, 6, 5), (2, 8, 5, 13), (1, 33, 17, 26), (1, 4, 5, 67)]
CORR_BWD_NARROW = [(1, 5, 7, 1), (2, 8, 5, 2), (1, 33, 6, 3)]                                # W < 4: the gather kernel; C = 5, 33: a short last channel block
CORR_BWD = CORR_BWD_ALIGNED + CORR_BWD_RAGGED + CORR_BWD_NARROW
CORR_AUTOGRAD = [(2, 32, 4, 16), (1, 33, 9, 13)]                                             # H = 4: the dy = -4 / +4 channels are exact zeros everywhere
CORR_GENERAL_SHAPE = (2, 6, 20, 28)
CORR_NF_SHAPES = [(1, 32, 9, 40), (1, 33, 9, 35)]
CORR_NF_BWD_SHAPES = [(1, 5, 9, 12), (1, 5, 9, 13), (1, 5, 9, 3)]


def corr_operands(shape, dtype, go_shape=None, salt=0):
    """-> f1, f2, grad_out (fp32 CPU tensors on CORR_GRIDS[dtype], exactly representable in it)."""
    B, C, H, W = shape
    G = CORR_GRIDS[dtype]
    gen = torch.Generator().manual_seed(seed_of('corr', tuple(shape), DTYPE_NAMES[dtype], salt))
    f1, f2 = grid(shape, G['f'][0], G['f'][1], gen), grid(shape, G['f'][0], G['f'][1], gen)
    go = grid((B, CORR_ND, H, W) if go_shape is None else go_shape, G['g'][0], G['g'][1], gen)
    for t in (f1, f2, go, go * SLOPE):
        assert torch.equal(t.to(dtype).float(), t)
    return f1, f2, go


def corr_sums(f1, f2):
    """S[n, 9 (dy + 4) + (dx + 4), y, x] = sum_c f1[n,c,y,x] * f2[n,c,y+dy,x+dx], f2 = 0 outside: fp64, NOT divided by C."""
    B, C, H, W = f1.shape
    a, b = f1.double(), F.pad(f2.double(), (CORR_R,) * 4)
    S = a.new_zeros(B, CORR_ND, H, W)
    for dy in range(CORR_D):
        for dx in range(CORR_D):
            S[:, dy * CORR_D + dx] = (a * b[:, :, dy:dy + H, dx:dx + W]).sum(1)
    return S


def corr_grad_sums(f1, f2, go):
    """G1[n,c,y,x] = sum_d gO[n,d,y,x] * f2[n,c,y+dy,x+dx] (f2 = 0 outside: such a term is gO times that zero — nothing for a
    finite gO, NaN for a non-finite one); G2[n,c,y,x] = sum_d gO[n,d,y-dy,x-dx] * f1[n,c,y-dy,x-dx] over the source pixels that
    exist.  fp64, not divided by C."""
    B, C, H, W = f1.shape
    a, g, bp = f1.double(), go.double(), F.pad(f2.double(), (CORR_R,) * 4)
    G1 = torch.zeros_like(a)
    G2p = a.new_zeros(B, C, H + 2 * CORR_R, W + 2 * CORR_R)
    for dy in range(CORR_D):
        for dx in range(CORR_D):
            w = g[:, dy * CORR_D + dx].unsqueeze(1)
            G1 += w * bp[:, :, dy:dy + H, dx:dx + W]
            G2p[:, :, dy:dy + H, dx:dx + W] += w * a
    return G1, G2p[:, :, CORR_R:CORR_R + H, CORR_R:CORR_R + W]


def corr_general_sums(f1, f2, pad, k, md, s1, s2):
    """oracle/ops.py::correlation_general restated in fp64 without its division by k * k * C: padded inputs, kernel radius
    (k - 1) / 2, displacement radius md / s2, (2 dr + 1)^2 channels of ceil((H + 2 pad - 2 (kr + md)) / s1) rows."""
    B, C, H, W = f1.shape
    kr, dr = (k - 1) // 2, md // s2
    assert md - dr * s2 - kr >= 0, 'the reference reads outside its padded buffer for these parameters'
    oH, oW = -(-(H + 2 * pad - 2 * (kr + md)) // s1), -(-(W + 2 * pad - 2 * (kr + md)) // s1)
    ds = 2 * dr + 1
    p1, p2 = F.pad(f1.double(), (pad,) * 4), F.pad(f2.double(), (pad,) * 4)
    ys, xs = torch.arange(oH) * s1 + md, torch.arange(oW) * s1 + md
    chans = []
    for tj in range(-dr, dr + 1):
        for ti in range(-dr, dr + 1):
            acc = 0
            for j in range(-kr, kr + 1):
                for i in range(-kr, kr + 1):
                    acc = acc + (p1[:, :, ys + j][:, :, :, xs + i] * p2[:, :, ys + tj * s2 + j][:, :, :, xs + ti * s2 + i]).sum(1)
            chans.append(acc)
    return torch.stack(chans, 1)


def corr_general_grad_sums(f1, f2, go, pad, k, md, s1, s2):
    """The gradients of corr_general_sums wrt f1 and f2 (fp64 autograd: sums of products of grid values, exact like the rest)."""
    a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    return torch.autograd.grad(corr_general_sums(a, b, pad, k, md, s1, s2), (a, b), go.double())


def _finite(t):
    return torch.where(torch.isfinite(t), t, torch.zeros_like(t))


def guard_corr(f1, f2, dtype, what='cost volume'):
    st = CORR_GRIDS[dtype]['f'][0]
    a, b = _finite(f1), _finite(f2)
    return guard(what, corr_sums(a.abs(), b.abs()), st * st, (a, st), (b, st))


def guard_corr_grads(f1, f2, go, dtype, step_g, what='cost-volume gradients'):
    st = CORR_GRIDS[dtype]['f'][0]
    g = _finite(go)
    A1, A2 = corr_grad_sums(f1.abs(), f2.abs(), g.abs())
    return guard(what, torch.maximum(A1, A2), st * step_g, (f1, st), (f2, st), (g, step_g))


def guard_corr_general(f1, f2, go, params, dtype, what='general cost volume'):
    st, sg = CORR_GRIDS[dtype]['f'][0], CORR_GRIDS[dtype]['g'][0]
    top = guard(what, corr_general_sums(f1.abs(), f2.abs(), *params), st * st, (f1, st), (f2, st))
    if go is not None:
        A1, A2 = corr_general_grad_sums(f1.abs(), f2.abs(), go.abs(), *params)
        top = max(top, guard(what + ' gradients', torch.maximum(A1, A2), st * sg, (go, sg)))
    return top


def corr_quotients(S64, n):
    """The two fp32 spellings of S / n computed from the exact sum: (fp32(S / n), the IEEE quotient; fp32(S * fp32(1 / n)), the
    product with the correctly rounded fp32 reciprocal).  Equal — and exact — for a power-of-two n.  No double rounding on the way
    through fp64: S is an integer below 2^24 quanta and n < 2^13, so S / n lies at least 2^-38 (relative) from every fp32 rounding
    boundary unless it IS one, far more than fp64's 2^-53; S * fp32(1 / n) has at most 48 significant bits and is exact in fp64."""
    fin = torch.isfinite(S64)
    assert torch.equal(S64[fin].float().double(), S64[fin]), 'the sum is not exact in fp32: a broken test'
    r = (torch.ones((), dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)).double()
    return (S64 / n).float(), (S64 * r).float()


def corr_act32(v32, slope):
    """The kernels' epilogue on the fp32 value, before the one rounding: slope 0 = none; 0.125 exact; 0.1 = slope01_ref's order."""
    if slope == 0.0:
        return v32
    if slope == SLOPE:
        return torch.where(v32 > 0, v32, v32 * SLOPE)
    assert slope == 0.1
    return slope01_ref(v32.double(), torch.float32)


def corr_expected(S64, n, slope, dtype):
    """-> the (two) tensors of `dtype` a correct kernel may give: one RNE of the activated fp32 spelling (fp32: the spelling itself)."""
    return tuple(corr_act32(q, slope).to(dtype) for q in corr_quotients(S64, n))


@functools.lru_cache(maxsize=None)
def corr_case(shape, dtype):
    """-> (f1, f2, grad_out, S fp64) of one forward shape, guarded; computed once and shared (nobody writes to them)."""
    f1, f2, go = corr_operands(shape, dtype)
    guard_corr(f1, f2, dtype)
    return f1, f2, go, corr_sums(f1, f2)


def corr_mask(S64, slope):
    """The factor Corr81Function.backward applies: out > 0 ? 1 : slope — the sign of the 16-bit output is the sign of S (no
    non-zero S / C underflows to zero on these grids), exact zeros take the slope."""
    return torch.where(S64 > 0, torch.ones((), dtype=torch.float64), torch.full((), float(slope), dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def corr_grad_case(shape, dtype, slope=0.0):
    """-> (f1, f2, the gradient the backward kernels see [grad_out, masked if slope], G1 fp64, G2 fp64), guarded."""
    f1, f2, go = corr_operands(shape, dtype)
    sg = CORR_GRIDS[dtype]['g'][0]
    gm = go
    if slope:
        gm, sg = (go.double() * corr_mask(corr_sums(f1, f2), slope)).float(), sg * slope
        assert torch.equal(gm.to(dtype).float(), gm)
    guard_corr_grads(f1, f2, gm, dtype, sg)
    return (f1, f2, gm) + tuple(corr_grad_sums(f1, f2, gm))


@functools.lru_cache(maxsize=None)
def corr_general_case(params, dtype):
    """-> (f1, f2, grad_out or None, S, G1 or None, G2 or None) of one general parameter set at CORR_GENERAL_SHAPE, guarded; the
    gradients where kernel_size 1 and stride1 1 (oracle.ops.correlation_backward_supported)."""
    pad, k, md, s1, s2 = params
    probe = corr_general_sums(torch.zeros(CORR_GENERAL_SHAPE), torch.zeros(CORR_GENERAL_SHAPE), *params)
    f1, f2, go = corr_operands(CORR_GENERAL_SHAPE, dtype, tuple(probe.shape), salt=params)
    S = corr_general_sums(f1, f2, *params)
    if k == 1 and s1 == 1:
        guard_corr_general(f1, f2, go, params, dtype)
        G1, G2 = corr_general_grad_sums(f1, f2, go, *params)
        return f1, f2, go, S, G1, G2
    guard_corr_general(f1, f2, None, params, dtype)
    return f1, f2, None, S, None, None


# non-finite operands: one element each.  Forward kinds: (tensor, value, place); backward: (value, place)
CORR_NF_FWD = [('f2', 'nan', 'in'), ('f2', 'nan', 'corner'), ('f1', 'inf', 'in'), ('f1', 'inf', 'corner')]
CORR_NF_BWD = [(v, p) for v in ('nan', 'inf') for p in ('in', 'edge_out', 'edge_in')]
_NF = {'nan': float('nan'), 'inf': float('inf')}


def corr_nonfinite_fwd(shape, dtype, kind):
    """One NaN in f2 / one +inf in f1 at an interior pixel (n, c, H/2, W/2) or the corner pixel (H-1, W-1, the end of the last row).
    -> (f1, f2, S fp64, how many outputs are non-finite): a NaN at (y0, x0) of f2 reaches exactly the (d, y, x) with y + dy = y0,
    x + dx = x0 — one pixel per displacement whose source exists; an inf in f1 all 81 channels of its pixel (inf * 0 = NaN where f2
    or its zero padding holds a zero: the reference evaluates the same products)."""
    B, C, H, W = shape
    which, val, place = kind
    f1, f2, _ = corr_operands(shape, dtype, salt=('nf',) + tuple(kind))
    n, c, y0, x0 = (B - 1, C // 2, H // 2, W // 2) if place == 'in' else (0, C - 1, H - 1, W - 1)
    (f1 if which == 'f1' else f2)[n, c, y0, x0] = _NF[val]
    guard_corr(f1, f2, dtype)
    if which == 'f1':
        count = CORR_ND
    else:
        count = sum(0 <= y0 - dy < H for dy in range(-4, 5)) * sum(0 <= x0 - dx < W for dx in range(-4, 5))
    return f1, f2, corr_sums(f1, f2), count


def corr_nonfinite_bwd(shape, dtype, kind):
    """One NaN / +inf in grad_out[n, d, y, x]: 'in' an interior pixel, d = (dy, dx) = (1, -2); 'edge_out' pixel (0, W-1) with
    d = (-4, -4), whose f2 pixel and whose g2 target lie outside the image: g1 of that pixel is NaN (gO times the zero f2 holds
    there), g2 is untouched; 'edge_in' pixel (H-1, 0) with d = (-1, 0), inside.  -> (f1, f2, go, G1, G2, non-finite counts of G1, G2):
    C elements of g1 (the pixel, every channel); C of g2 (the target pixel) if it exists."""
    B, C, H, W = shape
    val, place = kind
    f1, f2, go = corr_operands(shape, dtype, salt=('nfb',) + tuple(kind))
    y, x, dy, dx = {'in': (H // 2, W // 2, 1, -2), 'edge_out': (0, W - 1, -4, -4), 'edge_in': (H - 1, 0, -1, 0)}[place]
    go[B - 1, (dy + 4) * CORR_D + dx + 4, y, x] = _NF[val]
    guard_corr_grads(f1, f2, go, dtype, CORR_GRIDS[dtype]['g'][0])
    inside = 0 <= y + dy < H and 0 <= x + dx < W
    return (f1, f2, go) + tuple(corr_grad_sums(f1, f2, go)) + (C, C if inside else 0)
