"""The gradient operators of the fp32 training mode on the matrix cores (csrc/conv_x3_bwd.hip: upf_act_grad_x3, upf_conv_x3_dgrad,
upf_conv_x3_wgrad; ops.ConvX3TrainFunction) on the paths and ranges tests/test_hip_conv_x3_train.py does not reach: the multi-level
weight gradient, un-scaled uses, every argument combination of the autograd node, activations far from O(1), gradients that span
many octaves inside one tensor, zeros, non-finite values and the ends of the exponent range.

Yardstick = test_hip_conv_x3_train.py's: fp64 gradients of the SAME fp32 operands are the truth (the LeakyReLU mask taken from the
layer's own forward output), torch's fp32 gradient kernels on those operands give err32, the bar is err <= max(3.0e-6, 2.5 * err32).
The analytic floors come with tests/_x3_model.py, whose model of the split passes the same bounds on the same inputs without a GPU
(tests/test_x3_train_cpu.py)."""
import types

import pytest
import torch

import _x3_model as M
from test_hip_conv_x3_train import _flat_view, _grads, _rel

pytestmark = pytest.mark.gpu


def _mask_of(y, slope):
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))


def _check(label, got, ref32, want):
    """The project's bar; prints ours beside torch fp32."""
    assert got.shape == want.shape and got.dtype == torch.float32
    err, err32 = _rel(got, want), _rel(ref32, want)
    print('%s: max err %.2e of max |.| (torch fp32: %.2e)' % (label, err, err32))
    assert err <= M.bar(err32), (label, err, err32)
    return err, err32


def _train(x, w, b, gy, d, s, slope, x_grad=True, w_grad=True, b_grad=True):
    """(y, gx, gw, gb) of ops.conv_x3_train on plain tensors; a gradient that was not asked for is None."""
    from upflow_pytorch_amd import ops
    xl, wl = x.clone().requires_grad_(x_grad), w.clone().requires_grad_(w_grad)
    bl = b.clone().requires_grad_(b_grad) if b is not None else None
    y = ops.conv_x3_train(xl, wl, bl, d, slope, s)
    y.backward(gy)
    return y.detach(), xl.grad, wl.grad, bl.grad if bl is not None else None


# ---- A1: the multi-level weight gradient ----------------------------------------------------------------------------------
_A1_REF = {}


def _a1_reference(conv, levels):
    """Per level, at unit magnitude, on the GPU: x, grad_y, y, and the fp64 / torch-fp32 weight and bias gradients.  A level's
    magnitude is a power of two, so its gradients at that magnitude are these times it, exactly.  Computed once, never changed."""
    if (conv, levels) not in _A1_REF:
        Cin, Cout, k, d, s = M.A1_CONVS[conv]
        shape, geom = (Cout, Cin, k, k), dict(stride=s, padding=d * (k - 1) // 2, dilation=d)
        ref = []
        for x, gy, y in M.a1_inputs(conv, levels):
            x, gy, y = x.cuda(), gy.cuda(), (y.cuda() if y is not None else None)
            gpre = M.a1_grad_pre(gy, y, 1.0)
            ref.append(dict(x=x, gy=gy, y=y, gw64=torch.nn.grad.conv2d_weight(x.double(), shape, gpre.double(), **geom),
                            gb64=gpre.double().sum((0, 2, 3)), gw32=torch.nn.grad.conv2d_weight(x, shape, gpre, **geom), gb32=gpre.sum((0, 2, 3))))
        _A1_REF[(conv, levels)] = ref
    return _A1_REF[(conv, levels)]


def _a1_run(conv, ref, mags, want_bias, order=None, scaled=True):
    """ops.act_grad_x3 per level, then ONE ops.conv_x3_wgrad over all of them.  x and gs of the first and the last level are channel
    slices of wider buffers (batch strides that are not C*H*W), one of them 4 bytes off a 16-byte boundary."""
    from upflow_pytorch_amd import ops
    Cin, Cout, k, d, s = M.A1_CONVS[conv]
    uses = []
    for l in (order if order is not None else range(len(ref))):
        r = ref[l]
        if scaled:
            gs, slot, part = ops.act_grad_x3(r['gy'] * mags[l], r['y'], M.A1_SLOPE if r['y'] is not None else 0.0, want_bias=want_bias)
        else:
            gs, slot, part = M.a1_grad_pre(r['gy'], r['y'], mags[l]), None, None
        x = r['x']
        if l in (0, len(ref) - 1):
            B, _, H, W = x.shape
            xbuf = _flat_view(torch.full((B, Cin + 5, H, W), 3.0, device='cuda'), 1 if l else 0)
            xbuf[:, 5:] = x
            gbuf = _flat_view(torch.full((B, Cout + 3) + tuple(gs.shape[2:]), 7.0, device='cuda'), 0 if l else 1)
            gbuf[:, 2:2 + Cout] = gs
            x, gs = xbuf[:, 5:], gbuf[:, 2:2 + Cout]
            assert x.stride(0) != Cin * H * W and gs.stride(0) != Cout * gs.shape[2] * gs.shape[3]
        uses.append((x, gs, slot, part))
    return ops.conv_x3_wgrad(uses, Cin, Cout, k, d, s, want_bias=want_bias)


def _a1_sums(ref, mags):
    """fp64 truth and torch's fp32 result (per-level conv2d_weight, summed in fp32 in level order) at these magnitudes."""
    gw64 = sum(r['gw64'] * m for r, m in zip(ref, mags))
    gb64 = sum(r['gb64'] * m for r, m in zip(ref, mags))
    gw32, gb32 = torch.zeros_like(ref[0]['gw32']), torch.zeros_like(ref[0]['gb32'])
    for r, m in zip(ref, mags):
        gw32 += r['gw32'] * m
        gb32 += r['gb32'] * m
    return gw64, gb64, gw32, gb32


@pytest.mark.parametrize('want_bias', [True, False])
@pytest.mark.parametrize('conv,levels', M.A1_CASES)
def test_multi_level_weight_gradient_is_fp32_class(conv, levels, want_bias):
    """upf_conv_x3_wgrad over 2, 3, 5 and 6 uses of one convolution, every use with its own scale slot, against the fp64 sum over the
    levels.  Level l's grad_y is 2^(-7 ((l - rot) mod L)) times a randn tensor, for EVERY rotation rot: each level dominates the
    result once, and its neighbours' scales are 2^7 and 2^-7 away — a wrong level select in the GEMM (lsel, slice0, cps) or another
    level's 2^-s in the reduction is an error of orders of magnitude in that rotation, not of rounding.  Same bits on a second run;
    the levels in reverse order (another summation order) within the same bar.
    # Measured on MI355X, maxima over all cases and rotations, ours (torch fp32):  gw 7.1e-7 (9.8e-7);  gb 3.1e-7 (3.0e-7).
    # Tried on scratch builds (not committed): level 0's slot for every level in wgrad_x3_reduce_kernel -> all 28 cases fail, first
    # failing gw error 0.48 ... 9.4 of max |gw|; `slice > slice0` in wgrad_x3_kernel's level select -> all fail, 4.0e-4 ... 0.87."""
    ref = _a1_reference(conv, levels)
    L = len(ref)
    assert L in (2, 3, 5, 6)
    for rot in range(L):
        mags = M.a1_magnitudes(L, rot)
        gw64, gb64, gw32, gb32 = _a1_sums(ref, mags)
        gw, gb = _a1_run(conv, ref, mags, want_bias)
        _check('%s %s rot %d gw' % (conv, levels, rot), gw, gw32, gw64)
        if want_bias:
            _check('%s %s rot %d gb' % (conv, levels, rot), gb, gb32, gb64)
        else:
            assert gb is None
        if rot == 1:
            gw2, gb2 = _a1_run(conv, ref, mags, want_bias)
            assert torch.equal(gw, gw2) and (gb is None or torch.equal(gb, gb2))
            gwp, gbp = _a1_run(conv, ref, mags, want_bias, order=list(range(L))[::-1])
            _check('%s %s reversed gw' % (conv, levels), gwp, gw32, gw64)
            if want_bias:
                _check('%s %s reversed gb' % (conv, levels), gbp, gb32, gb64)


@pytest.mark.parametrize('case', [(2, 115, 128, 8, 26, 3, 1, 1), (1, 16, 32, 13, 27, 3, 1, 2), (2, 196, 32, 7, 11, 1, 1, 1), (1, 5, 3, 1, 1, 3, 1, 1)])
def test_one_level_list_equals_the_autograd_node(case):
    """act_grad_x3 + conv_x3_wgrad with a one-level list = the bits of ConvX3TrainFunction's gw and gb (which takes that path)."""
    from upflow_pytorch_amd import ops
    B, Cin, Cout, H, W, k, d, s = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Cin, H, W, generator=g).cuda()
    w = (torch.randn(Cout, Cin, k, k, generator=g) * 0.05).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    gy = torch.randn(B, Cout, *M.out_hw(H, W, s), generator=g).cuda() * 1e-3
    y, _, gw, gb = _train(x, w, b, gy, d, s, 0.1)
    gs, slot, part = ops.act_grad_x3(gy, y, 0.1, want_bias=True)
    gw1, gb1 = ops.conv_x3_wgrad([(x, gs, slot, part)], Cin, Cout, k, d, s, want_bias=True)
    assert torch.equal(gw, gw1) and torch.equal(gb, gb1)


# ---- A2: un-scaled uses (scale_slots == NULL) ------------------------------------------------------------------------------
@pytest.mark.parametrize('conv,levels', [('c115', 'pyramid'), ('s2', 'odd_s2'), ('p196', 'six'), ('d4', 'pixels')])
def test_unscaled_levels_meet_the_bar_for_o1_gradients(conv, levels):
    """upf_conv_x3_wgrad with a NULL slot array (ops.conv_x3_wgrad: every use's slot None): grad_pre is split as it is and nothing
    is un-scaled — plain behaviour for O(1) gradients, which is what is fed (randn, no magnitude ladder).  And a list that mixes
    scaled and un-scaled uses (NULL entries).
    # Measured on MI355X, maxima over the cases, ours (torch fp32):  all un-scaled 2.9e-7 (4.4e-7);  mixed 2.9e-7 (4.4e-7)."""
    from upflow_pytorch_amd import ops
    ref = _a1_reference(conv, levels)
    Cin, Cout, k, d, s = M.A1_CONVS[conv]
    mags = [1.0] * len(ref)
    gw64, _, gw32, _ = _a1_sums(ref, mags)
    gw, gb = _a1_run(conv, ref, mags, False, scaled=False)
    assert gb is None
    _check('%s %s un-scaled gw' % (conv, levels), gw, gw32, gw64)
    uses = []
    for l, r in enumerate(ref):
        if l % 2:
            uses.append((r['x'], M.a1_grad_pre(r['gy'], r['y'], 1.0), None, None))
        else:
            gs, slot, _ = ops.act_grad_x3(r['gy'], r['y'], M.A1_SLOPE if r['y'] is not None else 0.0)
            uses.append((r['x'], gs, slot, None))
    gwm, _ = ops.conv_x3_wgrad(uses, Cin, Cout, k, d, s)
    _check('%s %s mixed gw' % (conv, levels), gwm, gw32, gw64)


# ---- A3: the arguments of ConvX3TrainFunction ---------------------------------------------------------------------------------
A3_CASES = [(2, 35, 7, 9, 13, 3, 1, 1), (2, 35, 7, 9, 13, 1, 1, 1), (2, 35, 7, 9, 13, 3, 1, 2), (1, 70, 67, 6, 10, 3, 2, 1)]


def _a3_operands(case):
    B, Cin, Cout, H, W, k, d, s = case
    g = torch.Generator().manual_seed(sum(case) + k)
    x = torch.randn(B, Cin, H, W, generator=g).cuda()
    w = (torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    gy = torch.randn(B, Cout, *M.out_hw(H, W, s), generator=g).cuda() * 1e-4
    return x, w, b, gy


@pytest.mark.parametrize('case', A3_CASES)
def test_no_activation_against_fp64(case):
    """slope = 0: upf_act_grad_x3 with y = NULL (every conv_last, every layer without a ReLU); with and without a bias.
    # Measured on MI355X, maxima over the cases, ours (torch fp32):  gx 2.3e-7 (1.6e-7);  gw 1.5e-7 (2.6e-7);  gb 1.5e-7 (1.3e-7)."""
    B, Cin, Cout, H, W, k, d, s = case
    x, w, b, gy = _a3_operands(case)
    want = M.truth(x, w, gy, d, s)
    ref32 = M.torch32(x, w, gy, d, s)
    y, gx, gw, gb = _train(x, w, b, gy, d, s, 0.0)
    for name, got, r32, w64 in zip(('gx', 'gw', 'gb'), (gx, gw, gb), ref32, want):
        _check('%s slope 0 %s' % (case, name), got, r32, w64)
    # no bias: the bias enters neither gradient (no activation: no mask either) -> the same bits; and nothing comes back for it
    y0, gx0, gw0, gb0 = _train(x, w, None, gy, d, s, 0.0)
    assert gb0 is None and torch.equal(gx0, gx) and torch.equal(gw0, gw)


@pytest.mark.parametrize('case', A3_CASES)
def test_argument_combinations_give_the_bits_of_the_full_call(case):
    from upflow_pytorch_amd import ops
    B, Cin, Cout, H, W, k, d, s = case
    x, w, b, gy = _a3_operands(case)
    y, gx, gw, gb = _train(x, w, b, gy, d, s, 0.1)
    _, gx_a, gw_a, gb_a = _train(x, w, b, gy, d, s, 0.1)
    assert torch.equal(gx, gx_a) and torch.equal(gw, gw_a) and torch.equal(gb, gb_a)
    # a zero bias and no bias: the same forward, so the same mask -> gx and gw in the same bits; the node returns None for the bias
    yz, gxz, gwz, _ = _train(x, w, torch.zeros_like(b), gy, d, s, 0.1)
    yn, gxn, gwn, gbn = _train(x, w, None, gy, d, s, 0.1)
    assert torch.equal(yz, yn) and torch.equal(gxz, gxn) and torch.equal(gwz, gwn) and gbn is None
    ctx = types.SimpleNamespace(saved_tensors=(x, w, yn), cfg=(d, 0.1, False, s), needs_input_grad=(True, True, False, False, False, False))
    out = ops.ConvX3TrainFunction.backward(ctx, gy)
    assert len(out) == 6 and out[2] is None and all(o is None for o in out[3:])
    assert torch.equal(out[0], gxn) and torch.equal(out[1], gwn)
    # x without requires_grad: the data gradient is skipped, gw and gb are the full call's bits
    _, gx1, gw1, gb1 = _train(x, w, b, gy, d, s, 0.1, x_grad=False)
    assert gx1 is None and torch.equal(gw1, gw) and torch.equal(gb1, gb)
    # frozen weight, trainable bias: gw is dropped, gb is kept
    _, gx2, gw2, gb2 = _train(x, w, b, gy, d, s, 0.1, w_grad=False)
    assert gw2 is None and torch.equal(gb2, gb) and torch.equal(gx2, gx)
    # frozen bias: no bias partials
    _, gx3, gw3, gb3 = _train(x, w, b, gy, d, s, 0.1, b_grad=False)
    assert gb3 is None and torch.equal(gw3, gw) and torch.equal(gx3, gx)
    # a grad_y that is no channel slice: expanded (stride 0) and transposed -> the .float().contiguous() branch
    ho, wo = gy.shape[2:]
    ge = gy[:, :, :, :1].expand(B, Cout, ho, wo)
    gt = gy.transpose(2, 3).contiguous().transpose(2, 3)
    assert not ge.is_contiguous() and (not gt.is_contiguous() or ho == 1 or wo == 1) and torch.equal(gt, gy)
    for odd, dense in ((ge, ge.contiguous()), (gt, gy)):
        got, exp = _train(x, w, b, odd, d, s, 0.1), _train(x, w, b, dense, d, s, 0.1)
        assert all(torch.equal(p, q) for p, q in zip(got, exp))
    # slope 1: the mask multiplies by 1 -> the backward of slope 0 (no mask at all), bit for bit
    _, gx5, gw5, gb5 = _train(x, w, b, gy, d, s, 1.0)
    _, gx6, gw6, gb6 = _train(x, w, b, gy, d, s, 0.0)
    assert torch.equal(gx5, gx6) and torch.equal(gw5, gw6) and torch.equal(gb5, gb6)


# ---- A4: activation magnitude in the weight gradient -------------------------------------------------------------------------
@pytest.mark.parametrize('s', [1, 2])
def test_activation_magnitude_in_the_weight_gradient(s):
    """The backward twin of test_conv_x3_operand_magnitudes: the weight gradient splits the activations UN-SCALED, so |x| < 2^-3 has a
    subnormal low half (up to 2^-25 of absolute error each): fp32-class for |x| >= 1, for tiny activations the documented floor
    2^-25 * max_co sum |grad_pre[:, co]| (every activation off by the half-spacing, same sign).  gx and gb read x only through the
    mask: where the forward's mask is that of the first magnitude they are the same bits; they meet the bar in any case.
    # Measured on MI355X, gw ours (torch fp32) for |x| ~ 1e-4, 1e-2, 30, 3000:
    #   stride 1: 1.9e-4 (2.9e-7) = 0.07 of the floor, 2.4e-6 (3.7e-7), 1.6e-7 (3.4e-7), 1.8e-7 (3.9e-7)
    #   stride 2: 1.6e-4 (1.8e-7) = 0.13 of the floor, 1.8e-6 (1.7e-7), 1.2e-7 (1.7e-7), 1.3e-7 (1.4e-7)
    # gx <= 6.4e-7 (3.1e-7), gb <= 1.8e-7 (1.2e-7).  Stride 2: the forward's masks were equal at all four magnitudes, gx and gb compared
    # bit for bit; stride 1: pre-activations within rounding of zero changed side, the bar alone."""
    first = None
    for mag in M.A4_MAGS:
        x, w, b, gy = (t.cuda() for t in M.a4_inputs(mag, s))
        y, gx, gw, gb = _grads(x, w, b, gy, 1, s, M.A4_SLOPE)
        gpre = gy * _mask_of(y, M.A4_SLOPE)
        want_x, want_w, want_b = M.truth(x, w, gpre, 1, s)
        gx32, gw32, gb32 = M.torch32(x, w, gpre, 1, s)
        err, err32 = _rel(gw, want_w), _rel(gw32, want_w)
        abs_err, floor = float((gw.double() - want_w).abs().max()), M.a4_floor(gpre)
        print('|x| ~ %g stride %d gw: max err %.2e of max |.| (torch fp32: %.2e), absolute %.2e, floor %.2e' % (mag, s, err, err32, abs_err, floor))
        assert err <= M.bar(err32) or abs_err <= floor, (mag, err, err32, abs_err, floor)
        if mag >= 1.0:
            assert err <= M.bar(err32), (mag, err, err32)
        _check('|x| ~ %g stride %d gx' % (mag, s), gx, gx32, want_x)
        _check('|x| ~ %g stride %d gb' % (mag, s), gb, gb32, want_b)
        if first is None:
            first = (y > 0, gx, gb)
        elif torch.equal(first[0], y > 0):
            print('|x| ~ %g: same mask as the first magnitude' % mag)
            assert torch.equal(first[1], gx) and torch.equal(first[2], gb), mag


# ---- A5: dynamic range inside grad_y -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', M.A5_VARIANTS)
@pytest.mark.parametrize('layer', M.A5_LAYERS)
def test_dynamic_range_inside_grad_y(layer, variant):
    """One part of grad_y — the right half of the image, batch sample 1, the upper half of the output channels — is 2^-r of the rest,
    r = 8 ... 32, and the error is measured INSIDE that part against the part's own fp64 maximum (for the image half: more than a
    kernel radius from the seam).  ONE power of two per tensor: elements below 2^-16 of the maximum have a subnormal low half, an
    absolute error of up to 2^-38 * max |grad_pre| each (tests/_x3_model.py: a5_floors).  Bound per part: max(bar, that floor); for
    r <= 14 the bar alone ("down to 2^-16 of the maximum keeps 22 bits"); the stride-2 data gradient (plain fp32) and the bias
    gradient the bar alone at every r.  At r = 32 the attenuated gx is non-zero wherever the truth exceeds the floor.
    # Measured on MI355X, err / the part's max for r = 8, 14, 18, 24, 32, ours (torch fp32):
    #   stride 1 gx, right half:  3.7e-7 (2.7e-7), 4.7e-7 (2.7e-7), 3.2e-6 (2.7e-7), 2.0e-4 (2.7e-7), 5.3e-2 (2.7e-7) = 0.17 of the floor
    #   stride 1 gx, sample 1:    3.7e-7 (2.8e-7), 4.8e-7 (2.8e-7), 3.3e-6 (2.8e-7), 2.1e-4 (2.8e-7), 5.3e-2 (2.8e-7) = 0.16 of the floor
    #   stride 1 gw rows:         1.2e-7 (2.0e-7), 1.9e-7 (2.0e-7), 2.0e-6 (2.4e-7), 1.4e-4 (2.1e-7), 3.9e-2 (2.4e-7) = 0.05 of the floor
    #   stride 2 gx: right half 3.6e-7 (1.9e-7), sample 1 3.4e-7 (2.5e-7) at every r;  stride 2 gw rows: 1.2e-7, 1.7e-7, 1.9e-6, 9.1e-5,
    #   2.3e-2 (<= 1.9e-7) = 0.01 of the floor;  gb rows: 2.3e-7 (8.2e-8) / 1.3e-7 (1.3e-7) at every r.
    # The model (tests/_x3_model.py, no accumulation rounding) gives 3.3e-6, 2.0e-4, 5.3e-2 for r = 18, 24, 32: the floor IS the design's."""
    B, Cin, Cout, H, W, k, d, s = layer
    for r in M.A5_R:
        x, w, b, gy = (t.cuda() for t in M.a5_inputs(layer, variant, r))
        y, gx, gw, gb = _grads(x, w, b, gy, d, s, M.A5_SLOPE)
        gpre = gy * _mask_of(y, M.A5_SLOPE)
        want_x, want_w, want_b = M.truth(x, w, gpre, d, s)
        gx32, gw32, gb32 = M.torch32(x, w, gpre, d, s)
        floor_x, floor_w = M.a5_floors(x, w, gpre)
        label = '%s stride %d' % (variant, s)
        for name, got, r32, w64 in (('gx', gx, gx32, want_x), ('gw', gw, gw32, want_w), ('gb', gb, gb32, want_b)):
            _check('%s r=%d global %s' % (label, r, name), got, r32, w64)
        part = M.a5_gx_part(layer, variant)
        if part is not None:
            M.a5_check('gx', gx[part], gx32[part], want_x[part], floor_x if s == 1 else 0.0, r, label)
            if r == 32:
                big = want_x[part].abs() > floor_x
                assert bool(big.any()) and bool((gx[part][big] != 0).all()), 'attenuated data gradient flushed to zero'
        else:
            h = Cout // 2
            M.a5_check('gw', gw[h:], gw32[h:], want_w[h:], floor_w, r, label)
            M.a5_check('gb', gb[h:], gb32[h:], want_b[h:], 0.0, r, label)


# ---- A6: zeros, non-finite values, the ends of the exponent range --------------------------------------------------------------
A6_CASES = [(2, 19, 12, 9, 14, 3, 1, 1), (2, 16, 12, 9, 13, 3, 1, 2), (2, 19, 12, 9, 14, 1, 1, 1)]


def _a6_operands(case):
    B, Cin, Cout, H, W, k, d, s = case
    g = torch.Generator().manual_seed(sum(case) + 3 * k)
    x = torch.randn(B, Cin, H, W, generator=g).cuda()
    w = (torch.randn(Cout, Cin, k, k, generator=g) * 0.1).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    gy = torch.randn(B, Cout, *M.out_hw(H, W, s), generator=g).cuda()
    return x, w, b, gy


@pytest.mark.parametrize('case', A6_CASES)
def test_all_zero_gradient_gives_exact_zeros(case):
    B, Cin, Cout, H, W, k, d, s = case
    x, w, b, gy = _a6_operands(case)
    for slope in (0.1, 0.0):
        _, gx, gw, gb = _grads(x, w, b, torch.zeros_like(gy), d, s, slope)
        for t in (gx, gw, gb):
            assert bool(torch.isfinite(t).all()) and bool((t == 0).all())


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('case', A6_CASES)
def test_non_finite_gradient_elements_surface(case, bad):
    """One NaN / one +inf in grad_y at (n0, c0, y0, x0) (ordinary values a step can produce): it reaches gb[c0], every gw[c0], and gx
    on exactly the pixels of sample n0 whose receptive field holds (y0, x0); everything else stays finite.  NaN gradients do not
    define the scale (grad_absmax_kernel): the finite rest is still scaled from the finite maximum — grad_y is randn * 1e-6 here, far
    below the un-scaled split's floor — and meets the bar.
    # Measured on MI355X with the NaN, maxima over the cases, ours (torch fp32):  gw rows 1.7e-7 (3.0e-7);  gb 1.9e-7 (8.3e-8);
    # gx of the other sample 2.6e-7 (2.0e-7)."""
    B, Cin, Cout, H, W, k, d, s = case
    x, w, b, gy = _a6_operands(case)
    gy = gy * 1e-6
    n0, c0, y0, x0 = 1, 3, 4, 5
    clean = gy.clone()
    clean[n0, c0, y0, x0] = 0.0
    gy[n0, c0, y0, x0] = bad
    y, gx, gw, gb = _grads(x, w, b, gy, d, s, 0.1)
    hit = torch.zeros_like(gy)
    hit[n0, c0, y0, x0] = 1.0
    reach = torch.nn.grad.conv2d_input(x.shape, torch.ones_like(w).double(), hit.double(), stride=s, padding=d * (k - 1) // 2, dilation=d) > 0
    assert int(reach[n0].sum()) >= Cin and not bool(reach[0].any())
    assert not bool(torch.isfinite(gb[c0])) and not bool(torch.isfinite(gw[c0]).any())
    assert not bool(torch.isfinite(gx[reach]).any()), 'a non-finite gradient element vanished from the data gradient'
    others = [c for c in range(Cout) if c != c0]
    assert bool(torch.isfinite(gx[~reach]).all()) and bool(torch.isfinite(gw[others]).all()) and bool(torch.isfinite(gb[others]).all())
    if bad != bad:
        gpre = clean * _mask_of(y, 0.1)
        want_x, want_w, want_b = M.truth(x, w, gpre, d, s)
        gx32, gw32, gb32 = M.torch32(x, w, gpre, d, s)
        _check('%s NaN: gw rows of the other channels' % (case,), gw[others], gw32[others], want_w[others])
        _check('%s NaN: gb of the other channels' % (case,), gb[others], gb32[others], want_b[others])
        _check('%s NaN: gx of the other sample' % (case,), gx[0], gx32[0], want_x[0])


@pytest.mark.parametrize('case', A6_CASES)
def test_gradients_scale_exactly_up_to_the_clamp(case):
    """grad_y * 2^k, k = +20, +60, -60, -100, gives the bits of k = 0 times 2^k wherever that product is a normal fp32 number, and is
    within one subnormal spacing (2^-149) elsewhere: both signs, and out to the clamp of x3_scale_of.  That rule clamps the scale's
    exponent to +-100, and only an un-clamped scale can give the same split: the base gradient is normalised (a power of two from
    its maximum, no activation: grad_pre = grad_y) so that max |grad_pre| lies in [2^13, 2^14) — scale 2^0 at k = 0, 2^100, the last
    un-clamped one, at k = -100.  PAST the clamp (the same tensor at 2^-113: scale 2^100, maximum at 2^0 instead of 2^13) the bits
    differ and the result is that of an un-scaled O(1) gradient: it meets the bar against fp64.  A subnormal maximum (2^-130 of
    randn: every half is zero after the clamped scale) gives finite results.
    # Measured on MI355X: an un-normalised randn grad_y (maximum ~2^2) at 2^-100 is 11 octaves past the clamp: 19 - 26 % of the gx / gw
    # elements differ from the k = 0 bits, by at most 1.2e-7 of the maximum.
    # Past the clamp against fp64, maxima over the cases, ours (torch fp32):  gx 3.0e-7 (2.0e-7);  gw 1.6e-7 (4.0e-7);  gb 1.4e-7 (9.6e-8)."""
    B, Cin, Cout, H, W, k, d, s = case
    x, w, b, gy = _a6_operands(case)
    e = int(torch.floor(torch.log2(gy.abs().max())))
    base = gy * 2.0 ** (13 - e)
    assert 2.0 ** 13 <= float(base.abs().max()) < 2.0 ** 14
    _, gx0, gw0, gb0 = _grads(x, w, b, base, d, s, 0.0)
    assert float(gx0.abs().max()) > 0 and float(gw0.abs().max()) > 0
    for sh in (20, 60, -60, -100):
        _, gx, gw, gb = _grads(x, w, b, base * 2.0 ** sh, d, s, 0.0)
        for name, got, g0 in (('gx', gx, gx0), ('gw', gw, gw0), ('gb', gb, gb0)):
            prod = g0.double() * 2.0 ** sh
            normal = (prod.abs() >= 2.0 ** -126) & (prod.abs() <= 3.4e38)
            assert bool(normal.any())
            assert torch.equal(got[normal].double(), prod[normal]), (name, sh)
            assert bool(((got.double() - prod).abs()[~normal] <= 2.0 ** -149).all()), (name, sh)
    tiny = base * 2.0 ** -113
    _, gx, gw, gb = _grads(x, w, b, tiny, d, s, 0.0)
    want = M.truth(x, w, tiny, d, s)
    ref32 = M.torch32(x, w, tiny, d, s)
    for name, got, r32, w64 in zip(('gx', 'gw', 'gb'), (gx, gw, gb), ref32, want):
        _check('%s past the clamp %s' % (case, name), got, r32, w64)
    for slope in (0.0, 0.1):
        for t in _grads(x, w, b, gy * 2.0 ** -130, d, s, slope)[1:]:
            assert bool(torch.isfinite(t).all())
