"""The backward-warp kernels (csrc/warp.hip: warp_fwd_kernel with 1 / 2 / 4 pixels per thread, the narrow kernel, the octet kernel,
warp_bwd_kernel with its lane merge in the split and the unsplit launch form, the finishing kernel) against the sampling model of
tests/_exact_model.py — a reference, not each other.  tests/test_exact_model_cpu.py checks every condition without a GPU.

Two regimes:
  dyadic    positions, weights, products and partial sums exact in fp32 in any order: y, gx and gflow must equal the plain fp64
            bilinear formulas rounded ONCE to the storage type.  No tolerance.
  general   the weights are the fp32 values csrc/sampling.hpp prescribes step by step (taps32); y within gamma_4 * sum |w_k v_k| of
            their fp64 dot product (fp32: inside the interval; 16-bit: RNE of one of its two ends — they differ for <= 1 % of the
            elements —, or a 16-bit value between them where cancellation makes the interval wider than one 16-bit step:
            _exact_model.accept_y); gflow within gamma_(12 C + 2) * sum |terms| + 2^-44 per channel slice.
  gx        bit for bit in BOTH regimes: integers (rint(fp32(w * g) * 2^44)) summed in any order, converted once.
Pixels the mask rejects are exact zeros (y, gflow); NaN / inf / -1e30 flows give 0 in every mode.

Every operand and output is a block of a NaN-filled arena: a read outside an operand turns outputs into NaN, a store outside an
output shows in `untouched`.

Routes (tests/_exact_model.py warp_pxt / pick_cpt, read off upf_warp_forward_pitched / pick_cpt): narrow kernel W < 2; four pixels
per thread fp32 with W % 4 == 0, 16-byte aligned y and B*H*W >= 65536; pairs for 16-bit types with an even pitch, a 4-byte aligned
y and — at an odd W — a batch stride that promises the full pitch behind every row; else one pixel per thread.  Channel slices over
blockIdx.y from 16 channels up at these sizes (backward: fixed-point gflow partial sums)."""
import numpy as np
import pytest
import torch

import _exact_model as em

pytestmark = pytest.mark.gpu

F32 = em.F32
SDT = [pytest.param(d, id=em.SAMP_NAMES[d]) for d in em.SAMP_DTYPES]
DT16 = [pytest.param(d, id=em.SAMP_NAMES[d]) for d in em.SAMP_DTYPES[:2]]
OUTSIDE = 'stored outside the output'
UPF_EUNSUPPORTED = -4


def sid(s):
    return 'x'.join(str(v) for v in s)


def shifts_of(B):
    return (0,) if B == 1 else (0, B // 2)


def arena(dtype, nblocks, numel):
    elems = nblocks * (numel + em.Arena.MARGIN + 64) + em.Arena.MARGIN + 64
    return em.Arena32('cuda', elems) if dtype == F32 else em.Arena(dtype, 'cuda', elems)


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def lib_args(dtype, mode, shift):
    from upflow_pytorch_amd import _lib
    return _lib._DTYPES[dtype], em.MODE_CODES[mode], int(shift), _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))


def expect_y(c, dtype):
    """{(mode, shift): (ref fp64, bound fp64)} of one case: the bound is 0 in the dyadic regime."""
    out = {}
    for mode in em.MODES:
        for shift in shifts_of(c['shape'][0]):
            ref, ra = em.warp_forward_ref(c['x'], c['t'], mode, shift)
            out[mode, shift] = (ref, 0.0 * ra if c['dyadic'] else em.gamma(4) * ra)
    return out


def check_y(got, ref, bound, dtype, what):
    ok = em.accept_y(got, ref, bound, dtype)
    if not ok.all():
        bad = np.argwhere(~ok)[0]
        g = got.detach().cpu().double().numpy()
        raise AssertionError('%s: %d of %d outputs outside their bound (first at %s: got %r, reference %r +- %.3g)'
                             % (what, int((~ok).sum()), ok.size, tuple(bad), g[tuple(bad)], ref[tuple(bad)], float(np.broadcast_to(bound, ref.shape)[tuple(bad)])))


def carve(A, B, C, H, W, form, fill=None):
    """One [B,C,H,W] operand / output in the arena.  'plain': a contiguous block; 'even' / 'odd': a channel slice (one foreign plane
    either side) whose first element sits an even / odd number of elements past a 16-byte boundary; 'pitched': rows padded as
    ops.empty_nchw pads them, 16-byte aligned."""
    from upflow_pytorch_amd import ops
    if form == 'plain':
        return A.block(B, C, H, W, fill=fill)
    if form == 'pitched':
        Wp = ops.empty_nchw((B, C, H, W), A.dtype, 'cuda').stride(2) if H > 1 else (W + 7) // 8 * 8
        return A.nchw(B, C, H, W, pitch=Wp, align=8, fill=fill)
    m = (H * W + (form == 'odd')) % 2
    v = A.block(B, C + 2, H, W, misalign=m)[:, 1:1 + C]
    assert (v.data_ptr() // v.element_size()) % 2 == (form == 'odd')
    if fill is not None:
        v.copy_(fill.to(A.dtype))
    return v


def forms_of(dtype, shape):
    from upflow_pytorch_amd import ops
    B, C, H, W = shape
    f = ['plain', 'even', 'odd']
    if dtype != F32 and W >= 8 and W % ops.PITCH_MULTIPLE:
        f.append('pitched')
    return f


def run_forward(c, dtype, form, expect, what):
    from upflow_pytorch_amd import _lib, ops
    B, C, H, W = c['shape']
    keys = list(expect)
    A = arena(dtype, 1 + len(keys), B * (C + 2) * H * (W + 8))
    A32 = arena(F32, 1, B * 2 * H * W)
    flow = A32.block(B, 2, H, W, fill=t_(c['flow']))
    x = carve(A, B, C, H, W, form, t_(c['x']))
    ys = [carve(A, B, C, H, W, form) for _ in keys]
    snap, snap32 = A.snapshot(), A32.snapshot()
    for (mode, shift), y in zip(keys, ys):
        if form == 'plain':
            _lib.call('upf_warp_forward', _lib.ptr(x), _lib.ptr(flow), _lib.ptr(y), B, C, H, W, *lib_args(dtype, mode, shift))
        else:
            assert ops.warp_into(x, flow, y, mode, shift) is y
    torch.cuda.synchronize()
    for k, y in zip(keys, ys):
        check_y(y, expect[k][0], expect[k][1], dtype, '%s %s %s' % (what, form, k))
    # a pitched row may receive column W of an odd width (the pair store's second pixel), nothing beyond it
    allowed = [y.as_strided((B, C, H, W + W % 2), y.stride(), y.storage_offset()) if form == 'pitched' else y for y in ys]
    assert A.untouched(snap, *allowed) and A32.untouched(snap32), '%s %s: %s' % (what, form, OUTSIDE)


@pytest.mark.parametrize('shape', em.WARP_DYADIC + em.WARP_GENERAL, ids=sid)
@pytest.mark.parametrize('dtype', SDT)
def test_warp_forward(dtype, shape):
    """Every form (upf_warp_forward; channel slices at even and odd element offsets; pitched rows) x mask mode x batch shift x flow
    pattern against the one expectation of the case."""
    dyadic = shape in em.WARP_DYADIC
    for pattern in em.FWD_PATTERNS:
        c = em.warp_case(shape, dtype, pattern, dyadic)
        expect = expect_y(c, dtype)
        for form in forms_of(dtype, shape):
            run_forward(c, dtype, form, expect, '%s %s' % (sid(shape), pattern))


@pytest.mark.parametrize('form', ['plain', 'odd'])
def test_warp_forward_four_pixels_per_thread_and_its_fallback(form):
    """fp32 at the smallest grid that takes four pixels per thread; the same grid with a 4-byte but not 16-byte aligned y must take
    one pixel per thread and give values inside the same bounds."""
    B, C, H, W = em.WARP_PXT4
    assert em.warp_pxt(F32, B, C, H, W) == 'pxt4' and em.warp_pxt(F32, B, C, H, W, y_align=4) == 'pxt1'
    for pattern in ('rand4', 'nonfinite', 'edges'):
        c = em.warp_case(em.WARP_PXT4, F32, pattern, False)
        run_forward(c, F32, form, expect_y(c, F32), '%s %s' % (sid(em.WARP_PXT4), pattern))


@pytest.mark.parametrize('shape', em.WARP_C8_DYADIC + em.WARP_C8_GENERAL, ids=sid)
@pytest.mark.parametrize('dtype', DT16)
def test_warp_forward_octets(dtype, shape):
    """upf_warp_forward_c8 with 1, 4 and 5 octets (blockIdx.y covers four: the fifth is a second trip of the loop)."""
    from upflow_pytorch_amd import ops
    B, C, H, W = shape
    dyadic = shape in em.WARP_C8_DYADIC
    for pattern in ('const', 'rand4', 'nonfinite'):
        c = em.warp_case(shape, dtype, pattern, dyadic)
        expect = expect_y(c, dtype)
        A = arena(dtype, 1 + len(expect), B * (C + 16) * H * W)
        A32 = arena(F32, 1, B * 2 * H * W)
        flow = A32.block(B, 2, H, W, fill=t_(c['flow']))
        x8 = A.c8(B, C, H, W, fill=t_(c['x']))
        ys = [A.c8(B, C, H, W) for _ in expect]
        snap = A.snapshot()
        for (mode, shift), y8 in zip(expect, ys):
            assert ops.warp_c8_into(x8, flow, y8, mode, shift) is y8
        torch.cuda.synchronize()
        for k, y8 in zip(expect, ys):
            check_y(em.from_c8(y8.cpu(), C).contiguous(), expect[k][0], expect[k][1], dtype, 'octets %s %s %s' % (sid(shape), pattern, k))
        assert A.untouched(snap, *ys), OUTSIDE


def test_warp_forward_refuses_a_pitch_below_two_columns():
    from upflow_pytorch_amd import _lib
    x, y = torch.zeros(3 * 9 * 2, device='cuda'), torch.zeros(3 * 9 * 2, device='cuda')
    flow = torch.zeros(1, 2, 9, 1, device='cuda')
    rc = _lib.lib().upf_warp_forward_pitched(_lib.ptr(x), 0, 2, _lib.ptr(flow), _lib.ptr(y), 0, 2, 1, 3, 9, 1, *lib_args(F32, 'none', 0))
    assert rc == UPF_EUNSUPPORTED


@pytest.mark.parametrize('extra', [0, 1, 3], ids=['minimum', 'minimum_plus_1', 'full_pitch'])
@pytest.mark.parametrize('dtype', DT16)
def test_warp_forward_pitched_at_the_admitted_minimum_batch_stride(dtype, extra):
    """include/upflow_hip.h admits y_batch_stride >= C*H*pitch - (pitch - W): the padding of an image's last row need not exist.  y is
    carved with exactly (B-1) * stride + that minimum elements; at an odd W nothing outside the [.., :W] view may be written unless
    the stride promises the full pitch (then column W of a row, and only that)."""
    from upflow_pytorch_amd import _lib
    shape = (2, 5, 7, 13)
    B, C, H, W = shape
    yp = 16
    least = C * H * yp - (yp - W)
    ybs = least + extra
    full = ybs >= C * H * yp
    assert em.warp_pxt(dtype, B, C, H, W, yp, 16, ybs) == ('pxt2' if full else 'pxt1')
    c = em.warp_case(shape, dtype, 'rand4', False)
    expect = expect_y(c, dtype)
    A = arena(dtype, 1 + len(expect), B * (C + 2) * H * yp)
    A32 = arena(F32, 1, B * 2 * H * W)
    flow = A32.block(B, 2, H, W, fill=t_(c['flow']))
    x = A.block(B, C, H, W, fill=t_(c['x']))
    ys = []
    for _ in expect:
        raw = A._take((B - 1) * ybs + (C * H * yp if full else least), 0, 8)
        ys.append(raw.as_strided((B, C, H, W), (ybs, H * yp, yp, 1)))
    snap = A.snapshot()
    for (mode, shift), y in zip(expect, ys):
        _lib.call('upf_warp_forward_pitched', _lib.ptr(x), 0, 0, _lib.ptr(flow), _lib.ptr(y), ybs, yp, B, C, H, W, *lib_args(dtype, mode, shift))
    torch.cuda.synchronize()
    for k, y in zip(expect, ys):
        check_y(y, expect[k][0], expect[k][1], dtype, 'stride %d %s' % (ybs, k))
    allowed = [y.as_strided((B, C, H, W + 1), y.stride(), y.storage_offset()) if full else y for y in ys]
    assert A.untouched(snap, *allowed), OUTSIDE


@pytest.mark.parametrize('shape', em.WARP_DYADIC + em.WARP_BWD_GENERAL, ids=sid)
@pytest.mark.parametrize('dtype', SDT)
def test_warp_backward(dtype, shape):
    """upf_warp_backward: gx bit for bit against the fixed-point model; gflow exact (dyadic) or within its bound (general); exact
    zeros where the mask rejects the pixel and at non-finite flows; nothing stored outside gx / gflow."""
    from upflow_pytorch_amd import _lib
    B, C, H, W = shape
    dyadic = shape in em.WARP_DYADIC
    slices = em.pick_cpt(B, C, H * W)[1]
    n_terms = 3 * 4 * C + 2
    for pattern in em.BWD_PATTERNS:
        c = em.warp_case(shape, dtype, pattern, dyadic)
        keys = [(m, s) for m in em.MODES for s in shifts_of(B)]
        A = arena(dtype, 2 + len(keys), B * C * H * W)
        A32 = arena(F32, 1 + len(keys), B * 2 * H * W)
        flow = A32.block(B, 2, H, W, fill=t_(c['flow']))
        x, gy = A.block(B, C, H, W, fill=t_(c['x'])), A.block(B, C, H, W, fill=t_(c['gy']))
        outs = [(A.block(B, C, H, W), A32.block(B, 2, H, W)) for _ in keys]
        ws = torch.empty(_lib.lib().upf_warp_backward_workspace_bytes(B, C, H, W), dtype=torch.uint8, device='cuda')
        snap, snap32 = A.snapshot(), A32.snapshot()
        got = []
        for (mode, shift), (gx, gf) in zip(keys, outs):
            _lib.call('upf_warp_backward', _lib.ptr(x), _lib.ptr(flow), _lib.ptr(gy), _lib.ptr(gx), _lib.ptr(gf), _lib.ptr(ws),
                      B, C, H, W, *lib_args(dtype, mode, shift))
            torch.cuda.synchronize()
            got.append((gx.cpu(), gf.cpu()))
        assert A.untouched(snap, *[o[0] for o in outs]) and A32.untouched(snap32, *[o[1] for o in outs]), OUTSIDE
        for (mode, shift), (gx, gf) in zip(keys, got):
            what = '%s %s %s shift %d' % (sid(shape), pattern, mode, shift)
            want, _ = em.warp_gx_model(c['gy'], c['t'], mode, shift, dtype)
            bad = ~((gx == want) | (torch.isnan(gx) & torch.isnan(want)))
            assert not bool(bad.any()), '%s: gx differs at %d of %d elements (first %s: got %r, want %r)' % (
                what, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), float(gx[bad][0]), float(want[bad][0]))
            ref_x, ref_f, ref_fa = em.warp_backward_ref(c['x'], c['gy'], c['t'], mode, shift)
            g64 = gf.double().numpy()
            if dyadic:
                assert np.array_equal(g64, ref_f), '%s: gflow differs at %d pixels' % (what, int((g64 != ref_f).sum()))
            else:
                bound = em.gamma(n_terms) * ref_fa + 2.0 ** -44 * slices
                worst = np.abs(g64 - ref_f) - bound
                assert np.all(worst <= 0), '%s: gflow outside its bound at %d pixels, by up to %.3g' % (what, int((worst > 0).sum()), float(worst.max()))
            rejected = np.broadcast_to(~c['t']['valid'][mode][:, None], g64.shape)
            assert np.all(g64[rejected] == 0), '%s: gflow of a rejected pixel is not zero' % what
            if pattern == 'nonfinite':
                for n, _, i, j in em.nonfinite_places(B, H, W):
                    assert np.all(g64[n, :, i, j] == 0), what
