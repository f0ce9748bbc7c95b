"""The SGU interpolation-blend (csrc/sgu_blend.hip: blend_fwd_kernel with its flow16 forms, blend_bwd_kernel with its lane merge and
its partial last workgroup, the final level's sigmoid map, resize gradient and sigmoid gradient), the occlusion check and the soft
census distance (csrc/misc.hip) against the fp64 models of tests/_exact_model.py — references, not each other.
tests/test_exact_model_cpu.py checks every guard, cap, route and count without a GPU.  DESIGN.md 4.12.

Blend    dyadic (sizes 2^k + 1, flows on the 1/8 grid, logits in {0, +-100} so that m is exactly 0.5 / 1 / 0): flow_up, inter_flow,
         inter_mask, the 16-bit flow16 (both layouts, the six padding lanes exact zeros), g_flow_init and all three channels of g_x_out
         equal the fp64 formulas rounded once.  No tolerance.
         general: m within 5 u of the fp64 sigmoid; flow_up within gamma_7 (sum |w v| |1 - m| + |f m|) + 5 u |f - warped|; g_x_out
         within gamma_28 sum |terms|, evaluated with the m the forward returned (the backward recomputes the same sigmoid).
         g_flow_init is bit for bit in BOTH regimes given that m: integers rint(fp32(fp32((1 - m) g) w_k) 2^44) + rint(fp32(m g) 2^44).
         final level: inter_flow and (logits in {0, +-100}) inter_mask bit for bit from the fp32 lerp chain; the blend in the general
         regime on them; the backward's bounds carried through the exact adjoint of the resize.
Occlusion  dyadic: both masks equal the model at every pixel.  General: pixels whose comparison the association of the fp32 tap sum
         could decide either way (|lhs - thr| <= gamma_6 sum |terms| + 2 u thr) are left out, every other pixel must match.
Census   general only (hardware rsq / rcp, 1 ulp): running first-order bounds per term, doubled, plus gamma_K of the accumulation.

Every operand and output is a block of a NaN-filled fp32 / 16-bit arena; `untouched` is asserted after every call."""
import numpy as np
import pytest
import torch

import _exact_model as em

pytestmark = pytest.mark.gpu

F32 = em.F32
OUTSIDE = 'stored outside the output'
BDT = [pytest.param(d, id=em.SAMP_NAMES[d]) for d in em.BLEND_DTYPES]
DT16 = [pytest.param(d, id=em.SAMP_NAMES[d]) for d in em.SAMP_DTYPES[:2]]


def sid(s):
    return 'x'.join(str(v) for v in s)


def arena(dtype, nblocks, numel):
    elems = nblocks * (numel + em.Arena.MARGIN + 64) + em.Arena.MARGIN + 64
    return em.Arena32('cuda', elems) if dtype == F32 else em.Arena(dtype, 'cuda', elems)


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def stream():
    from upflow_pytorch_amd import _lib
    return _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))


def same_bits(got, want):
    g, w = got.detach().cpu().contiguous(), torch.as_tensor(want).contiguous()
    assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
    return (g == w) | (torch.isnan(g) & torch.isnan(w))


def assert_exact(got, want64, what, dtype=F32):
    ok = same_bits(got, em.rne(want64, dtype))
    assert bool(ok.all()), '%s: differs from the fp64 value rounded once at %d of %d elements (first %s)' % (
        what, int((~ok).sum()), ok.numel(), tuple((~ok).nonzero()[0].tolist()))


def assert_within(got, ref, bound, what):
    g = got.detach().cpu().double().numpy()
    with np.errstate(all='ignore'):
        bad = ~(np.abs(g - ref) <= bound) & ~(np.isnan(ref) & np.isnan(g))
    assert not bad.any(), '%s: %d of %d values outside their bound (first %s: got %r, reference %r +- %.3g)' % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), g[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])],
        float(np.broadcast_to(bound, ref.shape)[tuple(np.argwhere(bad)[0])]))


def run_blend(c, dtype):
    """upf_sgu_blend_forward and upf_sgu_blend_backward of one case in the arenas -> dict of CPU tensors flow_up, inter_flow, inter_mask,
    g_init, g_xo."""
    from upflow_pytorch_amd import _lib
    B, Hf, Wf = c['shape']
    h, w = c['lo']
    HW = Hf * Wf
    A32 = arena(F32, 9, B * 3 * HW)
    A = A32 if dtype == F32 else arena(dtype, 1, B * 3 * h * w)
    f0 = A32.block(B, 2, Hf, Wf, fill=t_(c['flow_init']))
    g = A32.block(B, 2, Hf, Wf, fill=t_(c['g']))
    xo = A.block(B, 3, h, w, fill=t_(c['x_out']))
    fu, fi, gi = (A32.block(B, 2, Hf, Wf) for _ in range(3))
    fm = A32.block(B, 1, Hf, Wf)
    gxo = A32.block(B, 3, h, w)
    lib = _lib.lib()
    ws_f = torch.empty(max(1, lib.upf_sgu_blend_forward_workspace_bytes(B, h, w, Hf, Wf)), dtype=torch.uint8, device='cuda')
    ws_b = torch.empty(lib.upf_sgu_blend_backward_workspace_bytes(B, h, w, Hf, Wf), dtype=torch.uint8, device='cuda')
    snap32, snap = A32.snapshot(), A.snapshot()
    code = _lib._DTYPES[dtype]
    _lib.call('upf_sgu_blend_forward', _lib.ptr(f0), _lib.ptr(xo), _lib.ptr(fu), _lib.ptr(fi), _lib.ptr(fm), _lib.ptr(ws_f), B, h, w, Hf, Wf, code, stream())
    _lib.call('upf_sgu_blend_backward', _lib.ptr(f0), _lib.ptr(xo), _lib.ptr(g), _lib.ptr(gi), _lib.ptr(gxo), _lib.ptr(ws_b), B, h, w, Hf, Wf, code, stream())
    torch.cuda.synchronize()
    assert A32.untouched(snap32, fu, fi, fm, gi, gxo), OUTSIDE
    assert dtype == F32 or A.untouched(snap), OUTSIDE
    return dict(flow_up=fu.cpu(), inter_flow=fi.cpu(), inter_mask=fm.cpu()[:, 0], g_init=gi.cpu(), g_xo=gxo.cpu())


def check_ginit(got, c, m32, what):
    want = t_(em.blend_ginit_model(c['g'], c['t'], m32))
    ok = same_bits(got['g_init'], want)
    assert bool(ok.all()), '%s: g_flow_init differs from the fixed-point model at %d of %d elements (first %s)' % (
        what, int((~ok).sum()), ok.numel(), tuple((~ok).nonzero()[0].tolist()))


@pytest.mark.parametrize('shape', em.BLEND_DYADIC, ids=sid)
@pytest.mark.parametrize('dtype', BDT)
def test_blend_dyadic(dtype, shape):
    c = em.blend_case(shape, dtype, 'dyadic')
    what = 'blend dyadic %s %s' % (sid(shape), em.SAMP_NAMES[dtype])
    got = run_blend(c, dtype)
    t64 = em.taps64(c['inter'], shape[1], shape[2])
    fu, _ = em.blend_forward_ref(c['flow_init'], t64, c['m'])
    assert_exact(got['flow_up'], fu, what + ' flow_up')
    assert_exact(got['inter_flow'], c['inter'].astype(np.float64), what + ' inter_flow')
    assert_exact(got['inter_mask'], c['m'], what + ' inter_mask')
    check_ginit(got, c, c['m32'], what)
    full, _ = em.blend_backward_ref(c['flow_init'], c['g'], t64, c['m'])
    full[:, 2] *= c['m'] * (1.0 - c['m'])
    assert_exact(got['g_xo'], full, what + ' g_x_out')


@pytest.mark.parametrize('shape', em.BLEND_GENERAL, ids=sid)
@pytest.mark.parametrize('dtype', BDT)
def test_blend_general(dtype, shape):
    for regime in ('general', 'nonfinite'):
        c = em.blend_case(shape, dtype, regime)
        what = 'blend %s %s %s' % (regime, sid(shape), em.SAMP_NAMES[dtype])
        got = run_blend(c, dtype)
        assert_exact(got['inter_flow'], c['inter'].astype(np.float64), what + ' inter_flow')
        assert_within(got['inter_mask'], c['m'], em.SIGMOID_ULPS * em.U32 * c['m'], what + ' inter_mask')
        fu, b = em.blend_forward_ref(c['flow_init'], c['t'], c['m'])
        assert_within(got['flow_up'], fu, b, what + ' flow_up')
        m32 = got['inter_mask'].numpy()
        check_ginit(got, c, m32, what)
        m = m32.astype(np.float64)
        full, bound = em.blend_backward_ref(c['flow_init'], c['g'], c['t'], m)
        full[:, 2] *= m * (1.0 - m)
        bound[:, 2] = bound[:, 2] * m * (1.0 - m) + 3 * em.U32 * np.abs(full[:, 2])
        assert_within(got['g_xo'], full, bound, what + ' g_x_out')
        if regime == 'nonfinite':
            # a NaN / inf inter flow: every tap is outside, so warped is 0 (not NaN from an outside tap's weight) and flow_up = f m;
            # g_flow_init still receives m g at the pixel itself
            bad = ~np.isfinite(c['inter']).all(1)
            assert bad.sum() == 2
            f, gg = c['flow_init'].astype(np.float64), c['g'].astype(np.float64)
            for n, i, j in np.argwhere(bad):
                assert np.all(np.abs(got['flow_up'][n, :, i, j].double().numpy() - f[n, :, i, j] * m[n, i, j]) <= b[n, :, i, j])
                assert np.all(np.isfinite(got['g_init'][n, :, i, j].numpy()))


@pytest.mark.parametrize('sizes', em.BLEND_FINAL, ids=lambda s: '%s_to_%s' % (sid(s[0]), sid(s[1])))
@pytest.mark.parametrize('dtype', BDT)
def test_blend_final_level(dtype, sizes):
    lo, hi = sizes
    shape = (2,) + hi
    c = em.blend_case(shape, dtype, 'final', lo)
    what = 'blend final %s -> %s %s' % (sid(lo), sid(hi), em.SAMP_NAMES[dtype])
    got = run_blend(c, dtype)
    ok = same_bits(got['inter_flow'], t_(c['inter']))
    assert bool(ok.all()), '%s: inter_flow differs from the fp32 lerp chain at %d elements' % (what, int((~ok).sum()))
    ok = same_bits(got['inter_mask'], t_(c['m32']))
    assert bool(ok.all()), '%s: inter_mask differs from the fp32 lerp of the exact sigmoid values at %d elements' % (what, int((~ok).sum()))
    fu, b = em.blend_forward_ref(c['flow_init'], c['t'], c['m'])
    assert_within(got['flow_up'], fu, b, what + ' flow_up')
    check_ginit(got, c, c['m32'], what)
    ref, bound = em.blend_final_backward_ref(c)
    assert_within(got['g_xo'], ref, bound, what + ' g_x_out (%s)' % em.upsample_bwd_route(lo[0], lo[1], hi[0], hi[1], 3 * shape[0]))


@pytest.mark.parametrize('shape', em.BLEND_FLOW16, ids=sid)
@pytest.mark.parametrize('dtype', DT16)
def test_blend_flow16_forms(dtype, shape):
    """upf_sgu_blend_forward_flow16: flow_up as upf_sgu_blend_forward gives it, and the same value rounded ONCE to the 16-bit type as two
    planes of an NCHW buffer or as one octet [u, v, 0 x 6]."""
    from upflow_pytorch_amd import _lib
    B, H, W = shape
    c = em.blend_case(shape, dtype, 'dyadic')
    fu64, _ = em.blend_forward_ref(c['flow_init'], em.taps64(c['inter'], H, W), c['m'])
    want16 = em.rne(fu64, dtype)
    for c8 in (0, 1):
        A32, A = arena(F32, 2, B * 2 * H * W), arena(dtype, 2, B * 8 * 3 * H * W)
        f0 = A32.block(B, 2, H, W, fill=t_(c['flow_init']))
        fu = A32.block(B, 2, H, W)
        xo = A.block(B, 3, H, W, fill=t_(c['x_out']))
        f16 = A.c8(B, 8, H, W) if c8 else A.nchw(B, 2, H, W)
        snap32, snap = A32.snapshot(), A.snapshot()
        _lib.call('upf_sgu_blend_forward_flow16', _lib.ptr(f0), _lib.ptr(xo), _lib.ptr(fu), _lib.ptr(f16), f16.stride(0), c8, B, H, W, _lib._DTYPES[dtype], stream())
        torch.cuda.synchronize()
        assert A32.untouched(snap32, fu) and A.untouched(snap, f16), OUTSIDE
        what = 'flow16 %s %s %s' % (sid(shape), em.SAMP_NAMES[dtype], 'octet' if c8 else 'planes')
        assert_exact(fu, fu64, what + ' flow_up')
        got16 = f16.cpu()
        if c8:
            assert bool((got16[:, 0, :, :, 2:].view(torch.int16) == 0).all()), what + ': the six padding lanes are not exact zeros'
            got16 = got16[:, 0, :, :, :2].permute(0, 3, 1, 2).contiguous()
        ok = same_bits(got16.contiguous(), want16)
        assert bool(ok.all()), '%s: differs from the fp64 value rounded once at %d elements' % (what, int((~ok).sum()))


# ---- occlusion check -----------------------------------------------------------------------------------------------------------------
def run_occ(c):
    from upflow_pytorch_amd import _lib
    B, H, W = c['shape']
    A32 = arena(F32, 4, B * 2 * H * W)
    ff, fb = A32.block(B, 2, H, W, fill=t_(c['ff'])), A32.block(B, 2, H, W, fill=t_(c['fb']))
    o1, o2 = A32.block(B, 1, H, W), A32.block(B, 1, H, W)
    snap = A32.snapshot()
    _lib.call('upf_occ_check', _lib.ptr(ff), _lib.ptr(fb), _lib.ptr(o1), _lib.ptr(o2), B, H, W, em.OCC_ALPHA[0], em.OCC_ALPHA[1], stream())
    torch.cuda.synchronize()
    assert A32.untouched(snap, o1, o2), OUTSIDE
    return o1.cpu().numpy()[:, 0], o2.cpu().numpy()[:, 0]


@pytest.mark.parametrize('shape', em.OCC_DYADIC + em.OCC_GENERAL, ids=sid)
def test_occ_check(shape):
    dyadic = shape in em.OCC_DYADIC
    c = em.occ_case(shape, dyadic)
    ref = em.occ_ref(c['ff'], c['fb'], *em.OCC_ALPHA)
    gots = run_occ(c)
    for name, got, (want, undecided, _, _) in zip(('occ_fw', 'occ_bw'), gots, ref):
        assert np.all((got == 0) | (got == 1)), name
        bad = (got != want) if dyadic else (got != want) & ~undecided            # (dyadic: the sums are exact, every pixel is compared)
        assert not bad.any(), 'occ %s %s: %d pixels differ from the model (first %s)' % (sid(shape), name, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    if not dyadic and c['nonfinite']:
        B, H, W = shape
        n, ch, i, j = em.nonfinite_places(B, H, W)[0]                                  # the NaN flow: never consistent; outgoing only if
        assert np.isnan(c['ff'][n, ch, i, j]) and not ref[0][2][n, i, j]               # its OTHER coordinate leaves the frame
        assert gots[0][n, i, j] == (0.0 if ref[0][3][n, i, j] else 1.0)


# ---- soft census distance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', em.CENSUS_KINDS)
@pytest.mark.parametrize('R', em.CENSUS_R)
@pytest.mark.parametrize('size', em.CENSUS_SIZES, ids=sid)
def test_census(size, R, kind):
    from upflow_pytorch_amd import _lib
    H, W = size
    B = 2
    g1_np, g2_np, G_np = em.census_case(size, kind)
    ref = em.census_ref(g1_np, g2_np, G_np, R)
    A32 = arena(F32, 10, B * H * W)
    g1, g2, G = (A32.block(B, 1, H, W, fill=t_(a[:, None])) for a in (g1_np, g2_np, G_np))
    dist = A32.block(B, 1, H, W)
    outs = [A32.block(B, 1, H, W) for _ in range(4)]                                   # both, only the first, only the second
    snap = A32.snapshot()
    _lib.call('upf_census_forward', _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(dist), B, H, W, R, stream())
    _lib.call('upf_census_backward', _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(G), _lib.ptr(outs[0]), _lib.ptr(outs[1]), B, H, W, R, stream())
    _lib.call('upf_census_backward', _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(G), _lib.ptr(outs[2]), _lib.ptr(None), B, H, W, R, stream())
    _lib.call('upf_census_backward', _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(G), _lib.ptr(None), _lib.ptr(outs[3]), B, H, W, R, stream())
    torch.cuda.synchronize()
    assert A32.untouched(snap, dist, *outs), OUTSIDE
    what = 'census %s R %d %s' % (sid(size), R, kind)
    assert_within(dist[:, 0], ref['dist'], ref['b_dist'], what + ' dist')
    for out, key in zip(outs, ('gg1', 'gg2', 'gg1', 'gg2')):
        assert_within(out[:, 0], ref[key], ref['b_' + key], '%s %s' % (what, key))
    if kind == 'equal':
        assert float(dist.abs().max()) == 0 and all(float(o.abs().max()) == 0 for o in outs), what + ': equal images must give exact zeros'
