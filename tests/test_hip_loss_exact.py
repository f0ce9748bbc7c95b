"""The four operators of the default loss path on the GPU — boundary warp and abs_robust (csrc/loss.hip), first-order edge-aware
smoothness (csrc/loss.hip, loss_common.hpp), the fused distillation term (csrc/sgu_blend.hip msd_*) — against references that take
nothing from the code under test (tests/_exact_model.py; its conditions are checked without a GPU in tests/test_exact_model_cpu.py):

  boundary warp   operands on grids where every weight, product and partial sum is exact in fp32: bit equality with the fp64
                  restatement of the reference, forward and flow gradient, at the frame edge, on integer positions, far outside.
  smooth_edge1    a position-constant image (every edge weight exp(-0) = 1) and pred on a grid of 1/4: every workgroup's pair of
                  partial sums equals the exact one; gradients and textured images under the rule below.
  abs_robust      value and both gradients under the rule below; exact zeros for an all-zero mask and for x == y.
  msd_upup        value and every level's gradient under the rule below against the torch composition in fp64, on every route
                  of the backward kernel; exact zeros where a level equals the label; the refusals.

The rule is the project's (_lossvar.check): error against fp64 over max |fp64| <= max(3e-6, 2.5 x the error of the fp32 torch
composition on the same inputs)."""
import pytest
import torch

import _exact_model as em
import _lossvar as lv

pytestmark = pytest.mark.gpu


def _ops():
    from upflow_pytorch_amd import ops
    return ops


def _oracle():
    from oracle import ops as oracle_ops
    return oracle_ops


def _eval(fn, inputs, diff, dtype, device):
    """fn(*inputs in dtype on device) -> scalar; -> (value, gradients of the inputs whose index is in diff)."""
    xs = [None if t is None else t.to(device=device, dtype=dtype).clone().requires_grad_(i in diff) for i, t in enumerate(inputs)]
    v = fn(*xs)
    grads = torch.autograd.grad(v, [xs[i] for i in diff]) if diff else []
    return v.detach(), [g.detach() for g in grads]


def _compare(name, native, spelled, inputs, diff, names, zeros=False):
    """native(*cuda fp32) against spelled(*cpu) in fp64, bound from spelled in fp32; two native runs give identical bits; zeros: where
    the fp64 gradient is exactly 0 the native one is too.  -> the native (value, gradients)."""
    v, gs = _eval(native, inputs, diff, torch.float32, 'cuda')
    v2, gs2 = _eval(native, inputs, diff, torch.float32, 'cuda')
    assert torch.equal(v, v2) and all(torch.equal(a, b) for a, b in zip(gs, gs2)), name + ': two runs differ'
    v32, gs32 = _eval(spelled, inputs, diff, torch.float32, 'cpu')
    v64, gs64 = _eval(spelled, inputs, diff, torch.float64, 'cpu')
    lv.check(name + ' value', v, v32, v64)
    for n, a, a32, a64 in zip(names, gs, gs32, gs64):
        assert a.shape == a64.shape
        lv.check('%s grad %s' % (name, n), a, a32, a64)
        if zeros:
            z = a64 == 0
            print('%-40s %d of %d reference gradients are exactly 0' % (name, int(z.sum()), z.numel()))
            assert not a.cpu()[z].any(), '%s grad %s: non-zero where the reference is exactly 0' % (name, n)
    return v, gs


# ---- boundary warp -----------------------------------------------------------------------------------------------------------------------
def _bwarp_run(c, channels=None):
    image, go = c['image'], c['grad_out']
    if channels is not None:
        image, go = image[:, channels].contiguous(), go[:, channels].contiguous()
    flow = c['flow'].cuda().requires_grad_(True)
    out = _ops().boundary_warp(image.cuda(), flow, c['start'].cuda())
    (gf,) = torch.autograd.grad(out, flow, go.cuda())
    return out.detach().cpu(), gf.cpu()


def _same(what, got, want):
    bad = got != want
    if bad.any():
        at = tuple(int(v) for v in bad.nonzero()[0])
        print('%s: %d of %d differ, first at %s: got %r, want %r' % (what, int(bad.sum()), bad.numel(), at, float(got[at]), float(want[at])))
    assert torch.equal(got, want), what


@pytest.mark.parametrize('name', em.BWARP_CASES)
def test_boundary_warp_equals_the_fp64_reference_bit_for_bit(name):
    c = em.bwarp_case(name)
    em.bwarp_guard(c)
    want_out, want_gf = em.bwarp_expected(c)
    out, gf = _bwarp_run(c)
    _same('boundary warp %s output' % name, out, want_out)
    _same('boundary warp %s flow gradient' % name, gf, want_gf)
    out_b, gf_b = _bwarp_run(c)
    assert torch.equal(out, out_b) and torch.equal(gf, gf_b), 'two runs differ'
    # another channel count, the channels permuted: each channel's output is that of the channel it came from
    C = c['image'].shape[1]
    idx = [(C - 1 - k) % C for k in range(C + 2)]
    want_out2, want_gf2 = em.bwarp_expected(c, idx)
    out2, gf2 = _bwarp_run(c, idx)
    _same('boundary warp %s output, %d channels' % (name, C + 2), out2, want_out2)
    _same('boundary warp %s flow gradient, %d channels' % (name, C + 2), gf2, want_gf2)
    assert torch.equal(out2, out[:, idx])


# ---- first-order edge-aware smoothness ---------------------------------------------------------------------------------------------------
def _smooth1_partials(img, pred):
    """upf_smooth_edge1_forward launched the way ops._partial_sums launches it -> the [nblocks, 2] partial sums."""
    from upflow_pytorch_amd import _lib
    B, Ci, H, W = img.shape
    img, pred = img.cuda().contiguous(), pred.cuda().contiguous()
    partials = torch.full((_lib.lib().upf_loss_partials(B * H * W), 2), float('nan'), dtype=torch.float32, device=img.device)
    _lib.launch(img.device, 'upf_smooth_edge1_forward', _lib.ptr(img), _lib.ptr(pred), _lib.ptr(partials), B, Ci, pred.shape[1], H, W)
    return partials.cpu()


@pytest.mark.parametrize('shape', em.SMOOTH1_SHAPES)
def test_smooth_edge1_partial_sums_are_exact(shape):
    """A position-constant image, pred on a grid of 1/4: every workgroup's pair equals the model's, which holds only if expf(-0.f) is
    exactly 1 on the device and no pixel is dropped or taken twice (the last shape: one pixel past 1024 x 256)."""
    c = em.smooth1_exact_case(shape)
    got = _smooth1_partials(c['img'], c['pred'])
    assert tuple(got.shape) == (c['nblocks'], 2)
    bad = got.double() != c['partials']
    print('smooth_edge1 %s: %d workgroups, %d partial sums differ; totals %r, exact %r'
          % (shape, c['nblocks'], int(bad.sum()), tuple(got.double().sum(0).tolist()), c['total']))
    assert not bad.any(), (shape, bad.nonzero()[:4].tolist())
    assert tuple(got.double().sum(0).tolist()) == c['total']
    again = _smooth1_partials(c['img'], c['pred'])
    assert torch.equal(got, again)


@pytest.mark.parametrize('shape', em.SMOOTH1_SHAPES)
def test_smooth_edge1_gradient_on_the_exact_cases(shape):
    c = em.smooth1_exact_case(shape)
    _compare('edge1 exact %s' % (shape,), _ops().smooth_edge1, _oracle().smooth_edge1, [c['img'], c['pred']], [1], ['pred'], zeros=True)


@pytest.mark.parametrize('shape', em.SMOOTH1_SHAPES)
def test_smooth_edge1_gradient_piecewise_constant(shape):
    """pred constant on 4 x 4 cells under a textured image: sign(0) = 0 inside a cell, exactly."""
    B, Ci, H, W = shape
    img, pc = lv.textured(shape, 41), lv.piecewise_constant((B, 2, H, W), 42)
    _, (g,) = _compare('edge1 piecewise constant %s' % (shape,), _ops().smooth_edge1, _oracle().smooth_edge1, [img, pc], [1], ['pred'], zeros=True)
    if H >= 8 and W >= 8:
        assert not g[:, :, 1:3, 1:3].any() and g.any()


@pytest.mark.parametrize('shape', em.SMOOTH1_SHAPES[:4])
def test_smooth_edge1_textured(shape):
    B, Ci, H, W = shape
    img, pred = lv.textured(shape, 43), lv.flow_inputs((B, 2, H, W), 44)
    _compare('edge1 textured %s' % (shape,), _ops().smooth_edge1, _oracle().smooth_edge1, [img, pred], [1], ['pred'])


# ---- abs_robust --------------------------------------------------------------------------------------------------------------------------
ROBUST_SHAPES = [(1, 1, 1, 1), (1, 3, 1, 255), (1, 3, 1, 256), (1, 3, 1, 257), (5, 3, 10, 10), (2, 1, 37, 45), (1, 2, 545, 481)]


def _robust_inputs(shape, occ_mode):
    B, C, H, W = shape
    g = lv.gen(em.seed_of('robust', shape))
    x = torch.rand(shape, generator=g) - 0.45
    y = x + 0.1 * torch.randn(shape, generator=g)
    occ = {'none': None, 'binary': lv.binary_mask(shape, 51), 'zero': torch.zeros(B, 1, H, W)}[occ_mode]
    return x, y, occ


def _robust_pair(occ):
    def native(x, y):
        return _ops().robust_loss_sums(x, y, None if occ is None else occ.cuda())[0]

    def spelled(x, y):
        return _oracle().robust_loss_sums(x, y, None if occ is None else occ.to(x.dtype))[0]
    return native, spelled


@pytest.mark.parametrize('occ_mode', ['none', 'binary', 'zero'])
@pytest.mark.parametrize('shape', ROBUST_SHAPES)
def test_robust_loss_sums(shape, occ_mode):
    B, C, H, W = shape
    x, y, occ = _robust_inputs(shape, occ_mode)
    native, spelled = _robust_pair(occ)
    v, (gx, gy) = _compare('abs_robust occ %s %s' % (occ_mode, shape), native, spelled, [x, y], [0, 1], ['x', 'y'])
    _, so = _ops().robust_loss_sums(x.cuda(), y.cuda(), None if occ is None else occ.cuda())
    assert float(so) == (float(B * H * W) if occ is None else float(occ.sum()))          # one per pixel, exactly (0 / 1 values)
    assert torch.equal(gx, -gy)
    if occ_mode == 'zero':
        assert float(v) == 0.0 and float(so) == 0.0 and not gx.any() and not gy.any()
    elif occ is None or occ.any():
        assert gx.any()


@pytest.mark.parametrize('occ_mode', ['none', 'binary'])
@pytest.mark.parametrize('shape', ROBUST_SHAPES)
def test_robust_loss_sums_identical_operands(shape, occ_mode):
    """x == y bit for bit: sign(0) = 0, both gradients are exactly 0; the value (eps^q per counted element) passes the rule."""
    x, _, occ = _robust_inputs(shape, occ_mode)
    native, spelled = _robust_pair(occ)
    v, (gx, gy) = _compare('abs_robust x == y occ %s %s' % (occ_mode, shape), native, spelled, [x, x.clone()], [0, 1], ['x', 'y'])
    assert not gx.any() and not gy.any() and (float(v) > 0) == (occ is None or bool(occ.any()))


# ---- the distillation term ---------------------------------------------------------------------------------------------------------------
def _msd_pair(y, occ):
    yc, oc = y.cuda(), None if occ is None else occ.cuda()

    def native(*xs):
        assert _ops().msd_upup_supported(yc, xs)
        return _ops().msd_upup_loss(list(xs), yc, oc, em.MSD_WEIGHT)

    def spelled(*xs):
        return em.msd_ref(list(xs), y.to(xs[0].dtype), None if occ is None else occ.to(xs[0].dtype), em.MSD_WEIGHT)
    return native, spelled


def _msd_names(levels):
    return ['level %dx%d' % tuple(x.shape[2:]) for x in levels]


@pytest.mark.parametrize('name,B,masked', em.msd_cases())
def test_msd_upup(name, B, masked):
    levels, y, occ = em.msd_case(name, B, masked)
    route = em.msd_route([tuple(x.shape[2:]) for x in levels], y.shape[2], y.shape[3], B)
    assert route is not None and all(r['span'] <= em.MSD_BAND_COLS for r in route)
    native, spelled = _msd_pair(y, occ)
    _compare('msd %s B=%d %s' % (name, B, 'masked' if masked else 'mean'), native, spelled, levels, list(range(len(levels))), _msd_names(levels))


@pytest.mark.parametrize('B,masked', em.MSD_BATCHES)
def test_msd_upup_level_equal_to_the_label(B, masked):
    """The (9, 17) level of the dyadic case equal to the label bit for bit: that level's gradient is exactly 0 (the resize to its own
    size is the identity, sign(0) = 0); the other levels still pass the rule."""
    levels, y, occ = em.msd_case('dyadic_3', B, masked)
    assert tuple(levels[-1].shape) == tuple(y.shape)
    levels = list(levels[:-1]) + [y.clone()]
    native, spelled = _msd_pair(y, occ)
    _, gs = _compare('msd level == label B=%d' % B, native, spelled, levels, [0, 1, 2], _msd_names(levels), zeros=True)
    assert not gs[-1].any() and gs[0].any() and gs[1].any()


def test_msd_upup_refusals():
    """msd_upup_supported stops at a resize ratio of 250; the entry point itself refuses, before any launch, a ratio whose strip
    width would be 0 (its output and partial-sum buffers keep their contents)."""
    from upflow_pytorch_amd import _lib
    ops = _ops()
    lvl = torch.zeros(1, 2, 2, 2, device='cuda')
    assert ops.msd_upup_supported(torch.zeros(1, 2, 6, 251, device='cuda'), [lvl])
    assert not ops.msd_upup_supported(torch.zeros(1, 2, 6, 252, device='cuda'), [lvl])
    H, W = 6, 254
    assert em.msd_route([(2, 2)], H, W) is None and em.msd_route([(2, 2)], H, W - 1) is not None
    y = torch.zeros(1, 2, H, W, device='cuda')
    with pytest.raises(ops.UpflowHipError):
        ops.msd_upup_loss([lvl], y)
    partials = torch.full((_lib.lib().upf_msd_upup_partials(1, H, W), 7), -7.0, device='cuda')
    out2 = torch.full((2,), -7.0, device='cuda')
    xp, hs, ws = (_lib._vp * 1)(lvl.data_ptr()), (_lib._c.c_int * 1)(2), (_lib._c.c_int * 1)(2)
    with torch.cuda.device(y.device):
        rc = _lib.lib().upf_msd_upup_forward(xp, hs, ws, 1, _lib.ptr(y), _lib.ptr(None), _lib.ptr(partials), _lib.ptr(out2), 1, H, W,
                                             1.0, 0.01, 0.4, _lib.stream_ptr(y.device))
        glv = torch.full_like(lvl, -7.0)
        gp = (_lib._vp * 1)(glv.data_ptr())
        g = torch.ones(1, device='cuda')
        rc_b = _lib.lib().upf_msd_upup_backward(xp, gp, hs, ws, 1, _lib.ptr(y), _lib.ptr(None), _lib.ptr(g), _lib.ptr(out2), 1, H, W,
                                                1.0, 0.01, 0.4, _lib.stream_ptr(y.device))
    torch.cuda.synchronize()
    assert rc != 0 and rc_b != 0
    assert bool((partials == -7.0).all()) and bool((out2 == -7.0).all()) and bool((glv == -7.0).all())
