"""The native loss variants (csrc/loss_variants.hip) on the GPU: every operator against the fp64 torch composition and against the
reference's fixtures under one error rule (_lossvar.check: error against fp64 over max |fp64| <= max(3e-6, 2.5 x the error of the
fp32 torch composition on the same inputs), then the training step with the variants switched on, native against the torch
spelling (`net._no_native_loss_variants = True`)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _lossvar as lv
import _weights
from conftest import load_golden

pytestmark = pytest.mark.gpu

# the operator's minimum, one-tile strips, one pixel row / column of windows more than a tile, ragged with several tiles and a batch stride
SHAPES3 = [(2, 3, 3, 3), (2, 3, 3, 40), (2, 3, 40, 3), (1, 1, 5, 5), (2, 3, 37, 45)]
BIG = (4, 3, 256, 832)


def _nt():
    from upflow_pytorch_amd.model.upflow import network_tools
    return network_tools


def _ops():
    from upflow_pytorch_amd import ops
    return ops


def _lossfn():
    from upflow_pytorch_amd.utils.loss import loss_functions
    return loss_functions


def _eval(fn, inputs, diff, dtype, device):
    """fn(*inputs in dtype on device) -> scalar; -> (value, gradients of the inputs whose index is in diff)."""
    xs = [None if t is None else t.to(device=device, dtype=dtype).clone().requires_grad_(i in diff) for i, t in enumerate(inputs)]
    v = fn(*xs)
    grads = torch.autograd.grad(v, [xs[i] for i in diff]) if diff else []
    return v.detach(), [g.detach() for g in grads]


def _compare(name, native, spelled, inputs, diff, names, grads=True):
    """native(*cuda fp32) against spelled(*cpu) in fp64, bound from spelled in fp32; two native runs give identical bits."""
    diff = diff if grads else []
    v, gs = _eval(native, inputs, diff, torch.float32, 'cuda')
    v2, gs2 = _eval(native, inputs, diff, torch.float32, 'cuda')
    assert torch.equal(v, v2) and all(torch.equal(a, b) for a, b in zip(gs, gs2)), name + ': two runs differ'
    v32, gs32 = _eval(spelled, inputs, diff, torch.float32, 'cpu')
    v64, gs64 = _eval(spelled, inputs, diff, torch.float64, 'cpu')
    lv.check(name + ' value', v, v32, v64)
    for n, a, a32, a64 in zip(names, gs, gs32, gs64):
        assert a.shape == a64.shape
        lv.check('%s grad %s' % (name, n), a, a32, a64)


def _partials(n):
    from upflow_pytorch_amd import _lib
    return _lib.lib().upf_loss_partials(n)


# ---- A: second-order edge-aware smoothness -----------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES3)
def test_smooth_edge2(shape):
    B, C, H, W = shape
    img, pred = lv.textured(shape, 1), lv.flow_inputs((B, 2, H, W), 2)
    if shape == SHAPES3[-1]:
        assert _partials(B * H * W) > 1
    _compare('edge2 %s' % (shape,), _ops().smooth_edge2, _nt()._edge_aware_smoothness_order2_torch, [img, pred], [1], ['pred'])


def test_smooth_edge2_piecewise_constant_and_full_size():
    shape = (2, 3, 37, 45)
    img, pc = lv.textured(shape, 3), lv.piecewise_constant((2, 2, 37, 45), 4)
    _compare('edge2 piecewise constant', _ops().smooth_edge2, _nt()._edge_aware_smoothness_order2_torch, [img, pc], [1], ['pred'])
    img, pred = lv.textured(BIG, 5), lv.flow_inputs((4, 2, 256, 832), 6)
    _compare('edge2 full size', _ops().smooth_edge2, _nt()._edge_aware_smoothness_order2_torch, [img, pred], [1], ['pred'], grads=False)


# ---- B: delta smoothness -------------------------------------------------------------------------------------------------------
# (first order from its 2x2 minimum; the second order from 3x3)
@pytest.mark.parametrize('shape,second', [((2, 2, 2, 2), False)] + [(s, o) for s in SHAPES3 for o in (False, True)])
def test_smooth_delta(shape, second):
    flow = lv.flow_inputs(shape, 7)
    if shape == SHAPES3[-1]:
        assert _partials(flow.numel()) > 1
    _compare('delta %s order %d' % (shape, 1 + second), lambda f: _ops().smooth_delta(f, second),
             lambda f: _lossfn()._flow_smooth_delta_torch(f, second), [flow], [0], ['flow'])


@pytest.mark.parametrize('second', [False, True])
def test_smooth_delta_piecewise_constant_and_full_size(second):
    pc = lv.piecewise_constant((2, 2, 37, 45), 8)
    _compare('delta piecewise constant', lambda f: _ops().smooth_delta(f, second), lambda f: _lossfn()._flow_smooth_delta_torch(f, second),
             [pc], [0], ['flow'])
    flow = lv.flow_inputs((4, 2, 256, 832), 9)
    _compare('delta full size', lambda f: _ops().smooth_delta(f, second), lambda f: _lossfn()._flow_smooth_delta_torch(f, second),
             [flow], [0], ['flow'], grads=False)


# ---- C: point-wise photometric kinds --------------------------------------------------------------------------------------------
def _pointwise_pair(kind, occ):
    """(native, spelled) forms of photo_loss_multi_type with this kind; occ None: the plain mean."""
    def native(x, y):
        return _nt().photo_loss_multi_type(x, y, torch.ones_like(x[:, :1]) if occ is None else occ.cuda(), kind, 0.4, occ is not None)

    def spelled(x, y):
        return _nt()._photo_loss_multi_type_torch(x, y, torch.ones_like(x[:, :1]) if occ is None else occ.to(x.dtype), kind, 0.4, occ is not None)
    return native, spelled


@pytest.mark.parametrize('kind', ['charbonnier', 'L1'])
@pytest.mark.parametrize('occ_mode', ['none', 'binary', 'zero'])
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (1, 1, 5, 5), (2, 3, 37, 45)])
def test_pointwise_loss(shape, occ_mode, kind):
    B, C, H, W = shape
    x, y = lv.textured(shape, 11), lv.textured(shape, 12)
    occ = {'none': None, 'binary': lv.binary_mask(shape, 13), 'zero': torch.zeros(B, 1, H, W)}[occ_mode]
    if shape == (2, 3, 37, 45):
        assert _partials(B * H * W) > 1
    native, spelled = _pointwise_pair(kind, occ)
    _compare('%s occ %s %s' % (kind, occ_mode, shape), native, spelled, [x, y], [0, 1], ['x', 'y'])
    if occ is not None:
        s, so = _ops().pointwise_loss_sums(x.cuda(), y.cuda(), occ.cuda(), kind, 0.4)
        assert float(so) == float(occ.sum())               # the mask is summed once per pixel, exactly (0 / 1 values)
        if occ_mode == 'zero':
            assert float(s) == 0.0


@pytest.mark.parametrize('kind', ['charbonnier', 'L1'])
def test_pointwise_loss_full_size(kind):
    x, y, occ = lv.textured(BIG, 14), lv.textured(BIG, 15), lv.binary_mask(BIG, 16)
    native, spelled = _pointwise_pair(kind, occ)
    _compare(kind + ' full size', native, spelled, [x, y], [0, 1], ['x', 'y'], grads=False)


# ---- D: weighted SSIM ---------------------------------------------------------------------------------------------------------------
def _preclamp64(x, y, w, c2=9e-6, eps=0.01):
    x, y, w = x.double(), y.double(), w.double()
    pool = lambda z: F.avg_pool2d(z, (3, 3), (1, 1))
    inv = 1.0 / (pool(w) + eps)
    wp = lambda z: pool(z * (w + eps)) * inv
    mx, my = wp(x), wp(y)
    sx, sy, sxy = wp(x * x) - mx * mx, wp(y * y) - my * my, wp(x * y) - mx * my
    return (1 - (2 * sxy + c2) / (sx + sy + c2)) / 2


def _ssim_case(name, x, y, w, grads=True, away_from_clamp=True):
    nt, ops = _nt(), _ops()
    if away_from_clamp:
        v = _preclamp64(x, y, w)
        print('%s: fp64 pre-clamp value in [%.3g, %.3g]' % (name, float(v.min()), float(v.max())))
        assert float(v.min()) >= 1e-3 and float(v.max()) <= 1 - 1e-3, 'the inputs put a window on a clamp bound'
    B, C, H, W = x.shape
    # the map and the pooled weight, element by element
    m, wa = ops.weighted_ssim(x.cuda(), y.cuda(), w.cuda())
    m_b, wa_b = ops.weighted_ssim(x.cuda(), y.cuda(), w.cuda())
    assert torch.equal(m, m_b) and torch.equal(wa, wa_b)
    assert m.shape == (B, C, H - 2, W - 2) and wa.shape == (B, 1, H - 2, W - 2)
    m32, wa32 = nt._weighted_ssim_torch(x, y, w)
    m64, wa64 = nt._weighted_ssim_torch(x.double(), y.double(), w.double())
    lv.check(name + ' map', m, m32, m64)
    lv.check(name + ' w_avg', wa, wa32, wa64)
    G = torch.randn(B, C, H - 2, W - 2, generator=lv.gen(99))
    wc = w.cuda()
    _compare(name + ' map under a random upstream', lambda a, b: (ops.weighted_ssim(a, b, wc)[0] * G.cuda()).sum(),
             lambda a, b: (nt._weighted_ssim_torch(a, b, w.to(a.dtype))[0] * G.to(a.dtype)).sum(), [x, y], [0, 1], ['x', 'y'], grads=grads)
    for use_occ in (True, False):
        _compare('%s photometric form, occ %d' % (name, use_occ), lambda a, b: nt.photo_loss_multi_type(a, b, wc, 'SSIM', 0.4, use_occ),
                 lambda a, b: nt._photo_loss_multi_type_torch(a, b, w.to(a.dtype), 'SSIM', 0.4, use_occ), [x, y], [0, 1], ['x', 'y'], grads=grads)


@pytest.mark.parametrize('shape', SHAPES3)
def test_weighted_ssim(shape):
    x, y, w = lv.ssim_inputs(shape, 21)
    if shape == SHAPES3[-1]:
        assert _partials(shape[0] * (shape[2] - 2) * (shape[3] - 2)) > 1
    _ssim_case('ssim %s' % (shape,), x, y, w)


def test_weighted_ssim_full_size():
    x, y, w = lv.ssim_inputs(BIG, 22)
    # value only: the clamp is continuous, so a window near a bound cannot loosen a VALUE comparison; among 2.5 M windows the
    # recipe's smallest fp64 pre-clamp value is 4e-4, below the 1e-3 margin the gradient cases assert
    _ssim_case('ssim full size', x, y, w, grads=False, away_from_clamp=False)


@pytest.mark.parametrize('weight', ['zeros', 'ones'])
def test_weighted_ssim_constant_weight(weight):
    x, y, _ = lv.ssim_inputs((2, 3, 37, 45), 23)
    w = torch.zeros(2, 1, 37, 45) if weight == 'zeros' else torch.ones(2, 1, 37, 45)
    _ssim_case('ssim weight ' + weight, x, y, w)


def test_weighted_ssim_identical_images():
    """x == y bit for bit: the map is exactly 0 (the lower clamp bound, where the gradient passes) and the gradient is finite."""
    ops = _ops()
    x, _, w = lv.ssim_inputs((2, 3, 37, 45), 24)
    xc, yc = x.cuda().requires_grad_(True), x.clone().cuda().requires_grad_(True)
    m, _ = ops.weighted_ssim(xc, yc, w.cuda())
    assert float(m.abs().max()) == 0.0
    gx, gy = torch.autograd.grad(m.sum(), [xc, yc])
    assert torch.isfinite(gx).all() and torch.isfinite(gy).all()
    s_lw, s_w, s_l = ops.ssim_loss_sums(xc, yc, w.cuda())
    assert float(s_lw) == 0.0 and float(s_l) == 0.0 and float(s_w) > 0


# ---- fixtures recorded from the reference's own functions -----------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(lv.FIXTURE_SHAPES)))
def test_against_reference_fixtures(i):
    nt, ops = _nt(), _ops()

    def run(key, fn, inputs, diff, names, g):
        v, gs = _eval(fn, inputs, diff, torch.float32, 'cuda')
        lv.check('%s value' % key, v, g['%s_val32' % key], g['%s_val64' % key])
        for n, a in zip(names, gs):
            lv.check('%s grad %s' % (key, n), a, g['%s_g%s32' % (key, n)], g['%s_g%s64' % (key, n)])
    g = load_golden('lossvar_edge2_%d' % i)
    run('edge2', nt.edge_aware_smoothness_order2, [g['img'], g['pred']], [1], ['pred'], g)
    g = load_golden('lossvar_delta_%d' % i)
    for name in ('flow', 'pc'):
        for order in (1, 2):
            run('%s_o%d' % (name, order), lambda a, o=order: nt.flow_smooth_delta(a, o == 2), [g[name]], [0], ['flow'], g)
    g = load_golden('lossvar_pointwise_%d' % i)
    B, _, H, W = g['x'].shape
    for kind in ('charbonnier', 'L1'):
        for oname, occ in (('none', None), ('binary', g['occ_binary']), ('zero', torch.zeros(B, 1, H, W))):
            o = (torch.ones(B, 1, H, W) if occ is None else occ).cuda()
            run('%s_%s' % (kind, oname), lambda a, b, kind=kind, o=o, u=occ is not None: nt.photo_loss_multi_type(a, b, o, kind, 0.4, u),
                [g['x'], g['y']], [0, 1], ['x', 'y'], g)
    g = load_golden('lossvar_ssim_%d' % i)
    w, G = g['weight'].cuda(), g['G'].cuda()
    m, wa = nt.weighted_ssim(g['x'].cuda(), g['y'].cuda(), w)
    lv.check('fixture map', m, g['map32'], g['map64'])
    lv.check('fixture w_avg', wa, g['wavg32'], g['wavg64'])
    run('map', lambda a, b: (nt.weighted_ssim(a, b, w)[0] * G).sum(), [g['x'], g['y']], [0, 1], ['x', 'y'], g)
    for use_occ in (True, False):
        run('photo_occ%d' % use_occ, lambda a, b, u=use_occ: nt.photo_loss_multi_type(a, b, w, 'SSIM', 0.4, u), [g['x'], g['y']], [0, 1], ['x', 'y'], g)


# ---- routing ---------------------------------------------------------------------------------------------------------------------------------
def test_native_path_rejects_or_falls_back(monkeypatch):
    """The operators reject a non-contiguous, non-fp32 or too-small operand; the model-level functions make a GPU fp32 operand
    contiguous and take the torch spelling for what the kernels do not cover."""
    nt, ops = _nt(), _ops()
    Err = ops.UpflowHipError
    x, y, w = [t.cuda() for t in lv.ssim_inputs((2, 3, 12, 20), 31)]
    flow = lv.flow_inputs((2, 2, 12, 20), 32).cuda()
    xt, ft = x.transpose(2, 3), flow.transpose(2, 3)            # [.., 20, 12] views, not contiguous
    with pytest.raises(Err):
        ops.smooth_edge2(xt, ft)
    with pytest.raises(Err):
        ops.smooth_delta(ft)
    with pytest.raises(Err):
        ops.pointwise_loss_sums(xt, xt.contiguous(), None, 'L1', 0.4)
    with pytest.raises(Err):
        ops.weighted_ssim(xt, xt.contiguous(), w.transpose(2, 3).contiguous())
    with pytest.raises(Err):
        ops.smooth_edge2(x[..., :2], flow[..., :2].contiguous())
    with pytest.raises(Err):
        ops.smooth_delta(flow[:, :, :2, :2].contiguous(), True)
    with pytest.raises(Err):
        ops.smooth_delta(flow[:, :, :1].contiguous(), False)
    with pytest.raises(Err):
        ops.ssim_loss_sums(x[:, :, :2].contiguous(), y[:, :, :2].contiguous(), w[:, :, :2].contiguous())
    with pytest.raises(Err):
        ops.smooth_delta(flow.double())
    with pytest.raises(Err):
        ops.pointwise_loss_sums(x, y, None, 'abs_robust', 0.4)
    with pytest.raises(Err):
        ops.weighted_ssim(x, y, w.clone().requires_grad_(True))
    # model level: non-contiguous operands give the bits of their contiguous copies
    assert torch.equal(nt.edge_aware_smoothness_order2(xt, ft), ops.smooth_edge2(xt.contiguous(), ft.contiguous()))
    assert torch.equal(nt.flow_smooth_delta(ft, True), ops.smooth_delta(ft.contiguous(), True))
    # model level: what the kernels do not cover is the torch spelling (no native call)
    calls = []
    for name in ('smooth_edge2', 'smooth_delta', 'pointwise_loss_sums', 'weighted_ssim', 'ssim_loss_sums'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    assert nt.flow_smooth_delta(flow.double(), True).dtype == torch.float64
    assert nt.edge_aware_smoothness_order2(x.half(), flow.half()).dtype == torch.float16
    assert nt.flow_smooth_delta(flow[:, :, :2, :2], True).shape == ()           # (2x2 at the second order: too small)
    m, _ = nt.weighted_ssim(x, y, w, c1=1e-4)                                   # finite c1
    assert m.shape == (2, 3, 10, 18)
    wg = w.clone().requires_grad_(True)
    m, _ = nt.weighted_ssim(x, y, wg)                                           # a weight that wants a gradient
    assert m.requires_grad
    assert nt.photo_loss_multi_type(x.double(), y.double(), w.double(), 'charbonnier').dtype == torch.float64
    assert nt.flow_smooth_delta(flow, True, native=False).shape == ()
    assert calls == []


# ---- the training step ------------------------------------------------------------------------------------------------------------------------
FLAGS = {'if_norm_before_cost_volume': True, 'norm_moments_across_channels': False,
         'norm_moments_across_images': False, 'if_sgu_upsample': True, 'warp_mask_mode': 'robust'}
VARIANTS = {'ssim_occ_order2': {'photo_loss_type': 'SSIM', 'photo_loss_use_occ': True, 'smooth_order_2_weight': 1},
            'delta_charbonnier': {'smooth_type': 'delta', 'photo_loss_type': 'charbonnier'}}


def _net(variant, extra=None):
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    conf = UPFlow_net.config()
    d = dict(FLAGS)
    d.update(_weights.TRAIN_FLAGS)
    d.update(VARIANTS[variant])
    d.update(extra or {})
    conf.update(d, verbose=False)
    net = conf()
    net.load_state_dict(_weights.make_state_dict(0, head_scale=0.1))
    return net.cuda().train()


def _step(net, batch):
    out = net(batch)
    terms = {k: out[k].mean() for k in ('photo_loss', 'smooth_loss', 'census_loss', 'msd_loss')}
    sum(terms.values()).backward()
    return {k: float(v) for k, v in terms.items()}, {n: p.grad.detach().clone() for n, p in net.named_parameters()}


@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_train_step_native_matches_the_torch_spelling(variant, monkeypatch):
    """train_128x192 inputs and weights, fp32 mode: loss terms within 2e-4 relative, per-parameter gradient norms within 2e-3,
    cosines >= 0.9999 (test_hip_train.py's fp32 bars); no avg_pool2d call on the native path, some on the fallback."""
    batch = {k: v.cuda() for k, v in _weights.make_train_batch().items()}
    batch['if_loss'] = True
    pools = []
    real_pool = F.avg_pool2d

    def counting_pool(*a, **k):
        pools.append(1)
        return real_pool(*a, **k)
    monkeypatch.setattr(F, 'avg_pool2d', counting_pool)
    res = {}
    for native in (True, False):
        net = _net(variant)
        net._no_native_loss_variants = not native
        del pools[:]
        res[native] = _step(net, batch) + (len(pools),)
    (t1, g1, n1), (t0, g0, n0) = res[True], res[False]
    print(variant, 'avg_pool2d calls: native %d, torch spelling %d' % (n1, n0))
    assert n1 == 0
    if VARIANTS[variant].get('photo_loss_type') == 'SSIM':
        assert n0 > 0
    for k in t1:
        print(k, t1[k], t0[k])
        assert np.isfinite(t1[k]) and abs(t1[k] - t0[k]) <= 2e-4 * abs(t0[k]), (k, t1[k], t0[k])
    names = sorted(g1)
    got, want = np.array([float(g1[n].norm()) for n in names]), np.array([float(g0[n].norm()) for n in names])
    rel = np.abs(got - want) / np.maximum(want, 1e-3)
    cos = np.array([float((g1[n].double() * g0[n].double()).sum() / (g1[n].double().norm() * g0[n].double().norm()).clamp_min(1e-300)) for n in names])
    print('max rel grad-norm difference %.3g (%s), min cosine %.7f (%s)' % (rel.max(), names[int(rel.argmax())], cos.min(), names[int(cos.argmin())]))
    assert (got > 0).all() and rel.max() <= 2e-3 and cos.min() >= 0.9999


@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_trainer_captures_the_step_with_the_variants(variant):
    """The step with the variants is captured as one hipGraph, and two replayed steps leave the parameters bit-identical to two
    eager steps.  Both trainers are built with graph=True (the capturable Adam — an eager trainer's Adam is another floating-point
    spelling of the update, test_hip_train.py) and differ only in when they capture: after the first step, or never.  The
    convolutions are the bit-reproducible fp32 ones (fp32_train_conv='hip_x3'); PyTorch-ROCm's gradient kernels are not
    reproducible run to run at this size."""
    from upflow_pytorch_amd.train import Trainer
    batch = {k: v.cuda() for k, v in _weights.make_train_batch().items()}
    ends = {}
    for graphed in (True, False):
        tr = Trainer(_net(variant, {'fp32_train_conv': 'hip_x3'}), lr=1e-4, device=torch.device('cuda', 0), distributed=False, graph=True)
        tr.graph_warmup = 1 if graphed else 10 ** 9
        stats = [tr.step(batch) for _ in range(3)]
        assert (tr._graph is not None) == graphed, tr.capture_error
        assert all(np.isfinite(v) for s in stats for v in s.values())
        ends[graphed] = (stats, torch.cat([p.detach().flatten().clone() for p in tr.raw_net.parameters()]))
        del tr
    assert ends[True][0] == ends[False][0], (ends[True][0][-1], ends[False][0][-1])
    assert torch.equal(ends[True][1], ends[False][1])
