"""The split-precision fp32 convolutions (csrc/conv_x3.hip: upf_conv_x3_forward in its tiled and split-K kernels; csrc/conv_x3_bwd.hip:
upf_act_grad_x3, upf_conv_x3_dgrad, upf_conv_x3_wgrad; ops.conv_x3_train) against fp64 BIT FOR BIT.

The operands sit on the two-level grid of tests/_exact_model.py (x3 section): every fp32 operand splits losslessly into two fp16
halves with a non-zero low half, every product of halves and every partial sum of every summation order is exact in fp32, so a
correct kernel has ONE possible output: the fp64 sum of the three products include/upflow_hip.h documents (hi*hi + lo*hi + hi*lo),
plus the bias, un-scaled by the exact powers of two of x3_scale_of.  The guards — (a) lossless split, (b) fewer than 2^24 quanta of
absolute terms, (c) a reference exact in fp32, (d) both cross products non-zero in most outputs — run on each test's own operands
inside the *_case functions, before bit equality is trusted; tests/test_exact_model_cpu.py checks them without a GPU.  There is no
tolerance in this file: torch.equal on values, everywhere.

What bit equality shows that the tolerance suites (test_hip_conv_x3.py, test_hip_conv_x3_train.py, test_hip_conv_x3_bwd_ops.py)
cannot: every product counted once in every reduction order (three and eleven products, split-K forward, gather data gradient,
multi-level split-K weight gradient), elements far below the tensor's maximum, the place of the power-of-two scales relative to
bias, activation, level sum and bias gradient, the `y > 0` mask at exact zeros, and — every operand is a channel slice of a
NaN-filled arena, with NaN channels on both sides, a batch stride that is not C*H*W, once 16-byte aligned and once 4 bytes off —
no dependence on memory outside the operands and no store outside the output.  Where the public function allocates its result
(ops.act_grad_x3, ops.conv_x3_dgrad, ops.conv_x3_wgrad, ops.conv_x3_train) only the operands are arena slices.

Slope 0 is the project's "no activation"; the matrix uses 0.125 (exact); one case per kernel family runs the model's 0.1 against
the epilogue's own order (conv_x3.hip: `v *= winv; v = fmaxf(v, v * slope)`)."""
import pytest
import torch

import _exact_model as em
import _x3_model as xm

pytestmark = pytest.mark.gpu

ISOLATION = 'result depends on memory outside the operand'
OUTSIDE = 'stored outside the output slice'
ROUTES = {'tiled': 0, 'splitk': 1 << 30}
PLACEMENTS = (0, 1)                                   # floats past a 16-byte boundary


@pytest.fixture(autouse=True)
def _drop_packed_operands():
    yield
    from upflow_pytorch_amd import ops
    ops.train_caches_clear()


@pytest.fixture
def routed(request):
    """Sets the launch route of the test's `route` parameter for its duration."""
    from upflow_pytorch_amd import ops
    prev = ops.conv_x3_set_option('sk_max_tiles', ROUTES[request.getfixturevalue('route')])
    yield
    ops.conv_x3_set_option('sk_max_tiles', prev)


def fwd_routes(names):
    """(layer, route) pairs: 'tiled' for every layer, 'splitk' where upf_conv_x3_forward can take it (elsewhere it is 'tiled' again)."""
    return [(n, r) for n in names for r in sorted(ROUTES) if r == 'tiled' or em.x3_splitk_eligible(em.X3_FWD_BY_NAME[n])]


class nprod(object):
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        from upflow_pytorch_amd import ops
        self.prev, ops.CONV_X3_NPROD[0] = ops.CONV_X3_NPROD[0], self.n

    def __exit__(self, *exc):
        from upflow_pytorch_amd import ops
        ops.CONV_X3_NPROD[0] = self.prev


def same32(got, ref64, what):
    assert got.dtype == torch.float32
    g = got.detach().cpu()
    assert g.shape == ref64.shape, (what, g.shape, ref64.shape)
    assert torch.equal(g.double(), ref64), '%s: %d of %d elements differ from the fp64 reference%s' % (
        what, int((g.double() != ref64).sum()), g.numel(), ' — NaN: ' + ISOLATION if bool(torch.isnan(g).any()) else '')


def arena(*shapes):
    """An Arena32 large enough for NCHW blocks of these shapes with up to 5 foreign planes and the margins."""
    n = sum(B * (C + 5) * H * W + 2 * em.Arena.MARGIN + 8 for B, C, H, W in shapes) + em.Arena.MARGIN
    return em.Arena32('cuda', max(n, 1 << 16))


def place(A, t, skew, before=2, after=1):
    """A channel slice holding `t` (or, a shape: nothing yet): NaN planes on both sides, first element `skew` floats past 16 bytes."""
    shape = tuple(t.shape) if torch.is_tensor(t) else tuple(t)
    v = A.nchw(*shape, before=before, after=after, align=4, skew=skew, fill=t if torch.is_tensor(t) else None)
    assert v.data_ptr() % 16 == 4 * skew and (shape[0] == 1 or v.stride(0) != shape[1] * shape[2] * shape[3])
    return v


# ---- forward: ops.conv3x3_forward_raw on fp32 -----------------------------------------------------------------------------------------
def forward_raw(layer, o, slope, skew, n=3):
    from upflow_pytorch_amd import ops
    ho, wo = layer.out_hw
    A = arena(o['x'].shape, (layer.B, layer.Cout, ho, wo))
    x = place(A, o['x'], skew, before=3)
    y = place(A, (layer.B, layer.Cout, ho, wo), skew, before=2, after=2)
    snap = A.snapshot()
    assert ops.conv3x3_supported(x, layer.Cout, layer.d, layer.s, layer.k)
    with nprod(n):
        ops.conv3x3_forward_raw(x, ops.conv3x3_pack(o['w'].cuda()), o['b'].cuda(), y, layer.d, slope, layer.s, layer.k)
    assert A.untouched(snap, y), OUTSIDE
    return y


def products_of(route_name, layer):
    """The split-K kernel exists for three products only (upf_conv_x3_forward: nprod == 3); 11 there is the tiled launch again."""
    return (3,) if route_name == 'splitk' else (3, 11)


@pytest.mark.parametrize('name,route', fwd_routes([l.name for l in em.X3_FWD]))
def test_forward_is_the_three_product_sum(name, route, routed):
    """Every route of upf_conv_x3_forward: the tiled kernel (one 32-channel block per workgroup) in the halo widths 4 (d = 1, 2, 4),
    8 and 16, stride 2, 1x1, with 3 and with 11 products, and the split-K kernel (>= 49 input channels, stride 1) in its three halo
    widths and 1x1 — each on a 16-byte aligned slice (W % 4 == 0: the 16-byte load form) and 4 bytes off (element-wise loads), with
    the slope 0.125 on operands that hold exact zeros among the pre-activations, and without an activation."""
    layer = em.X3_FWD_BY_NAME[name]
    for slope, zeros in ((em.SLOPE, True), (0.0, False)):
        _, o, ref = em.x3_forward_case(name, zeros)                      # (guarded inside)
        assert ref['share'] > 0.5 and (not zeros or bool((ref['pre'] == 0).any()))
        want = em.x3_act(ref['pre'], slope)
        for skew in PLACEMENTS:
            for n in products_of(route, layer):
                same32(forward_raw(layer, o, slope, skew, n), want, (name, route, 'slope %g' % slope, 'skew %d' % skew, 'nprod %d' % n))


@pytest.mark.parametrize('n', [3, 11])
def test_forward_with_two_channel_blocks_per_workgroup(n):
    """conv_x3_kernel<MTW = 2>: Cout > 32 and tiles * ceil(ceil(Cout / 32) / 2) >= 256 — 2 x 16 -> 128 at 64 x 256 is the smallest
    such grid (2 * 8 * 8 tiles, 2 pairs of slabs)."""
    layer, o, ref = em.x3_forward_case(em.X3_TWO.name)
    tiles = layer.B * -(-layer.W // 32) * -(-layer.H // 8)
    assert layer.Cout > 32 and tiles * -(-(-(-layer.Cout // 32)) // 2) >= 256 and tiles > 96       # (beyond the split-K threshold too)
    for skew in PLACEMENTS:
        same32(forward_raw(layer, o, em.SLOPE, skew, n), em.x3_act(ref['pre'], em.SLOPE), (layer.name, skew, n))


@pytest.mark.parametrize('name,route', fwd_routes(em.X3_PLAIN))
def test_forward_equals_the_plain_fp64_convolution_where_no_pair_has_two_low_halves(name, route, routed):
    """Low halves of x on even channels, of w on odd (ci, co): the dropped lo * lo product is zero, the model is the TRUTH."""
    layer, o, ref = em.x3_forward_case(name, True, 'disjoint')
    assert ref['plain'] and ref['nolo']
    for n in products_of(route, layer):
        same32(forward_raw(layer, o, em.SLOPE, 1, n), em.x3_act(ref['pre'], em.SLOPE), (name, route, n))


@pytest.mark.parametrize('name,route', fwd_routes(em.X3_SLOPE01))
def test_forward_with_the_production_slope(name, route, routed):
    layer, o, ref = em.x3_forward_case(name, True)
    for n in products_of(route, layer):
        got = forward_raw(layer, o, 0.1, 0, n).cpu()
        assert torch.equal(got, em.x3_slope01(ref['pre'])), (name, route, n)


@pytest.mark.parametrize('name,route', fwd_routes(em.X3_SCALE))
def test_forward_scales_with_powers_of_two_of_x_and_of_w(name, route, routed):
    """x * 2^-11 (every low half an fp16 subnormal, down to the last one) and x * 2^14 (the top of fp16's range), the bias along with
    x; w * 2^-20 and w * 2^10 (the weight-scale rule and the place of the un-scaling): the same bits times the factor."""
    layer, o, ref = em.x3_forward_case(name, True)
    clean = forward_raw(layer, o, em.SLOPE, 0).cpu()
    same32(clean, em.x3_act(ref['pre'], em.SLOPE), (name, route))
    for kx, kw in [(k, 0) for k in em.X3_X_POW2] + [(0, k) for k in em.X3_W_POW2]:
        _, ok, refk = em.x3_forward_case(name, True, 'all', kx, kw)
        if kx == -11:
            lo = xm.split(ok['x'])[1]
            assert float(lo.abs().max()) == 2.0 ** -24 and bool((lo != 0).any())
        if kx == 14:
            assert float(ok['x'].abs().max()) > 32768.0
        got = forward_raw(layer, ok, em.SLOPE, 0).cpu()
        same32(got, em.x3_act(refk['pre'], em.SLOPE), (name, route, kx, kw))
        assert torch.equal(got.double(), clean.double() * 2.0 ** (kx + kw)), (name, route, kx, kw)


@pytest.mark.parametrize('value', em.X3_NF_VALUES, ids=['inf', 'nan', '65520'])
@pytest.mark.parametrize('name,route', fwd_routes(em.X3_NONFINITE))
def test_a_non_finite_element_stays_inside_its_receptive_field(name, value, route, routed):
    """One inf, NaN or finite |x| >= 65520 (inf as an fp16 half: include/upflow_hip.h, "Range: |x| < 65504") in x: every output whose
    receptive field holds the element is non-finite, every other output has the clean run's bits."""
    layer, o, ref = em.x3_forward_case(name, True)
    x = o['x'].clone()
    n, c, h, w = layer.B - 1, layer.Cin // 2, layer.H // 2, layer.W // 2 + 1
    x[n, c, h, w] = value
    hit = torch.zeros(layer.B, 1, layer.H, layer.W, dtype=torch.float64)
    hit[n, 0, h, w] = 1
    field = (torch.nn.functional.conv2d(hit, torch.ones(1, 1, layer.k, layer.k, dtype=torch.float64), **em.geom(layer.k, layer.d, layer.s)) > 0)
    field = field.expand(-1, layer.Cout, -1, -1)
    assert 0 < int(field.sum()) < field.numel()
    got = forward_raw(layer, dict(o, x=x), em.SLOPE, 1).cpu()
    assert not bool(torch.isfinite(got[field]).any()), 'a finite output inside the receptive field of a non-finite element'
    want = em.x3_act(ref['pre'], em.SLOPE)
    assert torch.equal(got[~field].double(), want[~field]), 'an output outside the receptive field differs from the clean run'


# ---- backward operators ---------------------------------------------------------------------------------------------------------------
def check_slot(slot, ag, what):
    """The slot's three fields: the bits of max |grad_pre|, 2^s, 2^-s (and a zero) — exactly _x3_model.scale_of's."""
    s = slot.cpu()
    assert float(s[0]) == ag['max'] and float(s[1]) == ag['sc'] and float(s[2]) == 1.0 / ag['sc'] and float(s[3]) == 0.0, (what, s.tolist(), ag['max'], ag['sc'])
    assert ag['sc'] == xm.scale_of(ag['max'])


def act_grad_on_arena(gy, y, slope, skew, want_bias):
    from upflow_pytorch_amd import ops
    A = arena(gy.shape, gy.shape)
    g = place(A, gy, skew)
    yv = place(A, y, 1 - skew, before=1, after=3) if y is not None else None
    snap = A.snapshot()
    out = ops.act_grad_x3(g, yv, slope, want_bias=want_bias)
    assert A.untouched(snap), OUTSIDE
    return out


@pytest.mark.parametrize('shape', em.X3_ACT_SHAPES)
def test_act_grad_x3_scales_by_the_power_of_two_of_its_maximum(shape):
    """ops.act_grad_x3 with and without y (exact zeros and negative values in y take the slope), want_bias on and off: gs = grad_pre * 2^s
    exactly, the slot = {max |grad_pre|, 2^s, 2^-s, 0} of _x3_model.scale_of, and each of the 32 first-stage bias sums per channel the
    exact sum of its run (B * H * W is no multiple of 32 in any shape)."""
    gy, y = em.x3_act_case(shape)
    assert (shape[0] * shape[2] * shape[3]) % 32 != 0
    for use_y in (False, True):
        ag = em.x3_act_grad_ref(gy, y if use_y else None, em.SLOPE)
        runs = em.x3_bias_runs(ag['gs'])
        em.guard('bias runs', ag['gs'].double().abs().sum((0, 2, 3)), ag['ug'] * em.X3_FINE)
        for want_bias in (True, False):
            for skew in PLACEMENTS:
                gs, slot, part = act_grad_on_arena(gy, y if use_y else None, em.SLOPE if use_y else 0.0, skew, want_bias)
                what = (shape, use_y, want_bias, skew)
                same32(gs, ag['gs'].double(), what)
                check_slot(slot, ag, what)
                assert (part is not None) == want_bias
                if want_bias:
                    same32(part, runs, what + ('bias runs',))


def dgrad_run(layer, o, ag, skew):
    from upflow_pytorch_amd import ops
    gs, slot, _ = ops.act_grad_x3(ag['gpre'].cuda())
    same32(gs, ag['gs'].double(), 'gs')
    A = arena(gs.shape)
    # (ops.conv_x3_dgrad takes a CONTIGUOUS gs: a channel slice where one image makes it contiguous, else a block between NaN margins)
    g = place(A, ag['gs'], skew) if layer.B == 1 else A.block(*gs.shape, misalign=skew, fill=ag['gs'])
    snap = A.snapshot()
    w = o['w'].cuda()
    shape = (layer.B, layer.Cin, layer.H, layer.W)
    first = ops.conv_x3_dgrad(g, slot, w, shape, layer.d, layer.s)
    second = ops.conv_x3_dgrad(g, slot, w, shape, layer.d, layer.s)      # the same cached pack: its header must have been restored
    assert A.untouched(snap), OUTSIDE
    return first, second


def _dgrad_splitk(layer):
    return layer.s == 1 and (layer.Cout + 15) // 16 >= 4          # (the data gradient's K is the layer's OUTPUT channels)


DGRAD_PARAMS = [(l.name, slope, r) for l in em.X3_DGRAD for slope in (0.0, em.SLOPE) for r in sorted(ROUTES)
                if (r == 'tiled' or _dgrad_splitk(l)) and not (slope and l.name in em.X3_DGRAD_PLAIN_ONLY)]


@pytest.mark.parametrize('name,slope,route', DGRAD_PARAMS)
def test_data_gradient_is_the_three_product_sum(name, slope, route, routed):
    """ops.conv_x3_dgrad.  Stride 1 = the forward kernel on the flipped, transposed pack with the header's 2^-s patched — on the
    tiled and (>= 49 OUTPUT channels of the layer) the split-K route, twice on the same cached pack.  Stride 2 = the fp32 gather
    kernel on the master weights, odd and even H and W, on operands without a pair of two low halves (it forms the plain product)."""
    layer, o, ag, ref = em.x3_dgrad_case(name, slope)
    if layer.s == 1:
        assert ref['share'] > 0.5
    for skew in PLACEMENTS:
        first, second = dgrad_run(layer, o, ag, skew)
        same32(first, ref['gx'], (name, route, slope, skew))
        same32(second, ref['gx'], (name, route, slope, skew, 'second call on the same pack'))


def wgrad_run(levels, conv, order, scaled, want_bias, skew):
    from upflow_pytorch_amd import ops
    Cin, Cout, k, d, s = em.X3_WG_CONVS[conv]
    A = arena(*[t.shape for x, gy, y, ag in levels for t in (x, gy)])
    uses = []
    for l in order:
        x, gy, y, ag = levels[l]
        if scaled:
            gs, slot, part = ops.act_grad_x3(gy.cuda(), y.cuda() if y is not None else None, em.SLOPE if y is not None else 0.0, want_bias=want_bias)
            same32(gs, ag['gs'].double(), 'gs of level %d' % l)
            check_slot(slot, ag, 'level %d' % l)
        else:
            gs, slot, part = ag['gpre'].cuda(), None, None
            if want_bias:                             # (a NULL-slot use's bias_part holds sums of the un-scaled grad_pre)
                part = em.x3_bias_runs(ag['gpre']).float().cuda()
        uses.append((place(A, x, (skew + l) % 2, before=1 + l % 3), place(A, gs, (skew + l + 1) % 2, after=1 + l % 2), slot, part))
    snap = A.snapshot()
    out = ops.conv_x3_wgrad(uses, Cin, Cout, k, d, s, want_bias=want_bias)
    assert A.untouched(snap), OUTSIDE
    return out


@pytest.mark.parametrize('scaled', [True, False], ids=['slots', 'null_slots'])
@pytest.mark.parametrize('conv,n', em.X3_WG_CASES + [em.X3_WG_ACT])
def test_weight_gradient_is_the_exact_sum_over_levels(conv, n, scaled):
    """ops.conv_x3_wgrad: k = 3 and 1, a dilation, stride 2, 1, 2 and 6 (MAXLV) levels whose magnitudes differ by powers of two,
    scaled uses and NULL-slot uses, with and without the bias gradient, Cin / Cout off the 32 / 64 blocks, the level order reversed
    and rotated (the reduction runs in slice order per level; every sum is exact, so any order gives these bits)."""
    slope = em.SLOPE if (conv, n) == em.X3_WG_ACT else 0.0
    levels, ref = em.x3_wgrad_case(conv, n, scaled, 'all', slope)
    assert ref['share'] > 0.5
    L = len(levels)
    orders = [list(range(L))] + ([list(range(L))[::-1], [(i + 2) % L for i in range(L)]] if L > 1 else [])
    for i, order in enumerate(orders):
        want_bias = i != 1
        gw, gb = wgrad_run(levels, conv, order, scaled, want_bias, i % 2)
        same32(gw, ref['gw'], (conv, n, scaled, order, 'grad_w'))
        if want_bias:
            same32(gb, ref['gb'], (conv, n, scaled, order, 'grad_b'))
        else:
            assert gb is None


@pytest.mark.parametrize('conv,n', [('w17', 1), ('w17', 6), ('w83p', 2), ('w5s2', 6)])
def test_weight_gradient_equals_the_plain_fp64_gradient_where_no_pair_has_two_low_halves(conv, n):
    """Low halves of x and of grad_y in different levels (one level: different images): the model is the TRUTH."""
    Cin, Cout, k, d, s = em.X3_WG_CONVS[conv]
    levels, ref = em.x3_wgrad_case(conv, n, True, 'levels')
    assert ref['nolo'] and torch.equal(ref['gw'], em.wgrad_ref([(x, ag['gpre']) for x, _, _, ag in levels], (Cout, Cin, k, k), d, s))
    gw, gb = wgrad_run(levels, conv, list(range(len(levels))), True, True, 0)
    same32(gw, ref['gw'], (conv, n, 'grad_w'))
    same32(gb, ref['gb'], (conv, n, 'grad_b'))


# ---- one full layer: ops.conv_x3_train ---------------------------------------------------------------------------------------------------
def train_run(layer, o, slope, skew):
    from upflow_pytorch_amd import ops
    ho, wo = layer.out_hw
    A = arena(o['x'].shape, o['gy'].shape)
    x = place(A, o['x'], skew, before=3).detach().requires_grad_(True)
    gy = place(A, o['gy'], 1 - skew, after=2)
    snap = A.snapshot()
    w, b = o['w'].cuda().requires_grad_(True), o['b'].cuda().requires_grad_(True)
    y = ops.conv_x3_train(x, w, b, layer.d, slope, layer.s)
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], gy)
    assert A.untouched(snap), OUTSIDE
    return y.detach(), gx, gw, gb


TRAIN_PARAMS = [(l.name, slope, r) for l in em.X3_TRAIN for slope in (em.SLOPE, 0.0) for r in sorted(ROUTES)
                if r == 'tiled' or (l.s == 1 and (em.x3_splitk_eligible(l) or _dgrad_splitk(l)))]


@pytest.mark.parametrize('name,slope,route', TRAIN_PARAMS)
def test_one_training_layer_is_exact_in_all_four_results(name, slope, route, routed):
    """y, grad_x, grad_w and grad_b of one layer through ops.conv_x3_train from ONE operand set: 3x3, dilated, stride 2, 1x1; the mask
    comes from the layer's own forward output, whose exact zeros take the slope."""
    layer, o, ref = em.x3_train_case(name, slope)
    if slope:
        assert bool((ref['pre'] == 0).any())
    for skew in PLACEMENTS:
        y, gx, gw, gb = train_run(layer, o, slope, skew)
        for n, got in (('y', y), ('gx', gx), ('gw', gw), ('gb', gb)):
            same32(got, ref[n], (name, slope, route, skew, n))


@pytest.mark.parametrize('name', em.X3_TRAIN_PLAIN)
def test_training_layer_equals_plain_fp64_where_no_pair_has_two_low_halves(name):
    """Forward and data gradient with the low halves of x and grad_y on even channels, of w on odd (ci, co): both are the plain fp64
    convolutions of the fp32 operands (the weight gradient's twin is test_weight_gradient_equals_the_plain_fp64_gradient...)."""
    layer, o, ref = em.x3_train_case(name, em.SLOPE, 'disjoint')
    assert ref['plain']
    truth = em.layer_ref(o['x'], o['w'], o['b'], o['gy'], layer.k, layer.d, layer.s, em.SLOPE)
    assert torch.equal(ref['y'], truth['y']) and torch.equal(ref['gx'], truth['gx'])
    y, gx, gw, gb = train_run(layer, o, em.SLOPE, 0)
    same32(y, truth['y'], (name, 'y'))
    same32(gx, truth['gx'], (name, 'gx'))
    same32(gw, ref['gw'], (name, 'gw'))
    same32(gb, truth['gb'], (name, 'gb'))


def test_training_layer_with_the_production_slope():
    """Slope 0.1 through ops.conv_x3_train: y in the epilogue's order; grad_pre = grad_y * float32(0.1) where !(y > 0) is no longer on
    the grid, so only y and the mask's effect on the slot are exact claims: gs / 2^s == grad_y * (y > 0 ? 1 : float32(0.1)) in fp32."""
    from upflow_pytorch_amd import ops
    layer, o, ref = em.x3_train_case('t17', em.SLOPE)
    y = forward_raw(layer, o, 0.1, 1)
    assert torch.equal(y.cpu(), em.x3_slope01(ref['pre']))
    gs, slot, _ = act_grad_on_arena(o['gy'], y.cpu(), 0.1, 0, False)
    gpre = o['gy'] * torch.where(y.cpu() > 0, torch.ones(()), torch.tensor(0.1, dtype=torch.float32))
    sc = xm.scale_of(float(gpre.abs().max()))
    assert float(slot.cpu()[1]) == sc and torch.equal(gs.cpu(), gpre * sc)
