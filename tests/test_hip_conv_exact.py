"""The 16-bit convolution kernels (csrc/conv3x3.hip + conv_kernel.hpp with every launch variant, conv_c8.hip, conv_pair.hip,
conv_wgrad.hip with upf_act_grad, the gated data-gradient epilogue and the bias reductions) against an fp64 reference BIT FOR BIT.

The operands sit on grids for which every partial sum of every summation order is exact in fp32 (tests/_exact_model.py; the guard
runs on each test's own operands before bit equality is trusted; tests/test_exact_model_cpu.py checks the conditions without a GPU).
The kernels' results are then fully determined: a 16-bit output is ONE round-to-nearest-even of the exact value, an fp32 output is
the exact value.  Bit equality proves what the tolerance tests cannot see: every product counted exactly once, RNE stores, the
mask convention at exact zeros (`y > 0`: zeros take the slope), and — every operand and output is a slice of a NaN-filled arena —
no dependence on memory outside the operands and no store outside the output.  There is no tolerance in this file.

Where the public function allocates its own result (ops.conv_train: y and the gradients; ops.conv_wgrad_multi: the fp32 gradient)
only the operands are arena slices.  Slope 0 is the project's "no activation" (ops.ConvTrainFunction.forward; conv_kernel.hpp
epilogue_store, "slope = 1 -> identity"); the exact matrix uses slope 0.125, and one forward case per kernel family runs the
production slope 0.1 against the documented order of the epilogue (`v = fmaxf(v, v * slope)` on the fp32 accumulator, then the
conversion — see _exact_model.slope01_ref): conv3x3_forward_raw (conv_kernel.hpp epilogue_store, :204), conv_c8_forward_raw with
both output layouts (the wide NCHW epilogue :270, the octet epilogue :729), the narrow kernel (:674), the split and finishing
launches, the dual 1x1, and conv_pair_forward_raw (conv_pair.hip:215, :226; its first layer, :154, keeps 0.125 so that the
intermediate stays on its grid).  No kernel family had to be excluded.

ops.conv_train copies a channel-sliced x (`x.contiguous()`, ops.ConvTrainFunction.forward) and grad_y (`gy.contiguous()`, backward)
before any kernel reads them unless the batch is 1 (a one-image slice IS contiguous): through conv_train the arena proves isolation
for the B = 1 layers only — the raw-function tests below carry that claim for every kernel."""
import functools

import pytest
import torch

import _exact_model as em

pytestmark = pytest.mark.gpu

DT = [pytest.param(d, id=em.DTYPE_NAMES[d]) for d in em.DTYPES]
ISOLATION = 'result depends on memory outside the operand'
OUTSIDE = 'stored outside the output slice'

MODES = {'auto': {}, 'tiled': {'force_sk': 0, 'small_grid': 0, 'rpw4_min': 0},
         'slabs': {'force_sk': 0, 'force_mtw': 1, 'rpw4_min': 1 << 30}, 'splitk': {'force_sk': 1, 'ph_fit': 0},
         'mtw2_th8': {'force_sk': 0, 'force_mtw': 2, 'ph_fit': 0}}
C8_MODES = {'auto': {}, 'mtw1': {'force_mtw': 1}, 'mtw2': {'force_mtw': 2}, 'th8': {'ph_fit': 0}}


def _mode_fixture(modes):
    @pytest.fixture(params=sorted(modes))
    def fixture(request):
        from upflow_pytorch_amd import ops
        prev = {k: ops.conv_set_option(k, v) for k, v in modes[request.param].items()}
        yield request.param
        for k, v in prev.items():
            ops.conv_set_option(k, v)
    return fixture


conv_mode = _mode_fixture(MODES)
c8_mode = _mode_fixture(C8_MODES)


@pytest.fixture(autouse=True)
def _drop_packed_operands():
    yield
    from upflow_pytorch_amd import ops
    ops.train_caches_clear()


def r16(ref64, dtype):
    """The ONE rounding of the exact value: fp64 -> dtype.  The finite reference values are fp32 values (so there is no double
    rounding on the way)."""
    r32 = ref64.float()
    fin = torch.isfinite(ref64)
    assert torch.equal(r32[fin].double(), ref64[fin]), 'the reference is not exact in fp32: a broken test'
    return r32.to(dtype)


def same16(got, ref64, what):
    want = r16(ref64, got.dtype)
    g = got.detach().cpu()
    assert g.shape == want.shape, (what, g.shape, want.shape)
    assert torch.equal(g, want), '%s: %d of %d elements differ from RNE(fp64 reference)%s' % (
        what, int((g != want).sum()), g.numel(), ' — NaN: ' + ISOLATION if bool(torch.isnan(g).any()) else '')


def same32(got, ref64, what):
    assert got.dtype == torch.float32
    g = got.detach().cpu()
    assert g.shape == ref64.shape, (what, g.shape, ref64.shape)
    assert torch.equal(g.double(), ref64), '%s: %d of %d elements differ from the fp64 reference%s' % (
        what, int((g.double() != ref64).sum()), g.numel(), ' — NaN: ' + ISOLATION if bool(torch.isnan(g).any()) else '')


def pitch8(W):
    return (W + 7) // 8 * 8


# ---- training: ops.conv_train ------------------------------------------------------------------------------------------------------
def run_train(layer, o, dtype, slope, need=(True, True, True)):
    """ops.conv_train + autograd on operands carved from an arena -> dict y, gx, gw, gb (None where not asked for).  (For B > 1
    conv_train copies the slices before its kernels read them: see the file's docstring.)"""
    from upflow_pytorch_amd import ops
    A = em.Arena(dtype, 'cuda')
    ho, wo = layer.out_hw
    x = A.nchw(layer.B, layer.Cin, layer.H, layer.W, before=2, fill=o['x']).detach().requires_grad_(need[0])
    gy = A.nchw(layer.B, layer.Cout, ho, wo, after=2, fill=o['gy'])
    snap = A.snapshot()
    w = o['w'].cuda().requires_grad_(need[1])
    b = o['b'].cuda().requires_grad_(need[2]) if o['b'] is not None else None
    assert ops.conv_train_supported(x, w, layer.s, layer.d)
    y = ops.conv_train(x, w, b, layer.d, slope, layer.s)
    names = [n for n, t, q in zip(('gx', 'gw', 'gb'), (x, w, b), need) if t is not None and q]
    grads = torch.autograd.grad(y, [{'gx': x, 'gw': w, 'gb': b}[n] for n in names], gy)
    out = {'y': y.detach(), 'gx': None, 'gw': None, 'gb': None}
    out.update(zip(names, grads))
    assert A.untouched(snap), OUTSIDE
    return out


def check_train(got, ref, what):
    same16(got['y'], ref['y'], '%s y' % (what,))
    if got['gx'] is not None:
        same16(got['gx'], ref['gx'], '%s grad_x' % (what,))
    if got['gw'] is not None:
        same32(got['gw'], ref['gw'], '%s grad_w' % (what,))
    if got['gb'] is not None:
        same32(got['gb'], ref['gb'], '%s grad_b' % (what,))


# (slope, bias, (grad x, grad w, grad b))
FULL = (em.SLOPE, True, (True, True, True))
VARIANTS = {'plain': (0.0, True, (True, True, True)), 'nobias': (em.SLOPE, False, (True, True, False)), 'plain_nobias': (0.0, False, (True, True, False)),
            'no_gx': (em.SLOPE, True, (False, True, True)), 'frozen_w': (em.SLOPE, True, (True, False, True)), 'frozen_b': (em.SLOPE, True, (True, True, False))}
TRAIN_PARAMS = [pytest.param(l.name, FULL, id=l.name) for l in em.TRAIN] + [pytest.param(n, v, id='%s-%s' % (n, vn)) for n in em.MATRIX_LAYERS for vn, v in VARIANTS.items()]


@pytest.mark.parametrize('name,variant', TRAIN_PARAMS)
@pytest.mark.parametrize('dtype', DT)
def test_conv_train_is_the_fp64_layer_rounded_once(name, variant, dtype):
    """Forward, data, weight and bias gradient of one layer through ops.conv_train: stride 1 (every dilation, 1x1), stride 2 on the
    space-to-depth path (even sizes) and on the torch fallback (odd sizes); the launch matrix (no activation, no bias, skipped data
    gradient, frozen weight / bias) on em.MATRIX_LAYERS."""
    from upflow_pytorch_amd import ops
    slope, bias, need = variant
    layer, o, ref, _ = em.train_case(name, dtype, slope, bias)           # (guarded inside)
    if layer.s == 2:
        assert ops._s2d_ok(o['x'].to(dtype).cuda(), o['w'].cuda(), 2, 1) == (layer.H % 2 == 0 and layer.W % 2 == 0)
    check_train(run_train(layer, o, dtype, slope, need), ref, (name, variant))


@pytest.mark.parametrize('dtype', DT)
def test_one_convolution_at_three_levels_inside_shared_conv_grads(dtype):
    """The sink contraction and the gate node (ops.shared_conv_grads) produce the exact sum over the uses."""
    from upflow_pytorch_amd import ops
    levels, os_, refs = em.shared_case(dtype)                            # (guarded inside)
    Cin, Cout = 33, 32
    conv = torch.nn.Conv2d(Cin, Cout, 3, padding=1).cuda()
    with torch.no_grad():
        conv.weight.copy_(os_[0]['w'])
        conv.bias.copy_(os_[0]['b'])
    A = em.Arena(dtype, 'cuda')
    xs = [A.nchw(l.B, Cin, l.H, l.W, before=1 + i, fill=o['x']).detach().requires_grad_(True) for i, (l, o) in enumerate(zip(levels, os_))]
    gys = [A.nchw(l.B, Cout, l.H, l.W, fill=o['gy']) for l, o in zip(levels, os_)]
    snap = A.snapshot()
    with ops.shared_conv_grads([conv]):
        ys = [ops.conv_train(x, conv.weight, conv.bias, 1, em.SLOPE) for x in xs]
    assert not ops._GATES
    grads = torch.autograd.grad(ys, xs + [conv.weight, conv.bias], gys)
    for i, r in enumerate(refs):
        same16(ys[i], r['y'], 'level %d y' % i)
        same16(grads[i], r['gx'], 'level %d grad_x' % i)
    same32(grads[3], sum(r['gw'] for r in refs), 'grad_w over three uses')
    same32(grads[4], sum(r['gb'] for r in refs), 'grad_b over three uses')
    assert A.untouched(snap), OUTSIDE


# ---- the weight gradient and its companions, through the raw functions ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wg_case(conv, n, dtype):
    Cin, Cout, k, d = em.WG_CONVS[conv]
    uses, st = em.wgrad_operands(conv, n, dtype)
    em.guard_wgrad(uses, (Cout, Cin, k, k), d, 1, st['x'], st['gy'])
    em.guard_bias([g for _, g in uses], st['gy'])
    return uses, em.wgrad_ref(uses, (Cout, Cin, k, k), d), sum(g.double().sum((0, 2, 3)) for _, g in uses)


@pytest.mark.parametrize('conv,n', em.WG_CASES)
@pytest.mark.parametrize('dtype', DT)
def test_wgrad_multi_is_the_exact_sum_over_uses(conv, n, dtype):
    """ops.conv_wgrad_multi over 1, 2, 6 and 7 uses (7: two launches), aligned and ragged levels mixed in one call, wide and narrow
    (Cin, Cout <= 32) layers, with and without the fused bias finish (`bias_parts`)."""
    from upflow_pytorch_amd import ops
    Cin, Cout, k, d = em.WG_CONVS[conv]
    uses_cpu, ref_w, ref_b = _wg_case(conv, n, dtype)
    A = em.Arena(dtype, 'cuda')
    uses = [(A.nchw(x.shape[0], Cin, x.shape[2], x.shape[3], before=1 + i % 2, fill=x), A.nchw(g.shape[0], Cout, g.shape[2], g.shape[3], after=1 + i % 3, fill=g))
            for i, (x, g) in enumerate(uses_cpu)]
    snap = A.snapshot()
    same32(ops.conv_wgrad_multi(uses, Cin, Cout, k, d), ref_w, 'grad_w')
    parts = [ops.act_grad(g, dst=False, want_bias=True)[1] for _, g in uses]
    same32(ops.conv_bias_grad_finish(parts, Cout), ref_b, 'grad_b (separate finish)')
    if n <= 6:
        gw, gb = ops.conv_wgrad_multi(uses, Cin, Cout, k, d, bias_parts=parts)
        same32(gw, ref_w, 'grad_w (fused bias finish)')
        same32(gb, ref_b, 'grad_b (fused finish)')
    assert A.untouched(snap), OUTSIDE


@pytest.mark.parametrize('name', ['s2e', 's2n'])
@pytest.mark.parametrize('dtype', DT)
def test_wgrad_of_the_space_to_depth_form(name, dtype):
    """ops.conv_wgrad_s2d on the space-to-depth input of a stride-2 layer == the strided layer's fp64 weight gradient."""
    from upflow_pytorch_amd import ops
    layer, o, ref, _ = em.train_case(name, dtype)
    A = em.Arena(dtype, 'cuda')
    ho, wo = layer.out_hw
    # (the function takes contiguous tensors: the whole batch is one block between foreign planes)
    xs = A.nchw(1, layer.B * 4 * layer.Cin, ho, wo).view(layer.B, 4 * layer.Cin, ho, wo)
    g = A.nchw(1, layer.B * layer.Cout, ho, wo, before=2).view(layer.B, layer.Cout, ho, wo)
    xs.copy_(torch.nn.functional.pixel_unshuffle(o['x'], 2))
    g.copy_(ref['gpre'])
    snap = A.snapshot()
    same32(ops.conv_wgrad_s2d(xs, g, layer.Cin, layer.Cout), ref['gw'], 'grad_w')
    assert A.untouched(snap), OUTSIDE


@pytest.mark.parametrize('value', [None, float('nan'), float('inf')], ids=['finite', 'nan', 'inf'])
@pytest.mark.parametrize('name', ['s2e', 's2n'])
@pytest.mark.parametrize('dtype', DT)
def test_space_to_depth_data_gradient_of_the_c_abi(name, value, dtype):
    """The data gradient of a stride-2 layer as include/upflow_hip.h describes it for C callers — upf_conv_pack_weights_f32(dgrad = 2),
    the stride-1 convolution of grad_pre, upf_space_to_depth2(inverse) — which ops.conv_train no longer takes: the fp64 gradient
    rounded once on finite operands.  With one non-finite element in grad_pre it behaves as the header says: every element the
    reference makes non-finite is non-finite, everything outside the 6x6 pixel block around it keeps the clean run's bits (inside
    the block the packed kernel's structural zeros give 0 * NaN = NaN: the documented limit of this form)."""
    from upflow_pytorch_amd import ops
    layer, o, ref, _ = em.train_case(name, dtype)
    ho, wo = layer.out_hw
    gpre = ref['gpre'].float()
    want = ref['gx']
    h0, w0 = ho // 2, wo // 2
    if value is not None:
        gpre = gpre.clone()
        gpre[0, 1, h0, w0] = value
        want = torch.nn.grad.conv2d_input(o['x'].shape, o['w'].double(), gpre.double(), **em.geom(3, 1, 2))
    A = em.Arena(dtype, 'cuda')
    g = A.nchw(layer.B, layer.Cout, ho, wo, before=2, fill=gpre)
    gxs = A.nchw(layer.B, 4 * layer.Cin, ho, wo)
    snap = A.snapshot()
    packed = ops._conv_pack_from_master(o['w'].cuda(), dtype, 2)
    ops.conv3x3_forward_raw(g, packed, torch.zeros(4 * layer.Cin, device='cuda'), gxs, 1, 0.0, 1, 3)
    assert A.untouched(snap, gxs), OUTSIDE
    got = ops.space_to_depth2(gxs, inverse=True).cpu()
    if value is None:
        same16(got, want, 'grad_x')
        return
    fin = torch.isfinite(want)
    assert bool((~fin).any()) and not bool(torch.isfinite(got)[~fin].any())
    outside = torch.ones_like(fin)
    outside[0, :, 2 * h0 - 2:2 * h0 + 4, 2 * w0 - 2:2 * w0 + 4] = False
    assert bool(fin[outside].all()) and torch.equal(got[outside], r16(ref['gx'], dtype)[outside])


@pytest.mark.parametrize('shape', em.ACT_SHAPES)
@pytest.mark.parametrize('dtype', DT)
def test_act_grad_and_the_bias_reductions(shape, dtype):
    """ops.act_grad with and without `add` and `y` (exact zeros in y take the slope), into an arena slice; its bias partial sums
    through ops.conv_bias_grad_finish over 1, 2 and 9 partial buffers."""
    from upflow_pytorch_amd import ops
    B, C, H, W = shape
    G = em.GRIDS[dtype]
    src, add, yv = em.act_case(shape, dtype)
    for use_add in (False, True):
        for use_y in (False, True):
            A = em.Arena(dtype, 'cuda')
            s, a, y, dst = (A.nchw(B, C, H, W, before=1 + i, fill=t) for i, t in enumerate((src, add, yv, None)))
            snap = A.snapshot()
            ref = src.double() + (add.double() if use_add else 0.0)
            if use_y:
                ref = ref * em.act_mask(yv.double(), em.SLOPE)
            step = G['gy'][0] * (em.SLOPE if use_y else 1.0)
            top = em.guard_bias([ref], step)
            assert 9 * top < em.LIMIT
            out, part = ops.act_grad(s, y if use_y else None, em.SLOPE, add=a if use_add else None, dst=dst, want_bias=True)
            assert out is dst
            same16(dst, ref, 'act_grad add=%s y=%s' % (use_add, use_y))
            assert A.untouched(snap, dst), OUTSIDE
            same32(ops.conv_bias_grad_finish([part], C), ref.sum((0, 2, 3)), 'bias gradient of the stored result')
    # 1, 2 and 9 DIFFERENT partial buffers (9: two launches of the finish): a finish that mis-indexes them gives another sum
    A = em.Arena(dtype, 'cuda')
    ts = em.bias_parts_case(shape, dtype)
    parts = [ops.act_grad(A.nchw(B, C, H, W, fill=t), dst=False, want_bias=True)[1] for t in ts]
    for n in (1, 2, 9):
        same32(ops.conv_bias_grad_finish(parts[:n], C), sum(t.double().sum((0, 2, 3)) for t in ts[:n]), 'bias gradient over %d partial buffers' % n)


@pytest.mark.parametrize('layer', em.GATED, ids=repr)
@pytest.mark.parametrize('dtype', DT)
def test_gated_convolution_is_the_fp64_composition(layer, dtype):
    """ops.conv3x3_forward_gated_raw against fp64 in the order its docstring states (ops.py, conv3x3_forward_gated_raw:
    `y = round16(round16(conv) + add) * (act > 0 ? 1 : mask_slope)`, rounded): every step is one RNE of an exact value."""
    from upflow_pytorch_amd import ops
    o, add, actv, conv64 = em.gated_case(layer, dtype)
    shape = (layer.B, layer.Cout, layer.H, layer.W)
    conv16 = r16(conv64, dtype).double()
    packed = ops.conv3x3_pack(o['w'].to(dtype).cuda())
    bias = o['b'].cuda()
    for use_add, use_act in ((False, True), (True, True), (True, False)):
        A = em.Arena(dtype, 'cuda')
        x = A.nchw(layer.B, layer.Cin, layer.H, layer.W, before=3, fill=o['x'])
        y, a, m = (A.nchw(*shape, before=1 + i, fill=t) for i, t in enumerate((None, add, actv)))
        snap = A.snapshot()
        ref = conv16
        if use_add:
            ref = (ref + add.double()).to(dtype).double()
        if use_act:
            ref = ref * em.act_mask(actv.double(), em.SLOPE)
        ops.conv3x3_forward_gated_raw(x, packed, bias, y, a if use_add else None, m if use_act else None, em.SLOPE)
        same16(y, ref, 'gated add=%s act=%s' % (use_add, use_act))
        assert A.untouched(snap, y), OUTSIDE


# ---- non-finite operands, range ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('value', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('where', ['gy', 'x'])
@pytest.mark.parametrize('layer', em.NONFINITE_LAYERS, ids=repr)
@pytest.mark.parametrize('dtype', DT)
def test_non_finite_operands_surface_in_every_gradient_they_reach(layer, where, value, dtype):
    """One NaN / +inf at an interior pixel (>= dilation from every border: no padding product) of grad_y, or of x for the weight
    gradient; operands without exact zeros.  isfinite(got) == isfinite(fp64 reference) elementwise; grad_y: every gradient has
    non-finite elements; x: the weight gradient has.  Every element that is finite in the reference has the reference's bits (for
    grad_y these are the clean run's bits too).  NaN versus inf is not asserted.

    Found by this test and fixed with it: the stride-2 data gradient used to run as a stride-1 convolution of grad_pre with the
    space-to-depth kernel w4, whose structural zero weights were multiplied like any weight — 0 * NaN = NaN made 576 elements of
    grad_x non-finite (6x6 pixels x 16 channels) where the reference has 144 (3x3 x 16).  ops.ConvTrainFunction.backward now takes
    the transposed form (zeros in the data, not in the weights); [nf_s2-gy-*] are the regression cases."""
    _, o, clean_ref, _ = em.train_case(layer.name, dtype, em.SLOPE, True, True)
    t = o[where].clone()
    h, w = t.shape[2] // 2, t.shape[3] // 2
    assert min(h, t.shape[2] - 1 - h, w, t.shape[3] - 1 - w) >= (layer.d if layer.k == 3 else 0)
    t[0, 1, h, w] = value
    p = dict(o)
    p[where] = t
    ref = em.layer_ref(p['x'], p['w'], p['b'], p['gy'], layer.k, layer.d, layer.s, em.SLOPE)
    em.guard_layer(p, ref, layer.k, layer.d, layer.s, em.SLOPE)          # (the planted operands: their finite part)
    got = run_train(layer, p, dtype, em.SLOPE)
    clean = run_train(layer, o, dtype, em.SLOPE) if where == 'gy' else None
    for n in ('gx', 'gw', 'gb'):
        fin = torch.isfinite(ref[n])
        g = got[n].detach().cpu()
        assert torch.equal(torch.isfinite(g), fin), '%s: finite where the reference is not, or the reverse (%d vs %d non-finite)' % (
            n, int((~torch.isfinite(g)).sum()), int((~fin).sum()))
        assert bool((~fin).any()) or (where == 'x' and n != 'gw'), n
        want = r16(ref[n], dtype) if n == 'gx' else ref[n].float()
        assert torch.equal(g[fin], want[fin]), n
        if clean is not None:
            assert torch.equal(g[fin], clean[n].detach().cpu()[fin]), n
            assert torch.equal(ref[n][fin], clean_ref[n][fin]), n


def test_fp16_data_gradient_overflows_to_inf_exactly_where_the_reference_does():
    name, k = em.FP16_OVERFLOW
    layer, o, ref, _ = em.train_case(name, torch.float16, em.SLOPE, True, False, k)
    got = run_train(layer, o, torch.float16, em.SLOPE)
    want = ref['gx'].to(torch.float16)
    assert bool(torch.isinf(want).any()) and bool(torch.isfinite(want).any())
    assert torch.equal(torch.isinf(got['gx'].cpu()), torch.isinf(want))
    check_train(got, ref, name)


def test_fp16_subnormal_grad_y_gives_the_exact_weight_gradient():
    """grad_y entirely in the fp16 subnormal range (multiples of 2^-24 after the slope): the matrix instruction keeps subnormal inputs
    (test_fp16_matrix_instruction_keeps_subnormal_inputs), so the weight gradient is the exact, non-zero fp64 value."""
    name, gg = em.FP16_SUBNORMAL
    layer, o, ref, _ = em.train_case(name, torch.float16, em.SLOPE, True, False, 0, gg)
    assert float(o['gy'].abs().max()) < 2.0 ** -14
    got = run_train(layer, o, torch.float16, em.SLOPE)
    assert float(got['gw'].abs().max()) > 0
    check_train(got, ref, name)


@pytest.mark.parametrize('name', em.SCALE_LAYERS)
@pytest.mark.parametrize('dtype', DT)
def test_gradients_scale_with_a_power_of_two_of_grad_y(name, dtype):
    """grad_y * 2^k gives bit-identical gradients times 2^k (k: em.SCALE_K; nothing leaves the normal range — the CPU file checks)."""
    gg = em.SCALE_GY[dtype]
    layer, o, ref, _ = em.train_case(name, dtype, em.SLOPE, True, False, 0, gg)
    clean = run_train(layer, o, dtype, em.SLOPE)
    check_train(clean, ref, (name, 0))
    for k in em.SCALE_K[dtype]:
        _, ok, refk, _ = em.train_case(name, dtype, em.SLOPE, True, False, k, gg)
        got = run_train(layer, ok, dtype, em.SLOPE)
        check_train(got, refk, (name, k))
        for n in ('gx', 'gw', 'gb'):
            assert torch.equal(got[n].cpu().double(), clean[n].cpu().double() * 2.0 ** k), (name, k, n)


# ---- inference forward, through the raw functions --------------------------------------------------------------------------------------
def _forward_raw(layer, o, dtype, slope, pitched):
    from upflow_pytorch_amd import ops
    A = em.Arena(dtype, 'cuda')
    x = A.nchw(layer.B, layer.Cin, layer.H, layer.W, before=5, pitch=pitch8(layer.W) if pitched else None, align=8 if pitched else 1, fill=o['x'])
    ho, wo = layer.out_hw
    y = A.nchw(layer.B, layer.Cout, ho, wo, before=2)
    snap = A.snapshot()
    assert ops.conv3x3_supported(x, layer.Cout, layer.d, layer.s, layer.k)
    ops.conv3x3_forward_raw(x, ops.conv3x3_pack(o['w'].to(dtype).cuda()), o['b'].cuda(), y, layer.d, slope, layer.s, layer.k)
    assert A.untouched(snap, y), OUTSIDE
    return y


@pytest.mark.parametrize('name', [l.name for l in em.FWD])
@pytest.mark.parametrize('dtype', DT)
def test_conv_forward_is_the_fp64_layer_rounded_once(name, dtype, conv_mode):
    """ops.conv3x3_forward_raw in every launch mode of test_hip_conv.py — each mode against the ONE reference, so all variants of a
    layer give the same bits: stride 1 and 2, 1x1, every dilation, contiguous and row-pitched inputs (NaN in the pitch columns, the
    layout of ops.empty_nchw), with and without the activation."""
    layer, o, pre, y = em.forward_case(name, dtype)
    for pitched in ((False, True) if layer.W % 8 else (False,)):
        same16(_forward_raw(layer, o, dtype, em.SLOPE, pitched), y, (name, conv_mode, 'pitched' if pitched else 'contiguous'))
    same16(_forward_raw(layer, o, dtype, 0.0, False), pre, (name, conv_mode, 'no activation'))


@pytest.mark.parametrize('name', ['f115', 'f196p', 'f3s2'])
@pytest.mark.parametrize('dtype', DT)
def test_conv_forward_with_the_production_slope(name, dtype, conv_mode):
    """Slope 0.1 is no power of two: the expected bits follow the epilogue's documented order (conv_kernel.hpp, epilogue_store:
    `v0 = fmaxf(v0, v0 * slope)` on the fp32 accumulator, THEN the 16-bit conversion): the exact fp32 pre-activation times
    float32(0.1) in fp32, one RNE to the dtype."""
    layer, o, pre, _ = em.forward_case(name, dtype)
    got = _forward_raw(layer, o, dtype, 0.1, False).cpu()
    assert torch.equal(got, em.slope01_ref(pre, dtype)), (name, conv_mode)


@pytest.mark.parametrize('name', sorted(em.C8))
@pytest.mark.parametrize('dtype', DT)
def test_conv_c8_forward_is_the_fp64_layer_rounded_once(name, dtype, c8_mode):
    """ops.conv_c8_forward_raw: octet input (padding channels of the last octet zeros, as the layout's contract says) with and
    without an NCHW tail, both output layouts, its four launch modes."""
    from upflow_pytorch_amd import ops
    B, C8c, C2, Cout, H, W, d, y_c8 = em.C8[name]
    layer, o, pre, yref = em.forward_case(name, dtype)
    n8 = (C8c + 7) // 8
    A = em.Arena(dtype, 'cuda')
    x8 = A.c8(B, C8c, H, W, before=2, fill=o['x'][:, :C8c])
    x2 = A.nchw(B, C2, H, W, before=5, align=8, fill=o['x'][:, C8c:]) if C2 else None
    y = A.c8(B, Cout, H, W) if y_c8 else A.nchw(B, Cout, H, W, before=8)
    snap = A.snapshot()
    packed = ops.conv_c8_pack(o['w'].to(dtype).cuda(), list(range(C8c)) + [-1] * (n8 * 8 - C8c), list(range(C8c, C8c + C2)))
    assert ops.conv_c8_supported(H, W, dtype, Cout, d, 3, True, C2 > 0, y_c8)
    ops.conv_c8_forward_raw(x8, x2, packed, o['b'].cuda(), y, dilation=d, leaky_slope=em.SLOPE)
    _check_c8_or_nchw(y, yref, Cout, (name, c8_mode))
    assert A.untouched(snap, y), OUTSIDE
    if name in ('o32t83', 'o184'):         # the production slope, octet (conv_kernel.hpp:729) and NCHW (:270) epilogue
        ops.conv_c8_forward_raw(x8, x2, packed, o['b'].cuda(), y, dilation=d, leaky_slope=0.1)
        got = em.from_c8(y.cpu())[:, :Cout] if y_c8 else y.cpu()
        assert torch.equal(got, em.slope01_ref(pre, dtype)), (name, c8_mode, 'slope 0.1')
        assert A.untouched(snap, y), OUTSIDE


def _check_c8_or_nchw(y, ref64, Cout, what):
    if y.dim() == 5:
        full = em.from_c8(y.cpu())
        same16(full[:, :Cout], ref64, what)
        assert float(full[:, Cout:].float().abs().sum()) == 0.0, 'the channels that pad the last octet must be zeros'
    else:
        same16(y, ref64, what)


@pytest.mark.parametrize('name', sorted(em.C8_NARROW))
@pytest.mark.parametrize('dtype', DT)
def test_conv_c8_narrow_forward_is_the_fp64_layer_rounded_once(name, dtype):
    """ops.conv_c8_forward_narrow_raw (Cout <= 16 on the 16-output-channel matrix instruction), NCHW and octet outputs; one case
    also at the production slope 0.1 (same epilogue order as the wide kernels: activation on the fp32 sum, then the conversion)."""
    from upflow_pytorch_amd import ops
    B, Cin, Cout, H, W, y_c8 = em.C8_NARROW[name]
    layer, o, pre, yref = em.forward_case(name, dtype)
    n8 = (Cin + 7) // 8
    packed = ops.conv_c8_pack16(o['w'].to(dtype).cuda(), list(range(Cin)) + [-1] * (n8 * 8 - Cin))
    for slope in ((em.SLOPE, 0.1) if name == 'n184_3' else (em.SLOPE,)):
        A = em.Arena(dtype, 'cuda')
        x8 = A.c8(B, Cin, H, W, fill=o['x'])
        y = A.c8(B, Cout, H, W, before=2) if y_c8 else A.nchw(B, Cout, H, W, before=3)
        snap = A.snapshot()
        ops.conv_c8_forward_narrow_raw(x8, packed, o['b'].cuda(), y, slope)
        if slope == 0.1:
            assert torch.equal(y.cpu(), em.slope01_ref(pre, dtype)), name
        else:
            _check_c8_or_nchw(y, yref, Cout, name)
        assert A.untouched(snap, y), OUTSIDE


@pytest.mark.parametrize('geom', em.TAIL)
@pytest.mark.parametrize('dtype', DT)
def test_merged_tail_split_and_finishing_launch(geom, dtype):
    """ops.conv_c8_forward_split_raw + ops.conv_c8_forward_narrow_init_raw (the merged narrow tail of a dense stack): the main layer
    complete, the later layer's shared-input part as fp32 partials, finished from the main layer's 16-bit output — against the two
    layers in fp64 with the main layer's output rounded to the dtype (what the finishing launch reads)."""
    from upflow_pytorch_amd import ops
    B, Cin, Cm, Cj, H, W = geom
    c = em.tail_case(geom, dtype)                                        # (both layers guarded inside)
    x, wm, bm, wj, bj, ym, yj = (c[n] for n in ('x', 'wm', 'bm', 'wj', 'bj', 'ym', 'yj'))
    pad = (Cj + 3) // 4 * 4 - Cj
    rows = torch.cat([wm, wj[:, Cm:], torch.zeros(pad, Cin, 3, 3)], 0).to(dtype).cuda()
    bias = torch.cat([bm, bj, torch.zeros(pad)]).cuda()
    packed = ops.conv_c8_pack(rows, list(range(Cin)))
    finish = ops.conv_c8_pack16(wj[:, :Cm].contiguous().to(dtype).cuda(), list(range(Cm)))
    A = em.Arena(dtype, 'cuda')
    x8 = A.c8(B, Cin, H, W, fill=x)
    y8 = A.c8(B, Cm, H, W, before=2)
    y = A.nchw(B, Cj, H, W, before=2)
    part = torch.full((B, (Cj + 3) // 4, H, W, 4), float('nan'), device='cuda')
    snap = A.snapshot()
    ops.conv_c8_forward_split_raw(x8, packed, bias, y8, part, em.SLOPE)
    same16(em.from_c8(y8.cpu()), ym, 'main layer')
    ops.conv_c8_forward_narrow_init_raw(y8, finish, part, 0, Cj, y, em.SLOPE)
    same16(y, yj, 'finished layer')
    # the production slope in the finishing launch (from the same 0.125 main layer, whose output stays on its grid) ...
    ops.conv_c8_forward_narrow_init_raw(y8, finish, part, 0, Cj, y, 0.1)
    assert torch.equal(y.cpu(), em.slope01_ref(c['prej'], dtype)), 'finished layer, slope 0.1'
    # ... and in the split launch's own epilogue
    ops.conv_c8_forward_split_raw(x8, packed, bias, y8, part, 0.1)
    assert torch.equal(em.from_c8(y8.cpu()), em.slope01_ref(c['prem'], dtype)), 'main layer, slope 0.1'
    assert A.untouched(snap, y8, y), OUTSIDE


@pytest.mark.parametrize('geom', em.DUAL)
@pytest.mark.parametrize('dtype', DT)
def test_conv1x1_to_octets_one_and_two_destinations(geom, dtype):
    """ops.conv1x1_c8_dual_raw (both destinations) and the single-destination 1x1 NCHW -> octets of ops.conv_c8_forward_raw."""
    from upflow_pytorch_amd import ops
    layer, o, yref = em.dual_case(geom, dtype)
    B, Cin, Cout, H, W = geom
    A = em.Arena(dtype, 'cuda')
    x = A.nchw(B, Cin, H, W, before=3, pitch=pitch8(W), align=8, fill=o['x'])
    ya, yb, yc = A.c8(B, Cout, H, W), A.c8(B, Cout, H, W, before=2, after=3), A.c8(B, Cout, H, W)
    snap = A.snapshot()
    w16 = o['w'].to(dtype).cuda()
    ops.conv1x1_c8_dual_raw(x, ops.conv_c8_pack(w16, (), range(Cin)), o['b'].cuda(), ya, yb, em.SLOPE)
    ops.conv_c8_forward_raw(None, x, ops.conv3x3_pack(w16), o['b'].cuda(), yc, dilation=1, leaky_slope=em.SLOPE, kernel_size=1)
    for y in (ya, yb, yc):
        _check_c8_or_nchw(y, yref, Cout, geom)
    if geom == em.DUAL[0]:                 # the production slope
        pre = em.forward_ref(o['x'], o['w'], o['b'], 1, 1, 1)[0]
        ops.conv1x1_c8_dual_raw(x, ops.conv_c8_pack(w16, (), range(Cin)), o['b'].cuda(), ya, yb, 0.1)
        for y in (ya, yb):
            assert torch.equal(em.from_c8(y.cpu())[:, :Cout], em.slope01_ref(pre, dtype)), (geom, 'slope 0.1')
    assert A.untouched(snap, ya, yb, yc), OUTSIDE


@pytest.mark.parametrize('name', sorted(em.PAIR))
@pytest.mark.parametrize('dtype', DT)
def test_conv_pair_is_the_two_layer_composition(name, dtype):
    """ops.conv_pair_forward_raw, both stride orders and both output layouts, against the two layers in fp64 with the intermediate
    layer rounded to the 16-bit dtype; the guard runs on the second layer's real (rounded) input.  Second-layer slopes 0.125, none
    and the production 0.1 (first layer 0.125 throughout: the intermediate stays on its grid)."""
    from upflow_pytorch_amd import ops
    B, Cin, C1, C2, H, W, strides, y_c8 = em.PAIR[name]
    o = em.pair_operands(name, dtype)
    for sa, sb in ((em.SLOPE, em.SLOPE), (em.SLOPE, 0.0), (em.SLOPE, 0.1)):
        _, _, pre_b, yref = em.pair_ref(o, strides, sa, sb, dtype)
        A = em.Arena(dtype, 'cuda')
        x = A.nchw(B, Cin, H, W, before=2, pitch=pitch8(W), align=8, fill=o['x'])
        ho, wo = em.out_hw(H, W, 2)
        y = A.c8(B, C2, ho, wo) if y_c8 else A.nchw(B, C2, ho, wo, before=2)
        snap = A.snapshot()
        pa, pb = ops.conv_pair_pack(o['wa'].to(dtype).cuda(), o['wb'].to(dtype).cuda())
        ops.conv_pair_forward_raw(x, pa, o['ba'].cuda(), sa, pb, o['bb'].cuda(), sb, y, strides)
        if sb == 0.1:                      # the production slope in the second layer's epilogue (conv_pair.hip:215, :226)
            got = em.from_c8(y.cpu()) if y_c8 else y.cpu()
            assert torch.equal(got[:, :C2], em.slope01_ref(pre_b, dtype)), (name, 'slope 0.1')
        else:
            _check_c8_or_nchw(y, yref, C2, (name, sa, sb))
        assert A.untouched(snap, y), OUTSIDE
