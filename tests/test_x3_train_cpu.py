"""Host-side pieces of the fp32 training mode on the matrix cores (`fp32_train_conv`): flag validation, bindings, and the K-split
plan of the weight gradient (a pure host function).  No GPU needed."""
import ctypes

import pytest
import torch


def test_fp32_train_conv_flag_is_validated():
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    from upflow_pytorch_amd.model import pwc_modules
    conf = UPFlow_net.config()
    assert conf.fp32_train_conv == 'miopen'              # the default keeps today's behaviour
    conf.update({'fp32_train_conv': 'hip_x3'}, verbose=False)
    assert conf().conf.fp32_train_conv == 'hip_x3'
    conf.update({'fp32_train_conv': 'cudnn'}, verbose=False)
    with pytest.raises(ValueError):
        conf()
    with pytest.raises(ValueError):
        pwc_modules.fp32_train_conv_mode('hip_x4')
    assert pwc_modules.FP32_TRAIN_CONV[0] == 'miopen'
    with pwc_modules.fp32_train_conv_mode('hip_x3'):
        assert pwc_modules.FP32_TRAIN_CONV[0] == 'hip_x3'
    assert pwc_modules.FP32_TRAIN_CONV[0] == 'miopen'


def test_x3_train_entries_are_bound_and_exported():
    from upflow_pytorch_amd import _lib, ops
    names = ('upf_act_grad_x3', 'upf_conv_x3_pack_weights_dgrad', 'upf_conv_x3_dgrad', 'upf_conv_x3_wgrad', 'upf_conv_x3_wgrad_workspace_bytes')
    for n in names:
        assert n in _lib.SIGNATURES
        assert getattr(_lib.lib(), n) is not None
    header = open(__import__('os').path.join(__import__('os').path.dirname(_lib._PKG), 'include', 'upflow_hip.h')).read()
    for n in names:
        assert n + '(' in header
    assert hasattr(ops, 'ConvX3TrainFunction') and callable(ops.conv_x3_train)


def test_x3_wgrad_workspace_query():
    """Partial blocks: at most 64 MB, at least one slice per level, an error for what the kernel does not take; tiny levels are accepted
    (no W >= 8 or even-size restriction)."""
    from upflow_pytorch_amd import _lib
    L = _lib.lib()

    def levels(*shapes):
        arr = (_lib.WgradLevel * len(shapes))()
        for a, (B, H, W) in zip(arr, shapes):
            a.x, a.grad_pre, a.B, a.H, a.W = 16, 16, B, H, W         # (never dereferenced by the query)
        return arr

    def query(arr, n, Cin, Cout, k, d, s):
        out = ctypes.c_longlong(-1)
        rc = L.upf_conv_x3_wgrad_workspace_bytes(arr, n, Cin, Cout, k, d, s, ctypes.byref(out))
        return out.value if rc == 0 else -1
    one = query(levels((8, 64, 208)), 1, 565, 128, 3, 1, 1)
    per_slice = 565 * 128 * 9 * 4
    assert one > 0 and one % per_slice == 0 and one <= (64 << 20) + per_slice
    tiny = query(levels((2, 2, 7), (2, 4, 13), (2, 1, 1)), 3, 35, 2, 3, 1, 1)
    assert tiny == 3 * 35 * 2 * 9 * 4                     # one slice per level
    assert query(levels((1, 13, 27)), 1, 32, 64, 3, 1, 2) > 0       # stride 2, odd sizes
    assert query(levels((1, 13, 27)), 1, 32, 64, 3, 2, 2) == -1     # stride 2 with dilation
    assert query(levels((1, 13, 27)), 1, 32, 64, 5, 1, 1) == -1
    assert query(levels(*[(1, 4, 4)] * 7), 7, 32, 64, 3, 1, 1) == -1
    assert query(None, 1, 32, 64, 3, 1, 1) == -1
    assert ctypes.sizeof(_lib.WgradLevel) == 48


# ---- the model of the split (tests/_x3_model.py) on every input of tests/test_hip_conv_x3_bwd_ops.py -------------------------------
# The model has no accumulation rounding: if IT breaks a bound of the GPU tests, the bound or the input is wrong.  The bar here is
# the GPU tests' with err32 = 0, i.e. its 3.0e-6 part alone.
def test_x3_model_scale_rule():
    import _x3_model as M
    for e in range(-126, 128):
        for frac in (1.0, 1.5, 1.9999999):
            m = float(torch.tensor(frac * 2.0 ** e, dtype=torch.float32)) if e < 127 or frac < 1.9 else 3.0e38
            sc = M.scale_of(m)
            assert sc == 2.0 ** round(torch.log2(torch.tensor(sc, dtype=torch.float64)).item())       # a power of two
            if -87 <= e <= 113:
                assert 2.0 ** 13 <= m * sc < 2.0 ** 14, (e, frac)
            else:
                assert sc == (2.0 ** 100 if e < 0 else 2.0 ** -100), (e, frac)                          # the clamp
    assert M.scale_of(2.0 ** -140) == 2.0 ** 100          # a subnormal maximum
    for bad in (0.0, float('inf'), float('nan'), 3.3e38):
        assert M.scale_of(bad) == 1.0
    # NaN elements do not define the scale; an infinite one does (scale 1)
    gy = torch.tensor([1.0, float('nan'), -3.0]).view(1, 3, 1, 1)
    assert M.act_grad(gy)[2] == 2.0 ** 12
    gy[0, 0] = float('inf')
    assert M.act_grad(gy)[2] == 1.0
    assert M.act_grad(torch.zeros(1, 3, 1, 1))[2] == 1.0


@pytest.mark.parametrize('conv,levels', __import__('_x3_model').A1_CASES)
def test_x3_model_multi_level_weight_gradient(conv, levels):
    import _x3_model as M
    Cin, Cout, k, d, s = M.A1_CONVS[conv]
    data = M.a1_inputs(conv, levels)
    shape = (Cout, Cin, k, k)
    for rot in range(len(data)):
        mags = M.a1_magnitudes(len(data), rot)
        lv = [(x, M.a1_grad_pre(gy, y, m)) for (x, gy, y), m in zip(data, mags)]
        gw, gb = M.wgrad(lv, shape, d, s)
        want_w = sum(torch.nn.grad.conv2d_weight(x.double(), shape, g.double(), stride=s, padding=d * (k - 1) // 2, dilation=d) for x, g in lv)
        want_b = sum(g.double().sum((0, 2, 3)) for _, g in lv)
        ew, eb = M.rel(gw, want_w), M.rel(gb, want_b)
        print('%s %s rot %d: model gw %.2e gb %.2e' % (conv, levels, rot, ew, eb))
        assert ew <= M.bar(0.0) and eb <= M.bar(0.0)
    # the NULL-slot mode on un-scaled O(1) gradients
    lv = [(x, M.a1_grad_pre(gy, y, 1.0)) for x, gy, y in data]
    gw, _ = M.wgrad(lv, shape, d, s, scaled=False)
    want_w = sum(torch.nn.grad.conv2d_weight(x.double(), shape, g.double(), stride=s, padding=d * (k - 1) // 2, dilation=d) for x, g in lv)
    assert M.rel(gw, want_w) <= M.bar(0.0)


@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('mag', __import__('_x3_model').A4_MAGS)
def test_x3_model_activation_magnitude_in_the_weight_gradient(mag, s):
    import _x3_model as M
    import torch.nn.functional as F
    x, w, b, gy = M.a4_inputs(mag, s)
    mask = F.conv2d(x.double(), w.double(), b.double(), padding=1, stride=s) > 0
    gpre = M.act_grad(gy, mask, M.A4_SLOPE)[0]
    gw, gb = M.wgrad([(x, gpre)], tuple(w.shape), 1, s)
    gx = M.dgrad(gpre, w, x.shape, 1, s)
    want_x, want_w, want_b = M.truth(x, w, gpre, 1, s)
    err = M.rel(gw, want_w)
    abs_err, floor = float((gw - want_w).abs().max()), M.a4_floor(gpre)
    print('|x| ~ %g stride %d: model gw err %.2e (absolute %.2e, floor %.2e)' % (mag, s, err, abs_err, floor))
    assert err <= M.bar(0.0) or abs_err <= floor
    if mag >= 1.0:
        assert err <= M.bar(0.0)
    assert M.rel(gx, want_x) <= M.bar(0.0) and M.rel(gb, want_b) <= M.bar(0.0)


@pytest.mark.parametrize('variant', __import__('_x3_model').A5_VARIANTS)
@pytest.mark.parametrize('layer', __import__('_x3_model').A5_LAYERS)
def test_x3_model_dynamic_range_inside_grad_y(layer, variant):
    import _x3_model as M
    import torch.nn.functional as F
    B, Cin, Cout, H, W, k, d, s = layer
    for r in M.A5_R:
        x, w, b, gy = M.a5_inputs(layer, variant, r)
        mask = F.conv2d(x.double(), w.double(), b.double(), padding=1, stride=s) > 0
        gpre = M.act_grad(gy, mask, M.A5_SLOPE)[0]
        gw, gb = M.wgrad([(x, gpre)], tuple(w.shape), d, s)
        gx = M.dgrad(gpre, w, x.shape, d, s)
        want_x, want_w, want_b = M.truth(x, w, gpre, d, s)
        floor_x, floor_w = M.a5_floors(x, w, gpre)
        for name, got, want in (('gx', gx, want_x), ('gw', gw, want_w), ('gb', gb, want_b)):
            assert M.rel(got, want) <= M.bar(0.0), (name, r)                  # the global bar
        part = M.a5_gx_part(layer, variant)
        if part is not None:
            M.a5_check('gx', gx[part], None, want_x[part], floor_x if s == 1 else 0.0, r, 'model %s' % variant)
            if r == 32:
                big = want_x[part].abs() > floor_x
                assert bool(big.any()) and bool((gx[part][big] != 0).all())
        else:
            h = Cout // 2
            M.a5_check('gw', gw[h:], None, want_w[h:], floor_w, r, 'model %s' % variant)
            M.a5_check('gb', gb[h:], None, want_b[h:], 0.0, r, 'model %s' % variant)
