"""Loss variants without a GPU: the package's torch spellings against fixtures recorded from the reference's own functions
(tests/golden/lossvar_*.npz, make_golden_loss_variants.py), the C ABI of csrc/loss_variants.hip (upf_pointwise_loss_*: csrc/loss.hip), and the CPU routing."""
import ctypes

import pytest
import torch

import _lossvar as lv
from conftest import load_golden

NEW_SYMBOLS = ['upf_smooth_edge2_forward', 'upf_smooth_edge2_backward', 'upf_smooth_delta_forward', 'upf_smooth_delta_backward',
               'upf_pointwise_loss_forward', 'upf_pointwise_loss_backward', 'upf_ssim_forward', 'upf_ssim_backward']


def _nt():
    from upflow_pytorch_amd.model.upflow import network_tools
    return network_tools


def _run(fn, inputs, diff, dtype):
    xs = [t.to(dtype).clone().requires_grad_(i in diff) for i, t in enumerate(inputs)]
    v = fn(*xs)
    return v.detach(), [g.detach() for g in torch.autograd.grad(v, [xs[i] for i in diff])]


def _against_fixture(g, key, fn, inputs, diff, names):
    """The spelling in fp64 reproduces the reference's fp64 record; in fp32 it meets the error rule with the reference's fp32 record
    as the torch composition."""
    v64, gs64 = _run(fn, inputs, diff, torch.float64)
    v32, gs32 = _run(fn, inputs, diff, torch.float32)
    assert lv.relerr(v64, g['%s_val64' % key]) <= 1e-12, key
    lv.check(key + ' value', v32, g['%s_val32' % key], g['%s_val64' % key])
    for n, a64, a32 in zip(names, gs64, gs32):
        assert lv.relerr(a64, g['%s_g%s64' % (key, n)]) <= 1e-12, (key, n)
        lv.check('%s grad %s' % (key, n), a32, g['%s_g%s32' % (key, n)], g['%s_g%s64' % (key, n)])


@pytest.mark.parametrize('i', range(len(lv.FIXTURE_SHAPES)))
def test_edge2_torch_spelling_matches_the_reference(i):
    g = load_golden('lossvar_edge2_%d' % i)
    _against_fixture(g, 'edge2', lambda a, b: _nt()._edge_aware_smoothness_order2_torch(a, b), [g['img'], g['pred']], [1], ['pred'])


@pytest.mark.parametrize('i', range(len(lv.FIXTURE_SHAPES)))
def test_delta_torch_spelling_matches_the_reference(i):
    from upflow_pytorch_amd.utils.loss import loss_functions
    g = load_golden('lossvar_delta_%d' % i)
    for name in ('flow', 'pc'):
        for order in (1, 2):
            _against_fixture(g, '%s_o%d' % (name, order), lambda a, o=order: loss_functions._flow_smooth_delta_torch(a, o == 2),
                             [g[name]], [0], ['flow'])


@pytest.mark.parametrize('i', range(len(lv.FIXTURE_SHAPES)))
def test_pointwise_torch_spelling_matches_the_reference(i):
    g = load_golden('lossvar_pointwise_%d' % i)
    B, _, H, W = g['x'].shape
    occs = {'none': None, 'binary': g['occ_binary'], 'zero': torch.zeros(B, 1, H, W)}
    for kind in ('charbonnier', 'L1'):
        for oname, occ in occs.items():
            def fn(a, b, kind=kind, occ=occ):
                o = torch.ones(B, 1, H, W, dtype=a.dtype) if occ is None else occ.to(a.dtype)
                return _nt()._photo_loss_multi_type_torch(a, b, o, kind, 0.4, occ is not None)
            _against_fixture(g, '%s_%s' % (kind, oname), fn, [g['x'], g['y']], [0, 1], ['x', 'y'])


@pytest.mark.parametrize('i', range(len(lv.FIXTURE_SHAPES)))
def test_ssim_torch_spelling_matches_the_reference(i):
    g = load_golden('lossvar_ssim_%d' % i)
    x, y, w, G = g['x'], g['y'], g['weight'], g['G']
    nt = _nt()
    m64, wa64 = nt._weighted_ssim_torch(x.double(), y.double(), w.double())
    m32, wa32 = nt._weighted_ssim_torch(x, y, w)
    assert lv.relerr(m64, g['map64']) <= 1e-12 and lv.relerr(wa64, g['wavg64']) <= 1e-12
    lv.check('map', m32, g['map32'], g['map64'])
    lv.check('w_avg', wa32, g['wavg32'], g['wavg64'])
    _against_fixture(g, 'map', lambda a, b: (nt._weighted_ssim_torch(a, b, w.to(a.dtype))[0] * G.to(a.dtype)).sum(), [x, y], [0, 1], ['x', 'y'])
    for use_occ in (True, False):
        _against_fixture(g, 'photo_occ%d' % use_occ,
                         lambda a, b, u=use_occ: nt._photo_loss_multi_type_torch(a, b, w.to(a.dtype), 'SSIM', 0.4, u), [x, y], [0, 1], ['x', 'y'])


def test_library_exports_and_binds_the_loss_variant_entry_points():
    import __graft_entry__ as g
    g.build()
    from upflow_pytorch_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), 'missing symbol %s' % n
        assert n in _lib.SIGNATURES, 'unbound symbol %s' % n
        assert getattr(_lib.lib(), n).argtypes == _lib.SIGNATURES[n]


def test_cpu_tensors_take_the_torch_spelling(monkeypatch):
    """CPU tensors behave as before: the public functions never reach the native operators and equal the private spellings."""
    from upflow_pytorch_amd import ops
    from upflow_pytorch_amd.utils.loss import loss_functions

    def boom(*a, **k):
        raise AssertionError('native operator called on a CPU tensor')
    for name in ('smooth_edge2', 'smooth_delta', 'pointwise_loss_sums', 'weighted_ssim', 'ssim_loss_sums'):
        assert callable(getattr(ops, name))
        monkeypatch.setattr(ops, name, boom)
    nt = _nt()
    shape = (2, 3, 9, 11)
    x, y, w = lv.ssim_inputs(shape, 1)
    flow = lv.flow_inputs((2, 2, 9, 11), 2)
    assert torch.equal(nt.edge_aware_smoothness_order2(x, flow), nt._edge_aware_smoothness_order2_torch(x, flow))
    for second in (False, True):
        assert torch.equal(nt.flow_smooth_delta(flow, second), loss_functions._flow_smooth_delta_torch(flow, second))
        assert torch.equal(loss_functions.flow_smooth_delta(flow, second), loss_functions._flow_smooth_delta_torch(flow, second))
    m, wa = nt.weighted_ssim(x, y, w)
    m0, wa0 = nt._weighted_ssim_torch(x, y, w)
    assert torch.equal(m, m0) and torch.equal(wa, wa0)
    for kind in ('charbonnier', 'L1', 'SSIM'):
        for use_occ in (False, True):
            assert torch.equal(nt.photo_loss_multi_type(x, y, w, kind, 0.4, use_occ), nt._photo_loss_multi_type_torch(x, y, w, kind, 0.4, use_occ))
    with pytest.raises(ValueError):
        nt.photo_loss_multi_type(x, y, w, 'nope')
    with pytest.raises(ValueError):
        nt.weighted_ssim(x, y, w, c1=float('inf'), c2=float('inf'))
