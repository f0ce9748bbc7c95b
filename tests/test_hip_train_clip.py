"""Trainer(max_grad_norm=...): the bound on the global gradient norm and the 'grad_norm' statistic inside the training step — eager
against the host model of the contract (tests/_clip_model.py) on the gradients the step leaves in .grad, and captured against eager
with the bars of test_graphed_scaled_step_equals_eager, on its small network and batch."""
import math

import numpy as np
import pytest
import torch

import _clip_model
import _weights
import test_hip_train_loss_scale as LS

pytestmark = pytest.mark.gpu
DEV = LS.DEV
TERMS = set(LS.TERMS)


def _batch():
    return {k: v.cuda() for k, v in _weights.make_train_batch().items()}


def _trainer(mode, **kw):
    from upflow_pytorch_amd.train import Trainer
    return Trainer(LS.make_net(mode, 0.1), lr=1e-4, device=DEV, distributed=False, **kw)


def _model_norm(tr, scale):
    """The fp64 norm of p.grad / S as the step left it (the clip is folded into Adam's read: .grad holds the unclipped, scaled values)."""
    return _clip_model.norm64([p.grad for p in tr.raw_net.parameters() if p.grad is not None], scale)


def test_eager_clipped_trainer_reports_the_norm_and_clips():
    from upflow_pytorch_amd.optim import NativeAdam
    S = 2.0 ** 10
    batch = _batch()
    # measure only: the norm of the first step, which fixes the bound of the runs below
    tr = _trainer('fp32', loss_scale=S, max_grad_norm=math.inf)
    stats = tr.step(batch)
    assert set(stats) == {'loss', 'loss_scale', 'skipped_steps', 'grad_norm'} | TERMS
    assert list(stats)[-1] == 'grad_norm' and stats['skipped_steps'] == 0 and stats['loss_scale'] == S
    model = _model_norm(tr, S)
    print('first step, measure only: grad_norm %.9g, fp64 model of p.grad / S %.17g, clip_coef %r'
          % (stats['grad_norm'], model, float(tr.optimizer.clip_coef)))
    assert math.isfinite(model) and model > 0.0
    assert _clip_model.ulps32(stats['grad_norm'], np.float32(model)) <= 1.0
    assert float(tr.optimizer.clip_coef) == 1.0
    M = 0.5 * stats['grad_norm']
    # a bound that binds
    tr = _trainer('fp32', loss_scale=S, max_grad_norm=M)
    stats = tr.step(batch)
    assert set(stats) == {'loss', 'loss_scale', 'skipped_steps', 'grad_norm'} | TERMS
    model = _model_norm(tr, S)
    norm, coef = np.float32(stats['grad_norm']), np.float32(tr.optimizer.clip_coef.cpu().numpy())
    print('M = %.9g: grad_norm %.9g, model %.17g, clip_coef %.9g' % (M, norm, model, coef))
    assert _clip_model.ulps32(norm, np.float32(model)) <= 1.0
    assert float(tr.optimizer.grad_norm) == stats['grad_norm']
    assert 0.0 < coef < 1.0 and coef.tobytes() == _clip_model.coef32(norm, M).tobytes()
    # without a loss scale: NativeAdam at a fixed scale of 1, the old stat names plus 'grad_norm'
    tr = _trainer('fp32', max_grad_norm=M)
    stats = tr.step(batch)
    assert set(stats) == {'loss', 'grad_norm'} | TERMS
    assert type(tr.optimizer) is NativeAdam and float(tr.optimizer.loss_scale) == 1.0 and tr.loss_scale is None
    model = _model_norm(tr, 1.0)
    print('no loss scale: grad_norm %.9g, model %.17g, clip_coef %.9g' % (stats['grad_norm'], model, float(tr.optimizer.clip_coef)))
    assert _clip_model.ulps32(stats['grad_norm'], np.float32(model)) <= 1.0 and 0.0 < float(tr.optimizer.clip_coef) < 1.0
    # either option set: a NativeAdam only, and one that measures the norm
    params = list(tr.raw_net.parameters())
    with pytest.raises(TypeError):
        tr.optimizer = torch.optim.Adam(params, lr=1e-4, amsgrad=True, fused=True)
    with pytest.raises(TypeError):
        tr.optimizer = NativeAdam(params, lr=1e-4)
    new = NativeAdam(params, lr=1e-4, weight_decay=1e-4, max_grad_norm=M)
    tr.optimizer = new
    assert tr.optimizer is new and getattr(new, '_upf_version_hook', None) is not None


# (mode, replayed steps): warm-up plus 4 replays; the fp16 mode gets 5 more for the reason test_graphed_scaled_step_equals_eager
# gives: on this vector every one of the first seven steps overflows at the dynamic scale, and seven skipped steps compare no update
# and no finite norm.  Five applied steps at the most either way.
@pytest.mark.parametrize('mode,replays', [('fp32', 4), ('fp16', 9)])
def test_graphed_clipped_step_equals_eager(mode, replays):
    """Warm-up plus `replays` replayed steps with loss_scale='dynamic', growth_interval=2 and a bound of half the first applied
    step's norm, eager / eager / captured, with the bars of test_graphed_scaled_step_equals_eager: scale and skip count EQUAL at every
    step, every stat — 'grad_norm' among them — to 1e-2 relative, the parameters against the eager-vs-eager noise of the same run.
    'grad_norm' is finite exactly on the applied steps (the contract's if-and-only-if)."""
    batch = _batch()
    # the bound: half the norm of the first applied step of a measure-only run (skipped steps change no weight)
    tr = _trainer(mode, loss_scale='dynamic', growth_interval=2, max_grad_norm=math.inf)
    for i in range(18):
        first = tr.step(batch)
        if math.isfinite(first['grad_norm']):
            break
        assert first['skipped_steps'] == i + 1
    assert math.isfinite(first['grad_norm']) and first['grad_norm'] > 0.0 and first['skipped_steps'] == i
    M = 0.5 * first['grad_norm']
    res = []
    for graph in (False, False, True):
        tr = _trainer(mode, graph=graph, loss_scale='dynamic', growth_interval=2, max_grad_norm=M)
        stats = [tr.step(batch) for _ in range(tr.graph_warmup + replays)]
        assert (tr._graph is not None) == graph and not tr.capture_fallback
        res.append((stats, {n: p.detach().clone() for n, p in tr.raw_net.named_parameters()}))
    (s0, p0), (_, pe), (s1, p1) = res
    print('M = %.6g; scale / skipped / grad_norm per step (%s): %s'
          % (M, mode, [(a['loss_scale'], a['skipped_steps'], a['grad_norm']) for a in s1]))
    applied = [i for i in range(len(s1)) if s1[i]['skipped_steps'] == (s1[i - 1]['skipped_steps'] if i else 0)]
    for i, (a, b) in enumerate(zip(s0, s1)):
        assert set(a) == set(b) == {'loss', 'loss_scale', 'skipped_steps', 'grad_norm'} | TERMS
        assert a['loss_scale'] == b['loss_scale'] and a['skipped_steps'] == b['skipped_steps'], (a, b)
        assert math.isfinite(a['grad_norm']) == math.isfinite(b['grad_norm']) == (i in applied), (i, a, b)
        for k in a:
            if k == 'grad_norm' and i not in applied:
                continue                                         # (non-finite on both sides: checked above)
            assert abs(a[k] - b[k]) <= 1e-2 * max(1.0, abs(a[k])), (k, a[k], b[k])
    assert len([i for i in applied if i >= 3]) >= 2, 'replayed steps must have been applied, not only skipped: %s' % applied
    assert len(applied) <= 5, applied
    assert len({a['loss_scale'] for a in s1[3:]}) > 1, 'the scale must have moved inside the captured step'
    assert s1[applied[0]]['grad_norm'] > M, 'the bound must bind on the first applied step'
    diff = lambda u, v: (max(float((u[n] - v[n]).abs().max()) for n in u),
                         sum(float((u[n] - v[n]).abs().sum()) for n in u) / sum(u[n].numel() for n in u))
    (worst, mean), (noise_worst, noise_mean) = diff(p0, p1), diff(p0, pe)
    print('graphed vs eager after the clipped steps (%s): parameter difference worst %.3g mean %.3g; eager vs eager worst %.3g mean %.3g'
          % (mode, worst, mean, noise_worst, noise_mean))
    assert worst <= 1e-3 and mean <= max(3.0 * noise_mean, 2e-5), (worst, mean, noise_worst, noise_mean)
