"""Trainer(loss_scale=...): the scaled training step (device scalar S seeds backward, optim.NativeAdam un-scales, checks, skips,
updates S) against the same golden vectors and bars as the unscaled step of tests/test_hip_train.py — eager, captured, with an
overflow inside the captured graph, and under DDP's bucket views."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _weights
from conftest import load_golden
from test_hip_train import FLAGS, _realistic_step, grad_direction_check

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
TERMS = ('photo_loss', 'smooth_loss', 'census_loss', 'msd_loss')


def make_net(mode, head_scale):
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    conf = UPFlow_net.config()
    d = dict(FLAGS)
    d.update(_weights.TRAIN_FLAGS)
    d['train_conv_dtype'] = mode
    conf.update(d, verbose=False)
    net = conf()
    net.load_state_dict(_weights.make_state_dict(0, head_scale=head_scale))
    return net


def scaled_realistic_step(mode, loss_scale):
    """Trainer steps on train_128x416_hs1 with a loss scale, up to the first step that is APPLIED -> (stats, names, UNSCALED gradients,
    the scale of that step, trainer).  A dynamic scale may start too high for the vector: a step whose gradients overflow changes no
    parameter and halves S, so the following step sees the same weights and the same batch at the lower scale — at most 16 halvings to
    the floor of 1.  The applied step leaves its scaled gradients in .grad; S is a power of two, so grad / S is exact."""
    from upflow_pytorch_amd.train import Trainer
    tr = Trainer(make_net(mode, 1.0), lr=1e-4, device=DEV, distributed=False, loss_scale=loss_scale)
    before = {n: p.detach().clone() for n, p in tr.raw_net.named_parameters()}
    batch = {k: v.cuda() for k, v in _weights.make_train_batch(**_weights.TRAIN_HS1).items()}
    params = dict(tr.raw_net.named_parameters())
    names = sorted(params)
    for i in range(18):
        S = float(tr.loss_scale)
        stats = tr.step(batch)
        assert set(stats) == {'loss', 'loss_scale', 'skipped_steps'} | set(TERMS)
        if stats['skipped_steps'] == i:                      # this step was applied
            break
        assert stats['skipped_steps'] == i + 1 and stats['loss_scale'] == max(S / 2, 1.0) and loss_scale == 'dynamic'
        assert all(torch.equal(params[n].detach(), before[n]) for n in names), 'a skipped step changes no parameter'
        assert all(np.isfinite(stats[k]) for k in ('loss',) + TERMS), 'the overflow is in the scaled gradients, not in the loss'
    assert stats['skipped_steps'] == i and stats['loss_scale'] == S == float(tr.loss_scale) and int(tr.skipped_steps) == i
    assert all(torch.isfinite(params[n].grad).all() for n in names)
    assert all(not torch.equal(params[n].detach(), before[n]) for n in names), 'the applied step updates every parameter'
    return stats, names, {n: params[n].grad / S for n in names}, S, tr


def measures(names, grads, g):
    got = np.array([float(grads[n].norm()) for n in names])
    want = g['grad_norms'].numpy()
    rel = np.abs(got - want) / np.maximum(want, 1e-3)
    cos, worst = grad_direction_check(grads, g)
    return got, rel, cos, worst


def test_fp32_mode_with_a_fixed_scale_meets_the_unscaled_bars():
    from upflow_pytorch_amd.train import Trainer
    g = load_golden('train_128x416_hs1')
    stats, names, grads, S, tr = scaled_realistic_step('fp32', 2.0 ** 10)
    assert S == 2.0 ** 10 and stats['skipped_steps'] == 0
    got, rel, cos, worst = measures(names, grads, g)
    print('realistic motion, fp32, S = 2^10: max rel grad-norm error %.3g (param %s), min cosine %.7f, worst bias-gradient error %.3g'
          % (rel.max(), names[int(rel.argmax())], cos.min(), worst))
    # the bars of test_train_step_at_realistic_motion_matches_reference
    assert (got > 0).all() and rel.max() <= 1e-2 and cos.min() >= 0.9999 and worst <= 1.5e-2
    for k in TERMS:
        assert abs(stats[k] - float(g[k])) <= 2e-4 * max(1.0, abs(float(g[k]))), k
    # the reported loss is the UNSCALED loss: the unscaled trainer's, to 1e-6 relative
    plain = Trainer(make_net('fp32', 1.0), lr=1e-4, device=DEV, distributed=False)
    batch = {k: v.cuda() for k, v in _weights.make_train_batch(**_weights.TRAIN_HS1).items()}
    want = plain.step(batch)
    assert set(want) == {'loss'} | set(TERMS)
    print('loss: scaled run %.9g, unscaled run %.9g' % (stats['loss'], want['loss']))
    assert abs(stats['loss'] - want['loss']) <= 1e-6 * abs(want['loss'])


def test_fp16_mode_with_the_dynamic_scale_meets_the_tight_bars():
    """loss_scale='dynamic' on the vector of test_fp16_training_mode_at_realistic_motion_meets_the_tight_bars, same bars, next to the unscaled
    fp16 step computed here.  Measured on MI355X (printed below): 2^16 overflows on this vector — three steps are skipped, the first
    applied step runs at S = 2^13: norm error max 2.49 % / median 0.46 %, cosine min 0.99587 / median 0.99976, loss terms 9e-5; unscaled: 2.78 % /
    0.75 %, 0.99609 / 0.99972 (the coarsest levels' gradients are not reproducible run to run, so the figures move in the third digit)."""
    g = load_golden('train_128x416_hs1')
    stats, names, grads, S, tr = scaled_realistic_step('fp16', 'dynamic')
    print('dynamic scale on this vector: started at 2^16, %d steps skipped, first applied step at S = 2^%d' % (stats['skipped_steps'], int(np.log2(S))))
    got, rel, cos, worst = measures(names, grads, g)
    lrel = {k: abs(stats[k] - float(g[k])) / max(1.0, abs(float(g[k]))) for k in TERMS}
    # the unscaled fp16 step, the same way
    _, _, names1, params1 = _realistic_step('fp16')
    assert names1 == names
    got1, rel1, cos1, _ = measures(names, {n: params1[n].grad for n in names}, g)
    print('realistic motion, fp16, dynamic S: max rel grad-norm error %.4g median %.4g, cosine min %.6f median %.6f, loss terms rel. error max %.5f'
          % (rel.max(), np.median(rel), cos.min(), np.median(cos), max(lrel.values())))
    print('realistic motion, fp16, unscaled : max rel grad-norm error %.4g median %.4g, cosine min %.6f median %.6f'
          % (rel1.max(), np.median(rel1), cos1.min(), np.median(cos1)))
    # the bars of test_fp16_training_mode_at_realistic_motion_meets_the_tight_bars
    assert max(lrel.values()) <= 1e-3
    assert rel.max() <= 0.06 and cos.min() >= 0.97 and np.median(cos) >= 0.998


# (mode, replayed steps): warm-up plus 4 replayed steps; the fp16 mode gets 5 more, because on this vector every one of the first
# seven steps overflows (S walks down from 2^16 to 2^9 inside the captured graph) and seven skipped steps compare no parameter update.
# Five APPLIED steps at the most either way: the parameter tolerance below is the one of the five-step test it comes from.
@pytest.mark.parametrize('mode,replays', [('fp32', 4), ('fp16', 9)])
def test_graphed_scaled_step_equals_eager(mode, replays):
    """Warm-up plus `replays` replayed steps with growth_interval = 2 (S halves and doubles inside the captured graph) against the eager
    trainer, with the tolerances of test_graphed_training_step_equals_eager; the scale and the skip count must be EQUAL at every step."""
    from upflow_pytorch_amd.train import Trainer
    batch = {k: v.cuda() for k, v in _weights.make_train_batch().items()}
    res = []
    for graph in (False, False, True):
        tr = Trainer(make_net(mode, 0.1), lr=1e-4, device=DEV, distributed=False, graph=graph, loss_scale='dynamic', growth_interval=2)
        stats = [tr.step(batch) for _ in range(tr.graph_warmup + replays)]
        assert (tr._graph is not None) == graph and not tr.capture_fallback
        res.append((stats, {n: p.detach().clone() for n, p in tr.raw_net.named_parameters()}))
    (s0, p0), (_, pe), (s1, p1) = res
    print('scale / skipped per step (%s): %s' % (mode, [(a['loss_scale'], a['skipped_steps']) for a in s1]))
    for a, b in zip(s0, s1):
        assert a['loss_scale'] == b['loss_scale'] and a['skipped_steps'] == b['skipped_steps'], (a, b)
        for k in a:
            assert abs(a[k] - b[k]) <= 1e-2 * max(1.0, abs(a[k])), (k, a[k], b[k])
    applied = [i for i in range(len(s1)) if s1[i]['skipped_steps'] == (s1[i - 1]['skipped_steps'] if i else 0)]
    assert len([i for i in applied if i >= 3]) >= 2, 'replayed steps must have been applied, not only skipped: %s' % applied
    assert len(applied) <= 5, applied
    assert len({a['loss_scale'] for a in s1[3:]}) > 1, 'the scale must have moved inside the captured step'
    diff = lambda u, v: (max(float((u[n] - v[n]).abs().max()) for n in u),
                         sum(float((u[n] - v[n]).abs().sum()) for n in u) / sum(u[n].numel() for n in u))
    (worst, mean), (noise_worst, noise_mean) = diff(p0, p1), diff(p0, pe)
    print('graphed vs eager after the scaled steps (%s): parameter difference worst %.3g mean %.3g; eager vs eager worst %.3g mean %.3g'
          % (mode, worst, mean, noise_worst, noise_mean))
    assert worst <= 1e-3 and mean <= max(3.0 * noise_mean, 2e-5), (worst, mean, noise_worst, noise_mean)


def test_overflow_inside_the_captured_graph_skips_that_replay_only():
    """One inf in im1_raw of a REPLAYED step (no re-capture): an ordinary non-finite input — the loss and the gradients are non-finite,
    the check inside the graph sees it, the Adam launches write nothing, S is halved; the next clean replay trains on."""
    from upflow_pytorch_amd.train import Trainer
    batch = {k: v.cuda() for k, v in _weights.make_train_batch().items()}
    tr = Trainer(make_net('fp16', 0.1), lr=1e-4, device=DEV, distributed=False, graph=True, loss_scale='dynamic')
    # the dynamic scale settles first — on this vector 2^16 overflows, and the steps that halve it are replays already
    skipped = 0
    for i in range(tr.graph_warmup + 20):
        stats = tr.step(batch)
        if i >= tr.graph_warmup and stats['skipped_steps'] == skipped:
            break
        skipped = stats['skipped_steps']
    assert tr._graph is not None and stats['skipped_steps'] == skipped, 'no step was applied: %r' % (stats,)
    S = stats['loss_scale']
    print('settled: %d steps skipped, S = 2^%d' % (skipped, int(np.log2(S))))
    assert S >= 2.0
    graph = tr._graph
    snap = lambda: {n: p.detach().clone() for n, p in tr.raw_net.named_parameters()}
    opt_state = lambda: [tr.optimizer.state[p][k].detach().clone() for p in tr.optimizer.param_groups[0]['params']
                         for k in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq', 'step')]
    before, st_before = snap(), opt_state()
    bad = dict(batch)
    bad['im1_raw'] = batch['im1_raw'].clone()
    bad['im1_raw'][0, 1, 40, 60] = float('inf')
    stats = tr.step(bad)
    assert tr._graph is graph, 'the step must have been a replay of the same graph'
    after = snap()
    assert all(torch.equal(after[n].view(torch.int32), before[n].view(torch.int32)) for n in before), 'a skipped replay must not touch a parameter'
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(opt_state(), st_before))
    assert stats['skipped_steps'] == skipped + 1 and int(tr.skipped_steps) == skipped + 1
    assert stats['loss_scale'] == S / 2 and float(tr.loss_scale) == S / 2
    stats = tr.step(batch)
    assert tr._graph is graph
    final = snap()
    assert all(np.isfinite(v) for v in stats.values()) and stats['skipped_steps'] == skipped + 1 and stats['loss_scale'] == S / 2
    assert all(torch.isfinite(final[n]).all() for n in final)
    assert sum(not torch.equal(final[n], before[n]) for n in before) == 80, 'the next clean replay updates every parameter'


def test_scaled_trainer_takes_a_native_adam_only():
    from upflow_pytorch_amd.optim import NativeAdam
    from upflow_pytorch_amd.train import Trainer
    tr = Trainer(make_net('fp16', 0.1), lr=1e-4, device=DEV, distributed=False, loss_scale='dynamic')
    params = [p for p in tr.raw_net.parameters()]
    with pytest.raises(TypeError):
        tr.optimizer = torch.optim.Adam(params, lr=1e-4, amsgrad=True, fused=True)
    new = NativeAdam(params, lr=1e-4, weight_decay=1e-4, loss_scale=256.0)
    tr.optimizer = new
    assert tr.loss_scale is new.loss_scale and tr.skipped_steps is new.skipped_steps and getattr(new, '_upf_version_hook', None) is not None


def test_scaled_trainer_under_rccl_ddp_bucket_views():
    """The 1-rank RCCL DDP + hipGraph run of test_trainer_under_rccl_ddp_real_net with loss_scale='dynamic' (its own process:
    tests/_ddp_one_rank_loss_scale.py): the gradients NativeAdam reads are views into DDP's bucket."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, '_ddp_one_rank_loss_scale.py')], capture_output=True, text=True, timeout=900)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stderr[-4000:]
    assert 'DDP-ONE-RANK-LOSS-SCALE-OK' in out.stdout
