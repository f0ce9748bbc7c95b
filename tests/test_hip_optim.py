"""The device-resident optimizer step (csrc/optim.hip, optim.NativeAdam): Adam + amsgrad + L2 against torch's own formulas in
fp64, the exact division by a power-of-two loss scale, the skipped step on a non-finite gradient wherever it sits, the scale's
state machine against tests/_amp_model.py, and state-dict interchange with torch.optim.Adam in both directions.

Tensor set: sizes 1, 2, 7, 33, 4097, 65537 (four chunks and one element) plus a parameter that is a 4-byte-offset view
(buf[1:]); the gradients are views into ONE flat bucket at offsets 1, 3, 10, 43, ... elements — 4-byte aligned only, as DDP's
bucket views are — so both the float4 and the element-by-element routes of the kernels run, and their ragged ends."""
import copy

import pytest
import torch

import _amp_model

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 7, 33, 4097, 65537]
VIEW = 4099
LR, WD, STEPS = 1e-3, 1e-4, 5
KEYS = ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')


def make_params(dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    vals = [torch.randn(n, generator=g) for n in SIZES + [VIEW]]
    params = [torch.nn.Parameter(v.to('cuda', dtype)) for v in vals[:-1]]
    buf = torch.zeros(VIEW + 1, device='cuda', dtype=dtype)
    buf[1:] = vals[-1].to('cuda', dtype)
    params.append(torch.nn.Parameter(buf[1:]))
    assert params[-1].data_ptr() % 16 == buf.element_size()
    return params


def make_grads(step, dtype=torch.float32, scale=1.0):
    """Seeded gradients of step `step` as views into one flat bucket (fp32 values; `scale` a power of two: exact)."""
    g = torch.Generator().manual_seed(1000 + step)
    flat = torch.cat([torch.randn(n, generator=g) * (0.01 * 10.0 ** (i % 3 - 1)) for i, n in enumerate(SIZES + [VIEW])]) * scale
    return list(flat.to('cuda', dtype).split(SIZES + [VIEW]))


def set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = g


def snapshot(opt, params):
    s = {'param': [p.detach().clone() for p in params]}
    for k in KEYS:
        s[k] = [opt.state[p][k].detach().clone() for p in params]
    s['step'] = [float(opt.state[p]['step']) for p in params]
    return s


def worst_error(got, ref):
    """Worst error over the parameters and the three state tensors, relative to each tensor's maximum in the fp64 reference."""
    worst = 0.0
    for k in ('param',) + KEYS:
        for a, r in zip(got[k], ref[k]):
            worst = max(worst, float((a.double() - r).abs().max() / r.abs().max().clamp_min(1e-300)))
    return worst


def bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for k in ('param',) + KEYS for x, y in zip(a[k], b[k])) \
        and a['step'] == b['step']


def native(params, **kw):
    from upflow_pytorch_amd.optim import NativeAdam
    return NativeAdam(params, lr=LR, weight_decay=WD, amsgrad=True, **kw)


def run(make_opt, dtype, nsteps, scale=1.0, first=0, snaps=()):
    params = make_params(dtype)
    opt = make_opt(params)
    out = {}
    for s in range(first, first + nsteps):
        set_grads(params, make_grads(s, dtype, scale))
        opt.step()
        if s + 1 in snaps:
            out[s + 1] = snapshot(opt, params)
    return opt, params, out


@pytest.fixture(scope='module')
def trajectories():
    """fp64 reference (torch.optim.Adam on float64 copies), torch's fp32 fused Adam and the native step, snapshots after 3 and 5 steps."""
    t = {}
    t['ref'] = run(lambda p: torch.optim.Adam(p, lr=LR, weight_decay=WD, amsgrad=True), torch.float64, STEPS, snaps=(2, 3, 5))[2]
    t['fused'] = run(lambda p: torch.optim.Adam(p, lr=LR, weight_decay=WD, amsgrad=True, fused=True), torch.float32, STEPS, snaps=(3, 5))[2]
    t['native'] = run(lambda p: native(p), torch.float32, STEPS, snaps=(2, 3, 5))[2]
    return t


def test_adam_parity_with_fp64_within_twice_torchs_fused_error(trajectories):
    t = trajectories
    e_native, e_fused = worst_error(t['native'][5], t['ref'][5]), worst_error(t['fused'][5], t['ref'][5])
    print('Adam parity after %d steps, worst error vs fp64 relative to each tensor\'s maximum: native %.4g, torch fused fp32 %.4g'
          % (STEPS, e_native, e_fused))
    assert t['native'][5]['step'] == [float(STEPS)] * (len(SIZES) + 1)
    assert e_fused > 0 and e_native <= 2.0 * e_fused


def test_unscale_by_a_power_of_two_is_exact(trajectories):
    """The same gradients pre-multiplied by 2^16, run with S = 2^16: identical bits in every parameter and state tensor."""
    opt, params, out = run(lambda p: native(p, loss_scale=2.0 ** 16), torch.float32, STEPS, scale=2.0 ** 16, snaps=(5,))
    assert bits_equal(out[5], trajectories['native'][5])
    assert float(opt.loss_scale) == 2.0 ** 16 and int(opt.skipped_steps) == 0


def _poison_sites():
    from upflow_pytorch_amd import ops
    big = SIZES.index(65537)
    assert 65537 > ops.MT_CHUNK + 1
    return {'first': (0, 0), 'last': (len(SIZES), VIEW - 1), 'before_boundary': (big, ops.MT_CHUNK - 1), 'after_boundary': (big, ops.MT_CHUNK)}


@pytest.mark.parametrize('value', [float('inf'), float('nan')])
@pytest.mark.parametrize('site', ['first', 'last', 'before_boundary', 'after_boundary'])
def test_a_nonfinite_gradient_skips_the_step(site, value):
    ti, ei = _poison_sites()[site]
    params = make_params()
    opt = native(params, loss_scale='dynamic', growth_interval=2000)
    seq = []

    def state():
        return (float(opt.loss_scale), int(opt.growth_tracker), int(opt.skipped_steps))
    set_grads(params, make_grads(0, scale=2.0 ** 16))
    opt.step()                                                   # a clean step first: moments, maximum and counter are non-trivial
    seq.append(state())
    before = snapshot(opt, params)
    grads = make_grads(1, scale=2.0 ** 16)
    grads[ti][ei] = value
    set_grads(params, grads)
    opt.step()
    seq.append(state())
    assert bits_equal(snapshot(opt, params), before), 'a skipped step must leave parameters, moments, maximum and step counter alone'
    assert before['step'] == [1.0] * len(params)
    assert int(opt._flag) == 0, 'the flag is cleared again'
    assert seq[-1] == (2.0 ** 15, 0, 1)
    set_grads(params, make_grads(2, scale=2.0 ** 15))
    opt.step()                                                   # the next clean step updates again
    seq.append(state())
    after = snapshot(opt, params)
    assert after['step'] == [2.0] * len(params)
    assert all(not torch.equal(a, b) for a, b in zip(after['param'], before['param']))
    assert seq == _amp_model.run([False, True, False], growth_interval=2000)


def test_a_fixed_scale_skips_and_counts_but_never_moves():
    params = make_params()
    opt = native(params, loss_scale=1024.0)
    pattern = [False, True, False]
    seq = []
    for s, bad in enumerate(pattern):
        grads = make_grads(s, scale=1024.0)
        if bad:
            grads[3][5] = float('inf')
        set_grads(params, grads)
        before = snapshot(opt, params) if s else None
        opt.step()
        seq.append((float(opt.loss_scale), int(opt.growth_tracker), int(opt.skipped_steps)))
        if bad:
            assert bits_equal(snapshot(opt, params), before)
    assert seq == _amp_model.run(pattern, scale=1024.0, dynamic=False)
    assert snapshot(opt, params)['step'] == [2.0] * len(params)


def test_scale_grows_after_growth_interval_clean_steps_and_follows_the_model():
    params = make_params()
    opt = native(params, loss_scale='dynamic', growth_interval=2)
    seq = []
    for s in range(4):
        set_grads(params, make_grads(s, scale=float(opt.loss_scale)))
        opt.step()
        seq.append((float(opt.loss_scale), int(opt.growth_tracker), int(opt.skipped_steps)))
    assert seq[-1][0] == 2.0 ** 18
    assert seq == _amp_model.run([False] * 4, growth_interval=2)
    # ... and a longer pattern with overflows, down to the floor of 1
    params = make_params()
    opt = native(params, loss_scale='dynamic', growth_interval=2)
    opt.load_scaler_state_dict({'loss_scale': 4.0, 'growth_tracker': 0, 'skipped_steps': 0})
    pattern = [True, True, True, False, False, True, False, False, False]
    seq = []
    for s, bad in enumerate(pattern):
        grads = make_grads(s, scale=float(opt.loss_scale))
        if bad:
            grads[-1][0] = float('nan')
        set_grads(params, grads)
        opt.step()
        seq.append((float(opt.loss_scale), int(opt.growth_tracker), int(opt.skipped_steps)))
    assert seq == _amp_model.run(pattern, scale=4.0, growth_interval=2)
    assert min(s[0] for s in seq) == 1.0


def test_state_dict_moves_to_torch_adam_and_back(trajectories):
    t = trajectories
    e_fused = worst_error(t['fused'][3], t['ref'][3])
    e_native = worst_error(t['native'][3], t['ref'][3])
    # native -> torch: two native steps, the state dict (through a copy, as a checkpoint is) into torch.optim.Adam, one step there
    opt, params, _ = run(lambda p: native(p), torch.float32, 2)
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'}
    ref_groups = torch.optim.Adam([torch.zeros(1)]).state_dict()['param_groups'][0]
    assert set(sd['param_groups'][0]) == set(ref_groups)
    topt = torch.optim.Adam(params, lr=LR, weight_decay=WD, amsgrad=True)
    topt.load_state_dict(sd)
    set_grads(params, make_grads(2))
    topt.step()
    mixed = snapshot(topt, params)
    e1 = worst_error(mixed, t['ref'][3])
    assert mixed['step'] == [3.0] * len(params)
    # torch -> native: two steps of torch's default Adam (host step counters), its state dict into NativeAdam, one native step
    topt, params, _ = run(lambda p: torch.optim.Adam(p, lr=LR, weight_decay=WD, amsgrad=True), torch.float32, 2)
    nopt = native(params)
    nopt.load_state_dict(copy.deepcopy(topt.state_dict()))
    set_grads(params, make_grads(2))
    nopt.step()
    mixed = snapshot(nopt, params)
    e2 = worst_error(mixed, t['ref'][3])
    assert mixed['step'] == [3.0] * len(params)
    print('state-dict interchange after 3 steps, worst error vs fp64: native->torch %.4g, torch->native %.4g; three native steps %.4g, '
          'three fused steps %.4g' % (e1, e2, e_native, e_fused))
    assert e_native <= 2.0 * e_fused and e1 <= 2.0 * e_fused and e2 <= 2.0 * e_fused
    # and NativeAdam's own round trip is exact
    opt, params, _ = run(lambda p: native(p), torch.float32, 2)
    opt2 = native(params)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    set_grads(params, make_grads(2))
    opt2.step()
    assert bits_equal(snapshot(opt2, params), t['native'][3])


def test_step_does_not_synchronise_and_advances_versions_through_the_hook():
    """step() only enqueues: it runs inside a hipGraph capture (where any host synchronisation is an error), with gradients at
    addresses allocated during the capture; the replay applies the update.  ops.register_version_hook works on it."""
    from upflow_pytorch_amd import ops
    params = make_params()
    opt = native(params, loss_scale='dynamic', growth_interval=2)
    assert ops.register_version_hook(opt) is not None
    set_grads(params, make_grads(0, scale=2.0 ** 16))
    v0 = params[0]._version
    opt.step()                                                   # eager warm-up: the state exists before the capture
    assert params[0]._version > v0
    static = [g.clone() for g in make_grads(1, scale=2.0 ** 16)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        set_grads(params, [s * 1.0 for s in static])            # gradients allocated by the capture's pool
        opt.step()
    before = snapshot(opt, params)                               # (the capture itself executed nothing)
    assert before['step'] == [1.0] * len(params)
    graph.replay()
    torch.cuda.synchronize()
    after = snapshot(opt, params)
    assert after['step'] == [2.0] * len(params) and float(opt.loss_scale) == 2.0 ** 17
    # the same two steps eagerly
    ref_opt, ref_params, _ = run(lambda p: native(p, loss_scale='dynamic', growth_interval=2), torch.float32, 1, scale=2.0 ** 16)
    set_grads(ref_params, make_grads(1, scale=2.0 ** 16))
    ref_opt.step()
    assert bits_equal(after, snapshot(ref_opt, ref_params))


def test_exponential_lr_updates_the_device_learning_rate_the_step_reads():
    """Graph mode's lr is a device tensor that the scheduler updates in place; the kernel reads it at every step.  With the same
    gradient twice and no weight decay the bias-corrected moments of step 2 equal those of step 1 (m^ = g, v^ = g^2), so halving
    lr halves the update."""
    from upflow_pytorch_amd.optim import NativeAdam
    params = make_params()
    lr = torch.tensor(LR, dtype=torch.float32, device='cuda')
    opt = NativeAdam(params, lr=lr, weight_decay=0.0)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5)
    where = lr.data_ptr()
    p0 = [p.detach().clone() for p in params]
    set_grads(params, make_grads(0))
    opt.step()
    p1 = [p.detach().clone() for p in params]
    sched.step()
    assert opt.param_groups[0]['lr'] is lr and lr.data_ptr() == where and float(lr) == float(torch.tensor(LR) * 0.5)
    set_grads(params, make_grads(0))
    opt.step()
    for a, b, c in zip(p0, p1, params):
        d1, d2 = (b - a).double(), (c.detach() - b).double()
        assert float(d1.abs().max()) > 0.5 * LR
        assert float((d2 - 0.5 * d1).abs().max()) <= 4e-7 * max(1.0, float(a.abs().max())), 'the second update is half the first'


def test_raw_launches_reject_bad_arguments():
    from upflow_pytorch_amd import ops
    t = ops.MtTables([4, 5])
    with pytest.raises(ops.UpflowHipError):
        t.set('grad', [torch.zeros(4), torch.zeros(5)])                        # CPU tensors: no CPU path
    with pytest.raises(ops.UpflowHipError):
        t.set('grad', [torch.zeros(4, device='cuda'), torch.zeros(6, device='cuda')])      # not the planned size
    with pytest.raises(ops.UpflowHipError):
        t.set('grad', [torch.zeros(4, device='cuda'), torch.zeros(10, device='cuda')[::2]])  # not contiguous
    t.set('grad', [torch.zeros(4, device='cuda'), torch.zeros(5, device='cuda')])
    flag = torch.zeros((), dtype=torch.int32, device='cuda')
    with pytest.raises(ops.UpflowHipError):                                     # the other four lists were never set
        ops.adam_amsgrad_step(t, flag.float(), flag.float(), flag.float() + 1, flag, 0.9, 0.999, 1e-8, 0.0)
    ops.grads_nonfinite_check(t, flag)
    assert int(flag) == 0
