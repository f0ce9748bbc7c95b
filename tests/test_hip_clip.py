"""Gradient-norm clipping and the gradient-norm statistic inside the optimizer step (csrc/optim.hip: sumsq_check_kernel,
norm_finish_kernel, the clipped Adam; optim.NativeAdam(max_grad_norm=...)) against the host model of the header's contract
(tests/_clip_model.py) and against torch's clip_grad_norm_ + Adam in fp64.

Tensor set: the one of tests/test_hip_optim.py (sizes 1, 2, 7, 33, 4097, 65537 and the 4-byte-offset view of 4099, gradients as
views into one bucket): both routes of the kernels, the ragged ends, a chunk boundary, more than one workgroup per tensor.  The
seeded gradients have a norm of about 25.6 (65537 elements of standard deviation 0.1 dominate: sqrt(65537) * 0.1 = 25.6), so a
bound of 1.0 clips and a bound of 1000.0 does not; every test asserts 20 < norm < 32 before it relies on that."""
import math

import numpy as np
import pytest
import torch

import _clip_model
import test_hip_optim as T

pytestmark = pytest.mark.gpu

trajectories = T.trajectories                      # (the module-scoped fixture: fp64 reference, torch fused, native — unclipped)
S16 = 2.0 ** 16


def _f32(t):
    """A device fp32 scalar as a numpy float32 (the same bits)."""
    return np.float32(t.detach().cpu().numpy())


def _one_step(max_norm, scale, step=0, groups=False):
    params = T.make_params()
    plist = [{'params': params[:3]}, {'params': params[3:]}] if groups else params
    opt = T.native(plist, loss_scale=scale, max_grad_norm=max_norm)
    grads = T.make_grads(step, scale=scale)
    kept = [g.clone() for g in grads]
    T.set_grads(params, grads)
    opt.step()
    model = _clip_model.norm64(kept, scale)
    assert 20.0 < model < 32.0
    assert all(torch.equal(p.grad.view(torch.int32), k.view(torch.int32)) for p, k in zip(params, kept)), 'p.grad is not modified'
    return opt, params, kept, model


@pytest.mark.parametrize('groups', [False, True])
@pytest.mark.parametrize('scale', [1.0, S16])
def test_norm_is_within_one_ulp_of_the_fp64_norm(scale, groups):
    """Bound (derived, not measured): the double accumulation's relative error is at most (chain length) * 2^-53 — 16384 / 256
    elements per thread, 8 tree levels, twice: < 200 * 2^-53 — and the double square root adds an ulp or two of double, all many
    orders below 2^-24; one rounding to fp32 of a value that close to the exact norm lands on float32(exact) or, at a rounding
    boundary, its neighbour: 1 ulp."""
    opt, params, kept, model = _one_step(1.0, scale, groups=groups)
    got = float(_f32(opt.grad_norm))
    ulp = float(np.spacing(np.float32(model)))
    # torch's own total, on copies of the un-scaled gradients (clip_grad_norm_ rescales them in place)
    copies = [torch.nn.Parameter(torch.zeros_like(p)) for p in params]
    T.set_grads(copies, [k / scale for k in kept])
    torch_total = float(torch.nn.utils.clip_grad_norm_(copies, 1.0))
    e_ours, e_torch = abs(got - model), abs(torch_total - model)
    print('grad norm, S = %g, %d group(s): fp64 model %.17g, device %.9g (error %.3g = %.3f ulp), torch clip_grad_norm_ %.9g (error %.3g)'
          % (scale, 2 if groups else 1, model, got, e_ours, e_ours / ulp, torch_total, e_torch))
    assert _clip_model.ulps32(got, np.float32(model)) <= 1.0
    assert e_ours <= max(e_torch, ulp)


@pytest.mark.parametrize('max_norm', [1.0, 1000.0, math.inf])
def test_coefficient_is_the_models_from_the_devices_own_norm(max_norm):
    opt, _, _, _ = _one_step(max_norm, S16)
    norm, coef = _f32(opt.grad_norm), _f32(opt.clip_coef)
    want = _clip_model.coef32(norm, max_norm)
    print('max_norm %g: norm %.9g, clip_coef %.9g, model %.9g' % (max_norm, norm, coef, want))
    assert coef.tobytes() == want.tobytes()
    if max_norm == 1.0:
        assert 0.0 < coef < 1.0
    else:
        assert coef == np.float32(1.0)


def test_clipped_adam_equals_unclipped_adam_on_gradients_times_the_coefficient():
    """Five steps with max_grad_norm = 1.0 and S = 2^16 on pre-scaled gradients == five unclipped native steps (S = 1) on gradients
    multiplied by that step's clip_coef with a torch fp32 multiply: g * 2^16 / 2^16 is g exactly, so both sides round g * coef once."""
    params = T.make_params()
    opt = T.native(params, loss_scale=S16, max_grad_norm=1.0)
    ref_params = T.make_params()
    ref = T.native(ref_params)
    for s in range(T.STEPS):
        T.set_grads(params, T.make_grads(s, scale=S16))
        opt.step()
        coef = opt.clip_coef.clone()
        assert 20.0 < float(opt.grad_norm) < 32.0 and 0.0 < float(coef) < 1.0
        T.set_grads(ref_params, [g * coef for g in T.make_grads(s)])
        ref.step()
    a, b = T.snapshot(opt, params), T.snapshot(ref, ref_params)
    assert a['step'] == [float(T.STEPS)] * len(params)
    assert T.bits_equal(a, b)
    assert int(opt.skipped_steps) == 0 and float(opt.loss_scale) == S16


@pytest.mark.parametrize('max_norm', [1000.0, math.inf])
def test_a_bound_that_does_not_bind_leaves_the_unclipped_bits(max_norm, trajectories):
    opt, _, out = T.run(lambda p: T.native(p, max_grad_norm=max_norm), torch.float32, T.STEPS, snaps=(5,))
    assert 20.0 < float(opt.grad_norm) < 32.0 and float(opt.clip_coef) == 1.0
    assert T.bits_equal(out[5], trajectories['native'][5])


class _ClipThenStep():
    """torch.nn.utils.clip_grad_norm_ then the optimizer's step (what T.run calls), the state visible to T.snapshot."""

    def __init__(self, opt, params, max_norm):
        self.opt, self.params, self.max_norm = opt, params, max_norm
        self.state = opt.state

    def step(self):
        torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
        self.opt.step()


def test_clipped_parity_with_fp64_within_twice_torchs_fp32_error():
    """Reference: clip_grad_norm_ on fp64 gradients, then torch.optim.Adam(amsgrad=True) in fp64.  torch's fp32 path: clip_grad_norm_
    plus fused Adam.  The bar is the one of test_adam_parity_with_fp64_within_twice_torchs_fused_error, for the same reason: the
    native step rounds where torch's fp32 kernel rounds, so its error is of torch's order, not below it."""
    ref = T.run(lambda p: _ClipThenStep(torch.optim.Adam(p, lr=T.LR, weight_decay=T.WD, amsgrad=True), p, 1.0),
                torch.float64, T.STEPS, snaps=(5,))[2][5]
    fused = T.run(lambda p: _ClipThenStep(torch.optim.Adam(p, lr=T.LR, weight_decay=T.WD, amsgrad=True, fused=True), p, 1.0),
                  torch.float32, T.STEPS, snaps=(5,))[2][5]
    opt, _, out = T.run(lambda p: T.native(p, max_grad_norm=1.0), torch.float32, T.STEPS, snaps=(5,))
    assert 20.0 < float(opt.grad_norm) < 32.0
    e_native, e_fused = T.worst_error(out[5], ref), T.worst_error(fused, ref)
    print('clipped Adam after %d steps, worst error vs fp64 relative to each tensor\'s maximum: native %.4g, torch clip + fused fp32 %.4g'
          % (T.STEPS, e_native, e_fused))
    assert out[5]['step'] == [float(T.STEPS)] * (len(T.SIZES) + 1)
    assert e_fused > 0 and e_native <= 2.0 * e_fused


@pytest.mark.parametrize('value', [float('inf'), float('nan')])
@pytest.mark.parametrize('site', ['first', 'last', 'before_boundary', 'after_boundary'])
def test_a_nonfinite_gradient_skips_the_clipped_step_and_shows_in_the_norm(site, value):
    ti, ei = T._poison_sites()[site]
    params = T.make_params()
    opt = T.native(params, loss_scale='dynamic', growth_interval=2000, max_grad_norm=1.0)
    T.set_grads(params, T.make_grads(0, scale=S16))
    opt.step()                                                   # a clean step first
    assert 20.0 < float(opt.grad_norm) < 32.0 and int(opt.skipped_steps) == 0
    before = T.snapshot(opt, params)
    grads = T.make_grads(1, scale=S16)
    grads[ti][ei] = value
    T.set_grads(params, grads)
    opt.step()
    assert T.bits_equal(T.snapshot(opt, params), before), 'a skipped step must leave parameters, moments, maximum and step counter alone'
    assert before['step'] == [1.0] * len(params)
    assert int(opt.skipped_steps) == 1 and int(opt._flag) == 0 and float(opt.loss_scale) == 2.0 ** 15
    assert not math.isfinite(float(opt.grad_norm)), 'the norm is non-finite if and only if the step was skipped'
    T.set_grads(params, T.make_grads(2, scale=2.0 ** 15))
    opt.step()                                                   # the next clean step applies and reports a finite norm
    after = T.snapshot(opt, params)
    assert after['step'] == [2.0] * len(params) and int(opt.skipped_steps) == 1
    assert 20.0 < float(opt.grad_norm) < 32.0
    assert all(not torch.equal(a, b) for a, b in zip(after['param'], before['param']))
    assert all(torch.isfinite(a).all() for a in after['param'])


def test_clipped_step_does_not_synchronise_and_replays_on_fresh_gradients():
    """The clipped step() only enqueues: it is captured (any host synchronisation is an error there) reading gradient storage that
    exists before the capture; three replays, each on fresh values copied into that storage, give the bits of the same steps run
    eagerly — parameters, state, norm and coefficient."""
    params = T.make_params()
    opt = T.native(params, loss_scale=S16, max_grad_norm=1.0)
    T.set_grads(params, T.make_grads(0, scale=S16))
    opt.step()                                                   # eager warm-up: state, tables and partials exist before the capture
    where = (opt._partials.data_ptr(), opt.grad_norm.data_ptr(), opt.clip_coef.data_ptr())
    static = T.make_grads(1, scale=S16)
    T.set_grads(params, static)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    assert where == (opt._partials.data_ptr(), opt.grad_norm.data_ptr(), opt.clip_coef.data_ptr())
    assert T.snapshot(opt, params)['step'] == [1.0] * len(params)        # (the capture itself executed nothing)
    ref_params = T.make_params()
    ref = T.native(ref_params, loss_scale=S16, max_grad_norm=1.0)
    T.set_grads(ref_params, T.make_grads(0, scale=S16))
    ref.step()
    for s in (1, 2, 3):
        for dst, src in zip(static, T.make_grads(s, scale=S16)):
            dst.copy_(src)
        graph.replay()
        T.set_grads(ref_params, T.make_grads(s, scale=S16))
        ref.step()
        torch.cuda.synchronize()
        assert _f32(opt.grad_norm).tobytes() == _f32(ref.grad_norm).tobytes() and 20.0 < float(opt.grad_norm) < 32.0
        assert _f32(opt.clip_coef).tobytes() == _f32(ref.clip_coef).tobytes()
        a, b = T.snapshot(opt, params), T.snapshot(ref, ref_params)
        assert a['step'] == [float(s + 1)] * len(params)
        assert T.bits_equal(a, b), 'replay %d' % s


def test_raw_clip_launches_reject_bad_arguments():
    import ctypes
    from upflow_pytorch_amd import _lib, ops
    dev = torch.device('cuda')
    t = ops.MtTables([4, 5])
    flag = torch.zeros((), dtype=torch.int32, device=dev)
    partials = torch.zeros(2, dtype=torch.float64, device=dev)
    one = torch.ones((), dtype=torch.float32, device=dev)
    norm, coef = torch.zeros_like(one), torch.zeros_like(one)
    with pytest.raises(ops.UpflowHipError):                                     # the gradients were never set
        ops.grads_sumsq_check(t, partials, flag)
    grads = [torch.zeros(4, device=dev), torch.zeros(5, device=dev)]           # (kept alive: the table holds addresses only)
    t.set('grad', grads)
    for bad in (partials[:1], partials.float(), partials.cpu(), None):          # too short, not fp64, not on the GPU, missing
        with pytest.raises(ops.UpflowHipError):
            ops.grads_sumsq_check(t, bad, flag)
    with pytest.raises(ops.UpflowHipError):
        ops.grads_sumsq_check(t, partials, flag.float())
    with pytest.raises(ops.UpflowHipError):                                     # the other four lists were never set
        ops.adam_amsgrad_step(t, one, one, one, flag, 0.9, 0.999, 1e-8, 0.0, clip_coef=one)
    for bad in (dict(partials=partials[:0]), dict(partials=partials.float()), dict(norm_out=norm.double()), dict(coef_out=coef.cpu()),
                dict(loss_scale=1.0), dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=float('nan'))):
        kw = dict(dict(partials=partials, loss_scale=one, max_norm=1.0, norm_out=norm, coef_out=coef), **bad)
        with pytest.raises(ops.UpflowHipError):
            ops.grad_norm_clip_coef(**kw)
    # the entry points themselves: null pointers, n_partials <= 0
    stream, null = _lib.stream_ptr(dev), ctypes.c_void_p(0)
    L = t.launches[0][0]
    p, f, o, n, c = (_lib.ptr(x) for x in (partials, flag, one, norm, coef))
    for args in ((null, p, f), (ctypes.byref(L), null, f), (ctypes.byref(L), p, null)):
        with pytest.raises(ops.UpflowHipError):
            _lib.call('upf_grads_sumsq_check', *args, stream)
    for args in ((null, 2, o, 1.0, n, c), (p, 2, null, 1.0, n, c), (p, 2, o, 1.0, null, c), (p, 2, o, 1.0, n, null),
                 (p, 0, o, 1.0, n, c), (p, -1, o, 1.0, n, c)):
        with pytest.raises(ops.UpflowHipError):
            _lib.call('upf_grad_norm_clip_coef', *args, stream)
    with pytest.raises(ops.UpflowHipError):                                     # a null coefficient (before the table is looked at)
        _lib.call('upf_adam_amsgrad_step_clipped', ctypes.byref(L), o, o, o, null, f, 0.9, 0.999, 1e-8, 0.0, stream)
    with pytest.raises(ops.UpflowHipError):                                     # parameter / moment lists of the table not set
        _lib.call('upf_adam_amsgrad_step_clipped', ctypes.byref(L), o, o, o, o, f, 0.9, 0.999, 1e-8, 0.0, stream)
    # and what is accepted works: nothing above wrote anything
    assert ops.grads_sumsq_check(t, partials, flag) == 2
    ops.grad_norm_clip_coef(partials, one, 1.0, norm, coef)
    assert int(flag) == 0 and float(norm) == 0.0 and float(coef) == 1.0 and float(partials.abs().sum()) == 0.0


def _recorded_step(opt, monkeypatch):
    from upflow_pytorch_amd import _lib
    names = []
    real = _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', call)
    opt.step()
    monkeypatch.setattr(_lib, 'call', real)
    return names


def test_default_path_is_untouched(trajectories, monkeypatch):
    params = T.make_params()
    opt = T.native(params)
    assert opt.max_grad_norm is None and not hasattr(opt, 'clip_coef') and not hasattr(opt, 'grad_norm')
    for s in range(T.STEPS):
        T.set_grads(params, T.make_grads(s))
        names = _recorded_step(opt, monkeypatch)
        assert names == ['upf_grads_nonfinite_check', 'upf_adam_amsgrad_step', 'upf_loss_scale_update'], names
    assert T.bits_equal(T.snapshot(opt, params), trajectories['native'][5])
    # ... and the clipped step is the four launch families of the contract, the norm taken in the check's own pass
    opt = T.native(params, max_grad_norm=1.0)
    T.set_grads(params, T.make_grads(0))
    assert _recorded_step(opt, monkeypatch) == ['upf_grads_sumsq_check', 'upf_grad_norm_clip_coef', 'upf_adam_amsgrad_step_clipped',
                                                'upf_loss_scale_update']
    assert set(opt.state_dict()['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'}, 'the clip has no state'
