"""The fp32 training step on the matrix cores: split-precision convolutions under autograd (ops.ConvX3TrainFunction,
csrc/conv_x3_bwd.hip; config `fp32_train_conv='hip_x3'`).

Yardstick of the operator tests = tests/test_hip_conv_x3.py's: fp64 conv2d autograd of the SAME fp32 operands is the truth, torch's own
fp32 gradient kernels (torch.nn.grad.conv2d_input / conv2d_weight: MIOpen) on those operands give the error to compare against.
Whole-step tests: the goldens and the bars of tests/test_hip_train.py's fp32 mode, unchanged."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
import _weights
from conftest import load_golden
from test_hip_conv_x3 import CASES
from test_hip_train import FLAGS, grad_direction_check

pytestmark = pytest.mark.gpu


def _flat_view(t, misalign):
    """A copy of `t` whose storage starts `misalign` floats after a 16-byte boundary."""
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = flat[misalign:misalign + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _grads(x, w, b, gy, d, s, slope, off=5, misalign=0):
    """(y, gx, gw, gb) of ops.conv_x3_train with x and grad_y as channel slices of wider buffers (x: `off` channels in, as
    test_hip_conv_x3._run; grad_y: 2 channels in); misalign: both buffers start that many floats off a 16-byte boundary."""
    from upflow_pytorch_amd import ops
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    ho, wo = ops.conv3x3_out_hw(H, W, s)
    xbuf = _flat_view(torch.zeros(B, Cin + off, H, W, device='cuda'), misalign)
    xbuf[:, off:] = x
    xbuf.requires_grad_(True)
    gbuf = _flat_view(torch.full((B, Cout + 3, ho, wo), 7.0, device='cuda'), misalign)
    gbuf[:, 2:2 + Cout] = gy
    wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = ops.conv_x3_train(xbuf[:, off:], wl, bl, d, slope, s)
    y.backward(gbuf[:, 2:2 + Cout])
    assert bool((xbuf.grad[:, :off] == 0).all()), 'data gradient outside the channel slice'
    return y.detach(), xbuf.grad[:, off:].clone(), wl.grad.clone(), bl.grad.clone()


def _rel(got, want):
    return float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize('case', CASES)
def test_conv_x3_gradients_are_fp32_class(case):
    """gx, gw, gb of one layer against fp64, max |got - fp64| / max |fp64|, beside the same figure for torch's fp32 gradient kernels.
    The LeakyReLU mask is taken from the layer's OWN forward output on all three sides (a pre-activation within rounding of zero
    may fall on either side of it; that is the forward's rounding, tested in test_hip_conv_x3.py): the truth is the fp64 gradient
    of the LINEAR convolution for grad_pre = grad_y * (y > 0 ? 1 : 0.1)."""
    B, Cin, Cout, H, W, k, d, s = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Cin, H, W, generator=g).cuda()
    w = (torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    pad = d * (k - 1) // 2
    ho, wo = (H - 1) // s + 1, (W - 1) // s + 1
    gy = torch.randn(B, Cout, ho, wo, generator=g).cuda()
    y, gx, gw, gb = _grads(x, w, b, gy, d, s, 0.1)
    gpre = gy * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.1))
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    F.conv2d(x64, w64, b64, padding=pad, dilation=d, stride=s).backward(gpre.double())
    gx32 = torch.nn.grad.conv2d_input(x.shape, w, gpre, stride=s, padding=pad, dilation=d)
    gw32 = torch.nn.grad.conv2d_weight(x, w.shape, gpre, stride=s, padding=pad, dilation=d)
    gb32 = gpre.sum((0, 2, 3))
    for name, got, ref32, want in (('gx', gx, gx32, x64.grad), ('gw', gw, gw32, w64.grad), ('gb', gb, gb32, b64.grad)):
        assert got.shape == want.shape and got.dtype == torch.float32
        err, err32 = _rel(got, want), _rel(ref32, want)
        print('%s %s: max err %.2e of max |.| (torch fp32: %.2e)' % (case, name, err, err32))
        # 3.0e-6 = the forward's bar (test_hip_conv_x3.py), 2.5 = that bar / MIOpen's 1.2e-6 there.  Measured on MI355X, maxima
        # over all cases, ours (torch fp32):  gx 9.9e-7 (1.1e-6), ours at (8,115,128,48,160);  gw 6.0e-7 (1.4e-6), both at
        # (4,96,32,96,320);  gb 3.2e-7 (1.7e-7), ours at (1,35,2,5,9).  Worst case: 0.33 of its bound.
        assert err <= max(3.0e-6, 2.5 * err32), (name, err, err32)


@pytest.mark.parametrize('case', [(2, 115, 128, 24, 40, 3, 1, 1), (2, 16, 32, 32, 64, 3, 1, 2), (2, 32, 32, 24, 40, 1, 1, 1)])
def test_conv_x3_gradients_do_not_depend_on_the_gradient_magnitude(case):
    """The range problem: losses are mean()-reduced, grad_y is routinely 1e-6 ... 1e-9, below the un-scaled operand split's floor
    (low half subnormal below 2^-3, both halves zero below 6e-8).  grad_pre is scaled by a per-tensor power of two from its
    device-side maximum and un-scaled exactly: grad_y * 2^-k gives the bits of the k = 0 result times 2^-k."""
    B, Cin, Cout, H, W, k, d, s = case
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, Cin, H, W, generator=g).cuda()
    w = (torch.randn(Cout, Cin, k, k, generator=g) * 0.05).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    gy = torch.randn(B, Cout, (H - 1) // s + 1, (W - 1) // s + 1, generator=g).cuda()
    _, gx0, gw0, gb0 = _grads(x, w, b, gy, d, s, 0.1)
    assert float(gx0.abs().max()) > 0 and float(gw0.abs().max()) > 0
    for sh in (10, 20, 30):
        f = 2.0 ** -sh
        _, gx, gw, gb = _grads(x, w, b, gy * f, d, s, 0.1)
        assert torch.equal(gx, gx0 * f), sh
        assert torch.equal(gw, gw0 * f), sh
        assert torch.equal(gb, gb0 * f), sh


@pytest.mark.parametrize('case', [(2, 72, 64, 12, 24, 3, 1, 1), (2, 24, 40, 13, 24, 3, 1, 2), (1, 72, 64, 12, 24, 3, 4, 1)])
def test_conv_x3_gradients_are_deterministic_and_alignment_independent(case):
    B, Cin, Cout, H, W, k, d, s = case
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Cin, H, W, generator=g).cuda()
    w = (torch.randn(Cout, Cin, k, k, generator=g) * 0.05).cuda()
    b = torch.zeros(Cout).cuda()
    gy = torch.randn(B, Cout, (H - 1) // s + 1, (W - 1) // s + 1, generator=g).cuda() * 1e-5
    a0 = _grads(x, w, b, gy, d, s, 0.1, off=4)            # W % 4 == 0, buffers on 16-byte boundaries: aligned rows
    a1 = _grads(x, w, b, gy, d, s, 0.1, off=4)
    u = _grads(x, w, b, gy, d, s, 0.1, off=5, misalign=1)   # every row 4 bytes off a 16-byte boundary
    for p, q, r in zip(a0, a1, u):
        assert torch.equal(p, q)
        assert torch.equal(p, r)


# ---- the whole step ---------------------------------------------------------------------------------------------------
def _net(head_scale, **extra):
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    conf = UPFlow_net.config()
    d = dict(FLAGS)
    d.update(_weights.TRAIN_FLAGS)
    d['train_conv_dtype'] = 'fp32'
    d['fp32_train_conv'] = 'hip_x3'
    d.update(extra)
    conf.update(d, verbose=False)
    net = conf()
    net.load_state_dict(_weights.make_state_dict(0, head_scale=head_scale))
    return net


def _realistic_step():
    """tests/test_hip_train.py's _realistic_step with fp32_train_conv='hip_x3'."""
    net = _net(1.0).cuda().train()
    batch = {k: v.cuda() for k, v in _weights.make_train_batch(**_weights.TRAIN_HS1).items()}
    batch['if_loss'] = True
    out = net(batch)
    terms = {k: out[k].mean() for k in ('photo_loss', 'smooth_loss', 'census_loss', 'msd_loss')}
    sum(terms.values()).backward()
    names = sorted(n for n, _ in net.named_parameters())
    params = dict(net.named_parameters())
    return out, terms, names, params


def test_x3_train_step_at_realistic_motion_matches_reference():
    """test_train_step_at_realistic_motion_matches_reference with every convolution, forward and backward, on the split-precision
    kernels: the same golden (train_128x416_hs1: the crop reaches 4x13 and 2x7 levels) and exactly the same bounds."""
    g = load_golden('train_128x416_hs1')
    out, terms, names, params = _realistic_step()
    epe_f = oracle.epe(out['flow_f_out'].detach().cpu(), g['flow_f_out'])
    epe_b = oracle.epe(out['flow_b_out'].detach().cpu(), g['flow_b_out'])
    occ = {k_: float((out[k_].detach().cpu() != g[k_].float()).float().mean()) for k_ in ('occ_fw', 'occ_bw')}
    print('hip_x3 realistic motion: epe %.3g / %.3g px, occlusion mismatch %s' % (epe_f, epe_b, occ))
    for k, v in terms.items():
        print(k, float(v), float(g[k]))
    got = np.array([float(params[n].grad.norm()) for n in names])
    want = g['grad_norms'].numpy()
    rel = np.abs(got - want) / np.maximum(want, 1e-3)
    cos, worst = grad_direction_check({n: params[n].grad for n in names}, g)
    print('hip_x3 realistic motion: max rel grad-norm error %.3g (param %s), min cosine %.7f (param %s), worst bias-gradient error %.3g'
          % (rel.max(), names[int(rel.argmax())], cos.min(), names[int(cos.argmin())], worst))
    assert epe_f <= 1e-4 and epe_b <= 1e-4
    for k_ in occ:
        assert occ[k_] <= 2e-3, k_
    for k, v in terms.items():
        want_k = float(g[k])
        assert abs(float(v) - want_k) <= 2e-4 * max(1.0, abs(want_k)), k
    assert (got > 0).all() and rel.max() <= 1e-2 and cos.min() >= 0.9999 and worst <= 1.5e-2


def test_x3_train_losses_and_gradients_match_reference_at_small_motion():
    """test_train_losses_and_gradients_match_reference (train_128x192) with fp32_train_conv='hip_x3', the same bounds."""
    g = load_golden('train_128x192')
    net = _net(0.1).cuda().train()
    batch = {k: v.cuda() for k, v in _weights.make_train_batch().items()}
    batch['if_loss'] = True
    out = net(batch)
    terms = {k: out[k].mean() for k in ('photo_loss', 'smooth_loss', 'census_loss', 'msd_loss')}
    for k, v in terms.items():
        want = float(g[k])
        print(k, float(v), want)
        assert abs(float(v) - want) <= 2e-4 * max(1.0, abs(want)), k
    assert oracle.epe(out['flow_f_out'].detach().cpu(), g['flow_f_out']) <= 1e-4
    sum(terms.values()).backward()
    names = sorted(n for n, _ in net.named_parameters())
    params = dict(net.named_parameters())
    got = np.array([float(params[n].grad.norm()) for n in names])
    want = g['grad_norms'].numpy()
    rel = np.abs(got - want) / np.maximum(want, 1e-3)
    cos, worst = grad_direction_check({n: params[n].grad for n in names}, g)
    print('hip_x3 small motion: max rel grad-norm error %.3g (param %s), min cosine %.7f, worst bias-gradient error %.3g'
          % (rel.max(), names[int(rel.argmax())], cos.min(), worst))
    assert (got > 0).all(), 'every parameter must receive a gradient'
    assert rel.max() <= 2e-3
    assert cos.min() >= 0.9999 and worst <= 5e-3


def test_x3_train_step_calls_no_pytorch_convolution(monkeypatch):
    """With the mode on every nn.Conv2d of the network — feature pyramid, 1x1 projections, both dense stacks, context network, SGU
    guidance stem — runs through ops.ConvX3TrainFunction, forward and backward, down to the 2x7 level: the three Python entry points of
    PyTorch-ROCm's convolution are never called during a step."""
    from upflow_pytorch_amd import ops
    calls = {'conv2d': 0, 'conv2d_input': 0, 'conv2d_weight': 0, 'x3': 0}

    def counting(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapped
    monkeypatch.setattr(torch.nn.functional, 'conv2d', counting('conv2d', torch.nn.functional.conv2d))
    monkeypatch.setattr(torch.nn.grad, 'conv2d_input', counting('conv2d_input', torch.nn.grad.conv2d_input))
    monkeypatch.setattr(torch.nn.grad, 'conv2d_weight', counting('conv2d_weight', torch.nn.grad.conv2d_weight))
    monkeypatch.setattr(ops, 'conv_x3_train', counting('x3', ops.conv_x3_train))
    out, terms, names, params = _realistic_step()
    assert all(params[n].grad is not None for n in names)
    print(calls)
    assert calls['x3'] > 100                              # (12 + 5 + 5 x (6 + 7 + 6) + 4 + 6 layer uses)
    assert calls['conv2d'] == 0 and calls['conv2d_input'] == 0 and calls['conv2d_weight'] == 0, calls


def test_x3_train_step_is_bit_reproducible():
    """Two fresh runs of the step give the same bits for every parameter's gradient (the other backward kernels are
    bit-deterministic: test_backward_kernels_are_bit_deterministic; the MIOpen mode's convolution gradients are not)."""
    runs = []
    for _ in range(2):
        out, terms, names, params = _realistic_step()
        runs.append(({n: params[n].grad.clone() for n in names}, out['flow_f_out'].detach().clone()))
    assert torch.equal(runs[0][1], runs[1][1])
    diff = [n for n in runs[0][0] if not torch.equal(runs[0][0][n], runs[1][0][n])]
    assert not diff, diff


def test_x3_graphed_training_step_equals_eager_bit_for_bit():
    """Trainer(graph=True) with the mode on: 3 eager steps, capture, replays.  Parameters after 6 steps (3 eager + 3 replayed) equal a
    Trainer that ran the same 6 steps eagerly — bit for bit: the step has no host synchronisation and no non-deterministic kernel.
    (Both trainers use capturable Adam: the only difference between them is capture + replay.)"""
    from upflow_pytorch_amd.train import Trainer
    batch = {k: v.cuda() for k, v in _weights.make_train_batch().items()}
    ends = []
    for graph in (False, True):
        tr = Trainer(_net(0.1), lr=1e-4, device=torch.device('cuda', 0), distributed=False, graph=True)
        if not graph:
            tr.graph_warmup = 1 << 30                     # never captures: the same optimizer spelling, eager throughout
        stats = [tr.step(batch) for _ in range(6)]
        assert (tr._graph is not None) == graph and not tr.capture_fallback, tr.capture_error
        assert all(np.isfinite(v) for s_ in stats for v in s_.values())
        ends.append((stats, {n: p.detach().clone() for n, p in tr.raw_net.named_parameters()}))
    (s0, p0), (s1, p1) = ends
    assert s0 == s1
    diff = [n for n in p0 if not torch.equal(p0[n], p1[n])]
    assert not diff, diff


def test_x3_validation_between_replayed_steps_sees_the_current_weights():
    """test_validation_between_replayed_steps_sees_the_current_weights with the mode on: a validation forward after replayed steps
    equals one after invalidate_packed() bit for bit and differs from the one before them; a captured inference graph notices."""
    from upflow_pytorch_amd.train import Trainer
    from upflow_pytorch_amd.runtime import GraphedInference
    tr = Trainer(_net(0.1).cuda().train(), lr=1e-3, device=torch.device('cuda', 0), distributed=False, graph=True)
    batch = {k: v.cuda() for k, v in _weights.make_train_batch().items()}
    for _ in range(tr.graph_warmup + 1):
        tr.step(batch)
    assert tr._graph is not None
    im1, im2 = batch['im1'], batch['im2']

    def validate():
        tr.raw_net.eval()
        with torch.no_grad():
            return tr.raw_net({'im1': im1, 'im2': im2, 'if_loss': False})['flow_f_out'].clone()
    first = validate()
    runner = GraphedInference(tr.raw_net.eval(), im1.shape[0], im1.shape[2], im1.shape[3], device=im1.device)
    for _ in range(5):
        tr.step(batch)
    second = validate()
    tr.raw_net.invalidate_packed()
    fresh = validate()
    assert torch.equal(second, fresh), 'a validation forward after replayed steps used stale packed weights'
    assert not torch.equal(first, second), 'five optimizer steps at lr 1e-3 must move the validation output'
    with pytest.raises(RuntimeError):
        runner.replay()
