"""Measurements behind DESIGN §4.5 "loss scaling" (profiles/loss_scale_*.txt), at BASELINE config 3 (256x832 crops, batch 4):

  grads   one eager forward + backward per setting on the same batch and weights: the fp32 mode, and the fp16 mode with the
          backward seeded by S = 1, 2^4, ... 2^16.  Per setting: whether every gradient is finite; of the activation gradients the
          16-bit layers read (every tensor handed to ops.act_grad, i.e. after the cast to fp16) the fraction that is zero and the
          fraction that is subnormal (0 < |x| < 2^-14); the distance of the un-scaled gradients from the fp32 mode's.
  time    the captured step, three trainers alive at once and ALTERNATED in blocks: fp16 + loss_scale='dynamic' (NativeAdam),
          fp16 without a scale and bf16 without a scale (torch's fused Adam: the step as it was before loss scaling existed).

    python tools/loss_scale_measure.py grads
    python tools/loss_scale_measure.py time [--blocks 6] [--steps 40]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from upflow_pytorch_amd import ops, synthetic                        # noqa: E402
from upflow_pytorch_amd.train import Loss_manager, Trainer, synthetic_train_batch   # noqa: E402

FLAGS = {'if_norm_before_cost_volume': True, 'norm_moments_across_channels': False,
         'norm_moments_across_images': False, 'if_sgu_upsample': True, 'warp_mask_mode': 'robust'}
DEV = torch.device('cuda', 0)


def make_net(mode, seed=0):
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    conf = UPFlow_net.config()
    d = dict(FLAGS)
    d.update(synthetic.TRAIN_FLAGS)
    d['train_conv_dtype'] = mode
    conf.update(d, verbose=False)
    net = conf()
    net.load_state_dict(synthetic.make_state_dict(seed, head_scale=0.1))
    return net


class ActGradCensus():
    """Counts, on the device, the zero and subnormal elements of every 16-bit gradient tensor ops.act_grad is handed."""

    def __init__(self):
        self.counts = torch.zeros(3, dtype=torch.float64, device=DEV)      # elements, zeros, subnormals
        self.real = ops.act_grad

    def __enter__(self):
        def counted(g, *a, **kw):
            if torch.is_tensor(g) and g.dtype == torch.float16:
                m = g.abs().float()
                self.counts += torch.stack([torch.tensor(float(g.numel()), device=DEV, dtype=torch.float64), (m == 0).sum().double(),
                                            ((m > 0) & (m < 2.0 ** -14)).sum().double()])
            return self.real(g, *a, **kw)
        ops.act_grad = counted
        return self

    def __exit__(self, *exc):
        ops.act_grad = self.real

    def fractions(self):
        n, z, s = self.counts.tolist()
        return n, z / max(n, 1), s / max(n, 1)


def backward_once(mode, batch, scale):
    net = make_net(mode).to(DEV).train()
    b = dict(batch)
    b['if_loss'] = True
    loss, _ = Loss_manager().compute_loss(net(b))
    with ActGradCensus() as census:
        loss.backward(gradient=torch.tensor(float(scale), device=DEV))
    grads = {n: p.grad.detach() / scale for n, p in net.named_parameters()}
    return float(loss.detach()), grads, census.fractions()


def grads_main():
    batch = synthetic_train_batch(4, device=DEV)
    loss32, g32, _ = backward_once('fp32', batch, 1.0)
    names = sorted(g32)
    flat32 = torch.cat([g32[n].flatten().double() for n in names])
    print('config 3 (256x832, batch 4), %d parameters in %d tensors; fp32 mode: loss %.6f, |grad| %.6g' % (flat32.numel(), len(names), loss32, float(flat32.norm())))
    print('%-8s %-8s %-12s %-12s %-12s %-14s %-14s %-12s' % ('mode', 'S', 'finite', 'act-grad 0', 'act-grad sub', 'norm err max', 'norm err med', '|g-g32|/|g32|'))
    for s in (0, 4, 8, 10, 12, 14, 16):
        S = 2.0 ** s
        loss, g, (n, fz, fs) = backward_once('fp16', batch, S)
        finite = all(bool(torch.isfinite(g[k]).all()) for k in names)
        if finite:
            rel = np.array([abs(float(g[k].norm()) - float(g32[k].norm())) / max(float(g32[k].norm()), 1e-3) for k in names])
            flat = torch.cat([g[k].flatten().double() for k in names])
            dist = float((flat - flat32).norm() / flat32.norm())
            print('%-8s 2^%-6d %-12s %-12.5f %-12.5f %-14.4g %-14.4g %-12.4g' % ('fp16', s, 'yes', fz, fs, rel.max(), np.median(rel), dist))
        else:
            bad = sum(not bool(torch.isfinite(g[k]).all()) for k in names)
            print('%-8s 2^%-6d %-12s %-12.5f %-12.5f (%d of %d gradient tensors hold a NaN / inf: the step would be skipped)' % ('fp16', s, 'NO', fz, fs, bad, len(names)))
    print('(act-grad: %d elements per backward pass; zero includes structural zeros of masked pixels)' % n)


def time_main(blocks, steps):
    batch = synthetic_train_batch(4, device=DEV)
    variants = [('fp16 + dynamic loss scale', 'fp16', 'dynamic'), ('fp16, no scale', 'fp16', None), ('bf16, no scale', 'bf16', None)]
    trainers = []
    for name, mode, ls in variants:
        tr = Trainer(make_net(mode), lr=1e-4, device=DEV, distributed=False, graph=True, loss_scale=ls)
        for _ in range(3 + 25):                              # capture, then replays until the dynamic scale has settled
            st = tr.step(batch)
        assert tr._graph is not None
        trainers.append(tr)
        print('%-28s ready: %s' % (name, {k: round(v, 5) for k, v in st.items()}), flush=True)
    times = [[] for _ in variants]
    for blk in range(blocks):
        for i, tr in enumerate(trainers):
            s0 = int(tr.skipped_steps) if tr.skipped_steps is not None else 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(batch, sync_stats=False)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps * 1e3
            s1 = int(tr.skipped_steps) if tr.skipped_steps is not None else 0
            times[i].append(dt)
            print('block %d  %-28s %.3f ms/step%s' % (blk, variants[i][0], dt, '  (%d of %d steps skipped)' % (s1 - s0, steps) if s1 != s0 else ''), flush=True)
    for (name, _, _), t in zip(variants, times):
        print('%-28s mean %.3f ms  range %.3f .. %.3f  (%d blocks of %d replayed steps, alternated)' % (name, np.mean(t), min(t), max(t), blocks, steps))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['grads', 'time'])
    ap.add_argument('--blocks', type=int, default=6)
    ap.add_argument('--steps', type=int, default=40)
    a = ap.parse_args()
    if a.what == 'grads':
        grads_main()
    else:
        time_main(a.blocks, a.steps)
