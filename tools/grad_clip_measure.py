"""Measurements behind DESIGN §4.5 "gradient-norm clipping" (profiles/grad_clip_config3_*.txt), at BASELINE config 3 (256x832
crops, batch 4, train_conv_dtype='fp16', loss_scale='dynamic'):

  time    the captured step with max_grad_norm=math.inf (the norm is measured, nothing is clipped: the same launches and bytes as
          a step that clips) against the captured step without it, two trainers alive at once and ALTERNATED in blocks.
  trace   a few eager steps of the unclipped and of the clipped trainer, to be run under `rocprofv3 --kernel-trace --stats` (no
          counters): the kernel listing of sumsq_check_kernel, norm_finish_kernel and adam_clipped_kernel beside nonfinite_kernel
          and adam_kernel.

    python tools/grad_clip_measure.py time [--blocks 6] [--steps 40]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/grad_clip_measure.py trace
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_scale_measure import DEV, make_net                              # noqa: E402
from upflow_pytorch_amd.train import Trainer, synthetic_train_batch       # noqa: E402


def time_main(blocks, steps):
    batch = synthetic_train_batch(4, device=DEV)
    variants = [('fp16 + dynamic scale', None), ('fp16 + dynamic scale + norm', math.inf)]
    trainers = []
    for name, bound in variants:
        tr = Trainer(make_net('fp16'), lr=1e-4, device=DEV, distributed=False, graph=True, loss_scale='dynamic', max_grad_norm=bound)
        for _ in range(3 + 25):                              # capture, then replays until the dynamic scale has settled
            st = tr.step(batch)
        assert tr._graph is not None and not tr.capture_fallback
        trainers.append(tr)
        print('%-30s ready: %s' % (name, {k: round(v, 5) for k, v in st.items()}), flush=True)
    times = [[] for _ in variants]
    for blk in range(blocks):
        for i, tr in enumerate(trainers):
            s0 = int(tr.skipped_steps)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(batch, sync_stats=False)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps * 1e3
            s1 = int(tr.skipped_steps)
            times[i].append(dt)
            print('block %d  %-30s %.3f ms/step%s' % (blk, variants[i][0], dt, '  (%d of %d steps skipped)' % (s1 - s0, steps) if s1 != s0 else ''), flush=True)
    for (name, _), t in zip(variants, times):
        print('%-30s mean %.3f ms  median %.3f  range %.3f .. %.3f  (%d blocks of %d replayed steps, alternated)'
              % (name, np.mean(t), np.median(t), min(t), max(t), blocks, steps))
    d = np.array(times[1]) - np.array(times[0])
    print('norm - plain, per block: %s us; mean %.1f us = %.2f %% of the step'
          % (' '.join('%.0f' % (1e3 * v) for v in d), 1e3 * d.mean(), 100.0 * d.mean() / np.mean(times[0])))


def trace_main(steps):
    batch = synthetic_train_batch(4, device=DEV)
    for bound in (None, math.inf):                           # (the unclipped step beside it: nonfinite_kernel, adam_kernel)
        tr = Trainer(make_net('fp16'), lr=1e-4, device=DEV, distributed=False, graph=False, loss_scale='dynamic', max_grad_norm=bound)
        for _ in range(steps):
            st = tr.step(batch)
        print('max_grad_norm=%s, after %d eager steps: %s' % (bound, steps, {k: round(v, 5) for k, v in st.items()}))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['time', 'trace'])
    ap.add_argument('--blocks', type=int, default=6)
    ap.add_argument('--steps', type=int, default=None)
    a = ap.parse_args()
    if a.what == 'time':
        time_main(a.blocks, a.steps or 40)
    else:
        trace_main(a.steps or 12)
