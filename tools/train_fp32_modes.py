#!/usr/bin/env python3
"""The config-3 training step (256x832, batch 4, train_conv_dtype='fp32') with fp32_train_conv='miopen' and 'hip_x3', timed on ONE
box in ONE process: a Trainer is built and (where the capture succeeds) captured per mode and the two are stepped alternately —
ROUNDS rounds of N steps each, host clock around work that ends in a device synchronise, after warm-up.  Appends the table to --out.

    python tools/train_fp32_modes.py --out profiles/conv_x3_train.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/train_fp32_modes.py --profile hip_x3      (a run of its own: a few eager steps)
    python tools/train_fp32_modes.py --stats DIR --out profiles/conv_x3_train.txt                     (per-kernel table from that run's *_kernel_stats.csv)
"""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_trainer(mode, graph, B):
    import torch
    import bench
    import _weights
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    from upflow_pytorch_amd.train import Trainer
    conf = UPFlow_net.config()
    d = dict(bench.FLAGS)
    d.update(bench.TRAIN_FLAGS)
    d['train_conv_dtype'] = 'fp32'
    d['fp32_train_conv'] = mode
    conf.update(d, verbose=False)
    net = conf()
    net.load_state_dict(_weights.make_state_dict(0, head_scale=0.1))
    return Trainer(net, lr=1e-4, device=torch.device('cuda', 0), distributed=False, graph=graph)


def stats_table(directory, top):
    files = glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True)
    if not files:
        raise SystemExit('no *kernel_stats.csv under %s' % directory)
    rows = list(csv.DictReader(open(files[0])))
    lines = ['%-100s %8s %12s %7s' % ('kernel (rocprofv3 --kernel-trace --stats, hip_x3 mode, eager steps)', 'calls', 'total ms', '%')]
    for r in rows[:top]:
        lines.append('%-100s %8s %12.3f %7s' % (r['Name'][:100], r['Calls'], float(r['TotalDurationNs']) / 1e6, r['Percentage']))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--eager', action='store_true', help='do not capture the step')
    ap.add_argument('--profile', default=None, help="one mode, 3 eager steps (for a rocprofv3 run)")
    ap.add_argument('--stats', default=None, help='directory of a rocprofv3 --stats run: print its per-kernel table')
    ap.add_argument('--top', type=int, default=25)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    if a.stats:
        lines = stats_table(a.stats, a.top)
    else:
        import torch
        from upflow_pytorch_amd.train import synthetic_train_batch
        if not torch.cuda.is_available():
            raise SystemExit('train_fp32_modes: needs the GPU (a timing on the CPU says nothing)')
        batch = synthetic_train_batch(a.batch, seed=0, device=torch.device('cuda', 0))
        if a.profile:
            tr = make_trainer(a.profile, False, a.batch)
            for _ in range(3):
                tr.step(batch, sync_stats=False)
            torch.cuda.synchronize()
            return
        modes = ['miopen', 'hip_x3']
        trainers = []
        for m in modes:
            tr = make_trainer(m, not a.eager, a.batch)
            for _ in range(tr.graph_warmup + 2):
                tr.step(batch, sync_stats=False)
            torch.cuda.synchronize()
            print('%s: warmed up, %s' % (m, 'captured' if tr._graph is not None else 'eager'), file=sys.stderr, flush=True)
            trainers.append(tr)
        tot = [[] for _ in modes]
        for _ in range(a.rounds):
            for i, tr in enumerate(trainers):
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.steps):
                    tr.step(batch, sync_stats=False)
                torch.cuda.synchronize()
                tot[i].append((time.perf_counter() - t) / a.steps * 1e3)
                print('round %d %s: %.2f ms / step' % (len(tot[i]), modes[i], tot[i][-1]), file=sys.stderr, flush=True)
        lines.append('config-3 training step, %dx%d, batch %d, train_conv_dtype=fp32; %d alternating rounds of %d steps, ms / step'
                     % (batch['im1'].shape[2], batch['im1'].shape[3], a.batch, a.rounds, a.steps))
        for m, tr, ts in zip(modes, trainers, tot):
            ts = sorted(ts)
            lines.append('fp32_train_conv=%-7s %-9s median %9.2f  min %9.2f  max %9.2f%s'
                         % (m, 'captured' if tr._graph is not None else 'eager', ts[len(ts) // 2], ts[0], ts[-1],
                            ('   (capture failed: %s)' % tr.capture_error) if tr.capture_fallback else ''))
    print('\n'.join(lines), flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
