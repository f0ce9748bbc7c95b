#!/usr/bin/env python3
"""What the native loss variants (csrc/loss_variants.hip) change in a config-3 training step (256x832 crops, batch 4, bf16 matrix-core
mode, the step captured as one hipGraph): for each variant the captured step with the native operators and with the torch spelling
(`net._no_native_loss_variants = True`), alternated on one box, ms per step with the spread over the alternations; and the GPU
kernel launches of the variant's own loss call, forward + backward of both directions, counted with torch.profiler in eager mode.

    python tools/loss_variants_probe.py [--alternations 4] [--replays 10] [--out profiles/r07_loss_variants.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402
import bench  # noqa: E402
import _weights  # noqa: E402
from upflow_pytorch_amd.model.upflow import UPFlow_net, network_tools as nt  # noqa: E402
from upflow_pytorch_amd.train import Trainer, synthetic_train_batch  # noqa: E402

VARIANTS = [('SSIM + occ', {'photo_loss_type': 'SSIM', 'photo_loss_use_occ': True}),
            ('edge order 2', {'smooth_order_2_weight': 1}),
            ('delta order 1+2', {'smooth_type': 'delta', 'smooth_order_2_weight': 1}),
            ('charbonnier', {'photo_loss_type': 'charbonnier'}),
            ('L1', {'photo_loss_type': 'L1'})]


def trainer(over, native, dev, batch):
    conf = UPFlow_net.config()
    d = dict(bench.FLAGS)
    d.update(bench.TRAIN_FLAGS)
    d['train_conv_dtype'] = 'bf16'
    d.update(over)
    conf.update(d, verbose=False)
    net = conf()
    net.load_state_dict(_weights.make_state_dict(0, head_scale=0.1))
    net._no_native_loss_variants = not native
    tr = Trainer(net, lr=1e-4, device=dev, distributed=False, graph=True)
    for _ in range(tr.graph_warmup + 2):
        tr.step(batch, sync_stats=False)
    assert tr._graph is not None, tr.capture_error
    return tr


def loss_call(name, native, dev):
    """The variant's own loss call at config 3's sizes, both directions, forward + backward."""
    g = torch.Generator().manual_seed(0)
    im = [torch.rand(4, 3, 256, 832, generator=g).to(dev) for _ in range(2)]
    warp = [torch.rand(4, 3, 256, 832, generator=g).to(dev).requires_grad_(True) for _ in range(2)]
    flow = [torch.randn(4, 2, 256, 832, generator=g).to(dev).requires_grad_(True) for _ in range(2)]
    occ = [(torch.rand(4, 1, 256, 832, generator=g) > 0.3).float().to(dev) for _ in range(2)]

    def run():
        if name == 'SSIM + occ':
            v = sum(nt.photo_loss_multi_type(im[i], warp[i], occ[i], 'SSIM', 0.4, True, native=native) for i in range(2))
        elif name in ('charbonnier', 'L1'):
            v = sum(nt.photo_loss_multi_type(im[i], warp[i], occ[i], name, 0.4, False, native=native) for i in range(2))
        elif name == 'edge order 2':
            v = sum(nt.edge_aware_smoothness_order2(im[i], flow[i], native=native) for i in range(2))
        else:
            v = sum(nt.flow_smooth_delta(flow[i], False, native=native) + nt.flow_smooth_delta(flow[i], True, native=native) for i in range(2))
        v.backward()
        for t in warp + flow:
            t.grad = None
    return run


def launches(name, native, dev):
    run = loss_call(name, native, dev)
    run()
    torch.cuda.synchronize()
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            run()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return n if n else None
    except Exception as e:                                    # no GPU tracing in this build of torch: timings only
        print('launch count unavailable: %s: %s' % (type(e).__name__, e))
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--alternations', type=int, default=4)
    ap.add_argument('--replays', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    batch = synthetic_train_batch(4, seed=0, device=dev)
    lines = ['config-3 training step (256x832, batch 4, bf16 mode, captured), %s; %d alternations x %d replays'
             % (torch.cuda.get_device_name(0), a.alternations, a.replays),
             '%-18s %24s %24s %10s %22s' % ('variant', 'native ms/step (min-max)', 'torch ms/step (min-max)', 'delta ms', 'launches native/torch')]
    for name, over in VARIANTS:
        pair = [trainer(over, True, dev, batch), trainer(over, False, dev, batch)]
        t = [[], []]
        for _ in range(a.alternations):
            for i, tr in enumerate(pair):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.replays):
                    tr._graph.replay()
                torch.cuda.synchronize()
                t[i].append((time.perf_counter() - t0) / a.replays * 1e3)
        del pair
        torch.cuda.empty_cache()
        ln, lt = launches(name, True, dev), launches(name, False, dev)
        mean = [sum(v) / len(v) for v in t]
        lines.append('%-18s %9.3f (%6.3f-%6.3f) %10.3f (%6.3f-%6.3f) %+10.3f %14s / %s'
                     % (name, mean[0], min(t[0]), max(t[0]), mean[1], min(t[1]), max(t[1]), mean[0] - mean[1], ln, lt))
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
