#!/usr/bin/env python3
"""The uint8 data edge at config 3 (batch 4, 375x1242 frames -> 256x832 crops), three measurements:

  kernel  upf_frames_u8_assemble alone: HIP events around 200 back-to-back launches after warm-up, us per launch, and the
          algorithmic traffic (source bytes once + frames + crops written once) over the 6.3 TB/s achievable ceiling as a
          fraction of that time;
  step    the captured bf16 training step fed uint8 frames (the assemble launch inside the graph) against the same step fed the
          fp32 batch the host path builds from the same frames, both batches resident on the device, alternated on one box;
  host    ms per sample of kitti_data_with_start_point.__getitem__ against kitti_data_u8.__getitem__ on the same PNGs (a
          synthetic 375x1242 tree) — a figure of whichever HOST runs it, one thread.

    python tools/ingest_u8_measure.py [kernel] [step] [host] [--out profiles/r07_ingest_u8.txt]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, H, W, PH, PW = 4, 375, 1242, 256, 832
CEILING = 6.3e12


def u8_frames(seed):
    """Smooth moving texture, quantised: [B,H,W,3] uint8 pair."""
    import _weights
    im1, im2 = _weights.make_smooth_images(seed, B, H, W)
    q = lambda im: ((im + 0.45) * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # noqa: E731
    return q(im1), q(im2)


def aug_tensor(seed):
    g = np.random.default_rng(seed)
    return torch.tensor([[g.integers(8, W - 8 - PW), g.integers(8, H - 8 - PH), g.integers(0, 2)] for _ in range(B)], dtype=torch.int32)


def kernel(dev, nrep=200):
    from upflow_pytorch_amd import _lib, ops
    f1, f2 = (t.to(dev) for t in u8_frames(0))
    aug = aug_tensor(0).to(dev)
    want = ops.assemble_train_batch(f1, f2, aug, (PH, PW))
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
    raw1, raw2, crop1, crop2, start = new(B, 3, H, W), new(B, 3, H, W), new(B, 3, PH, PW), new(B, 3, PH, PW), new(B, 2)
    consts = ops._ingest_constants(True)

    def launch():                                        # the entry point itself, on preallocated outputs
        _lib.launch(dev, 'upf_frames_u8_assemble', _lib.ptr(f1), _lib.ptr(f2), _lib.ptr(aug), _lib.ptr(raw1), _lib.ptr(raw2),
                    _lib.ptr(crop1), _lib.ptr(crop2), _lib.ptr(start), B, H, W, PH, PW, *consts)
    for _ in range(20):
        launch()
    torch.cuda.synchronize(dev)
    assert torch.equal(raw2, want['im2_raw']) and torch.equal(crop1, want['im1'])
    g = torch.cuda.CUDAGraph()                           # the launches back to back: no python between them
    with torch.cuda.graph(g):
        for _ in range(nrep):
            launch()
    g.replay()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize(dev)
        times.append(e0.elapsed_time(e1) * 1e3 / nrep)
    traffic = 2 * B * (H * W * 3 + 3 * H * W * 4 + 3 * PH * PW * 4)
    floor = traffic / CEILING * 1e6
    best, mean = min(times), sum(times) / len(times)
    return ['kernel: upf_frames_u8_assemble, B=%d, %dx%d -> %dx%d, two frame sets, %s' % (B, H, W, PH, PW, torch.cuda.get_device_name(0)),
            '  %d launches back to back (one hipGraph of them, HIP events around a replay), 5 windows: us per launch %s'
            % (nrep, ' '.join('%.2f' % t for t in times)),
            '  mean %.2f us, best %.2f us; algorithmic traffic %.1f MB -> %.1f us at 6.3 TB/s = %.0f %% of the mean (%.2f TB/s achieved)'
            % (mean, best, traffic / 1e6, floor, 100 * floor / mean, traffic / mean / 1e6)]


def step(dev, alternations=5, replays=20):
    import bench
    import _weights
    from upflow_pytorch_amd import ops
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    from upflow_pytorch_amd.train import Trainer
    f1, f2 = (t.to(dev) for t in u8_frames(0))
    aug = aug_tensor(0).to(dev)
    fp32 = ops.assemble_train_batch(f1, f2, aug, (PH, PW))
    batches = [{'frames1_u8': f1, 'frames2_u8': f2, 'aug': aug, 'crop_size': (PH, PW)}, fp32]

    def trainer(batch):
        conf = UPFlow_net.config()
        d = dict(bench.FLAGS)
        d.update(bench.TRAIN_FLAGS)
        d['train_conv_dtype'] = 'bf16'
        conf.update(d, verbose=False)
        net = conf()
        net.load_state_dict(_weights.make_state_dict(0, head_scale=0.1))
        tr = Trainer(net, lr=1e-4, device=dev, distributed=False, graph=True)
        for _ in range(tr.graph_warmup + 2):
            tr.step(batch, sync_stats=False)
        assert tr._graph is not None, tr.capture_error
        return tr
    pair = [trainer(b) for b in batches]
    t = [[], []]
    for _ in range(alternations):
        for i, tr in enumerate(pair):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(replays):
                tr.step(batches[i], sync_stats=False)        # (the static-buffer copies included: device to device)
            torch.cuda.synchronize(dev)
            t[i].append((time.perf_counter() - t0) / replays * 1e3)
    mean = [sum(v) / len(v) for v in t]
    nbytes = [sum(v.numel() * v.element_size() for v in b.values() if torch.is_tensor(v)) for b in batches]
    return ['step: config-3 captured bf16 training step, batches resident on the device, %d alternations x %d steps' % (alternations, replays),
            '  fed uint8 frames (%.1f MB of static inputs): %.3f ms/step (%.3f-%.3f)' % (nbytes[0] / 1e6, mean[0], min(t[0]), max(t[0])),
            '  fed the fp32 batch (%.1f MB of static inputs): %.3f ms/step (%.3f-%.3f)' % (nbytes[1] / 1e6, mean[1], min(t[1]), max(t[1])),
            '  difference %+.3f ms' % (mean[0] - mean[1])]


def host(nsamples=12):
    import random
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_train
    from upflow_pytorch_amd.utils import flow_io
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'stereo_flow_2015', 'data_scene_flow_multiview', 'training', 'image_2')
        os.makedirs(root)
        g = np.random.default_rng(0)
        base = np.cumsum(g.integers(0, 3, size=(H, W, 3)), axis=1)
        for k in range(5):
            flow_io.write_png(os.path.join(root, '000000_%02d.png' % k), ((base + 17 * k) % 256).astype(np.uint8))
        conf = kitti_train.kitti_data_with_start_point.config(mv_type='2015', data_root=tmp)
        out = []
        for name, ds in (('kitti_data_with_start_point', conf()), ('kitti_data_u8', kitti_train.kitti_data_u8(conf))):
            random.seed(0), np.random.seed(0)
            ds[0]
            t0 = time.perf_counter()
            for i in range(nsamples):
                ds[i % len(ds)]
            out.append('  %-28s %8.1f ms per sample' % (name, (time.perf_counter() - t0) / nsamples * 1e3))
    return ['host: __getitem__ on %dx%d PNGs (decode included), one thread, %d samples, THIS host (%d CPUs visible)'
            % (H, W, nsamples, os.cpu_count() or 0)] + out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', nargs='*', default=['kernel', 'step', 'host'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    for w in a.what:
        part = host() if w == 'host' else {'kernel': kernel, 'step': step}[w](torch.device('cuda', 0))
        print('\n'.join(part), flush=True)
        lines += part
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
