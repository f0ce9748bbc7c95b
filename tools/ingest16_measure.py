#!/usr/bin/env python3
"""The 16-bit inference ingest (upf_frames_u8_stack16, ops.stack_frames_u8), two measurements:

  kernel  the entry point alone on preallocated fp16 + bf16 outputs: 200 launches in one hipGraph, HIP events around a replay, us
          per launch, at config 2 (B = 4, 384x1280) and at 375x1242 with B = 1 and B = 4 (pitched rows), against the algorithmic
          traffic (source bytes once + both outputs once) over 6.3 TB/s;
  step    the captured config-2 inference step (to_inference(bfloat16): fp16 pyramid, bf16 decoder), three arms alternated on
          one box, every arm's inputs resident on the device and copied into the runner's static inputs each step:
            u8-new     uint8 frames into a uint8 runner (the ingest launch inside the graph);
            u8-parent  uint8 frames through ops.frames_from_u8 (two eager launches), then the fp32 runner;
            fp32       the fp32 tensors into the fp32 runner.

    python tools/ingest16_measure.py [kernel] [step] [--out profiles/r08_ingest16.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

CEILING = 6.3e12


def u8_frames(seed, B, H, W):
    """Smooth moving texture, quantised: [B,H,W,3] uint8 pair."""
    import _weights
    im1, im2 = _weights.make_smooth_images(seed, B, H, W)
    q = lambda im: ((im + 0.45) * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # noqa: E731
    return q(im1), q(im2)


def kernel_case(dev, B, H, W, nrep=200):
    from upflow_pytorch_amd import _lib, ops
    f1, f2 = (t.to(dev) for t in u8_frames(0, B, H, W))
    want = torch.cat([ops.frames_from_u8(f1), ops.frames_from_u8(f2)], 0)
    X = ops.empty_nchw((2 * B, 3, H, W), torch.float16, dev)
    Xd = ops.empty_nchw((2 * B, 3, H, W), torch.bfloat16, dev)
    consts = ops._ingest_constants(True)

    def launch():                                        # the entry point itself, on preallocated outputs
        _lib.launch(dev, 'upf_frames_u8_stack16', _lib.ptr(f1), _lib.ptr(f2), None, _lib.ptr(X), _lib.UPF_F16, ops.nchw_pitch(X), X.stride(0),
                    _lib.ptr(Xd), _lib.UPF_BF16, ops.nchw_pitch(Xd), Xd.stride(0), B, H, W, *consts)
    for _ in range(20):
        launch()
    torch.cuda.synchronize(dev)
    assert torch.equal(X, want.half()) and torch.equal(Xd, want.bfloat16())
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
    traffic = 2 * B * H * W * 3 * (1 + 2 + 2)
    floor = traffic / CEILING * 1e6
    mean = sum(times) / len(times)
    return ['  B=%d %dx%d (pitch %d), fp16 + bf16 outputs: us per launch %s; mean %.2f, best %.2f; algorithmic traffic %.1f MB -> %.2f us '
            'at 6.3 TB/s = %.0f %% of the mean (%.2f TB/s achieved)'
            % (B, H, W, ops.nchw_pitch(X), ' '.join('%.2f' % t for t in times), mean, min(times), traffic / 1e6, floor, 100 * floor / mean,
               traffic / mean / 1e6)]


def kernel(dev):
    out = ['kernel: upf_frames_u8_stack16, %s; 200 launches in one hipGraph, HIP events around a replay (includes the gap between '
           'graph nodes), 5 windows' % torch.cuda.get_device_name(0)]
    for B, H, W in ((4, 384, 1280), (1, 375, 1242), (4, 375, 1242)):
        out += kernel_case(dev, B, H, W)
    return out


def step(dev, alternations=6, replays=50):
    import bench
    from upflow_pytorch_amd import ops
    from upflow_pytorch_amd.runtime import GraphedInference
    B, H, W = 4, 384, 1280
    net = bench.build_net(torch.bfloat16, dev, pyramid_dtype='fp16')
    f1, f2 = (t.to(dev) for t in u8_frames(0, B, H, W))
    a, b = ops.frames_from_u8(f1), ops.frames_from_u8(f2)
    r8 = GraphedInference(net, B, H, W, in_dtype=torch.uint8, device=dev)
    r32 = GraphedInference(net, B, H, W, device=dev)
    arms = [('u8-new', lambda: r8(f1, f2)),
            ('u8-parent', lambda: r32(ops.frames_from_u8(f1), ops.frames_from_u8(f2))),
            ('fp32', lambda: r32(a, b))]
    ref = r32(a, b)['flow_f_out'].clone()
    for name, run in arms:
        assert torch.equal(run()['flow_f_out'], ref), name
    t = {name: [] for name, _ in arms}
    for _ in range(alternations):
        for name, run in arms:
            for _ in range(5):
                run()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(replays):
                run()                                    # (the copy into the static inputs included: device to device)
            torch.cuda.synchronize(dev)
            t[name].append((time.perf_counter() - t0) / replays * 1e3)
    mean = {k: sum(v) / len(v) for k, v in t.items()}
    out = ['step: config-2 captured inference step (B=4, 384x1280, fp16 pyramid + bf16 decoder), inputs resident on the device, '
           '%d alternations x %d steps; all three arms return the same flow bits' % (alternations, replays)]
    for name, _ in arms:
        out.append('  %-10s %.3f ms/step (%.3f-%.3f)  windows: %s' % (name, mean[name], min(t[name]), max(t[name]), ' '.join('%.3f' % v for v in t[name])))
    out.append('  u8-new - u8-parent %+.3f ms; u8-new - fp32 %+.3f ms; static inputs %.1f MB (uint8) vs %.1f MB (fp32)'
               % (mean['u8-new'] - mean['u8-parent'], mean['u8-new'] - mean['fp32'], 2 * f1.numel() / 1e6, 2 * a.numel() * 4 / 1e6))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', nargs='*', default=['kernel', 'step'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    for w in a.what:
        part = {'kernel': kernel, 'step': step}[w](torch.device('cuda', 0))
        print('\n'.join(part), flush=True)
        lines += part
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
