#!/usr/bin/env python3
"""Saving evaluation results, measured: kitti_flow.Evaluation_bench(device_score=True) over an in-memory data set of 64 synthetic
375x1242 pairs (8 distinct items, each listed 8 times; tools/eval_score_measure.py's) with Test_model(streams=4,
pretrain_path=None) in bf16 — one network, four models around it — four arms alternated on one box, every window PASSES full
passes over the data set (host clock around a pass that ends with the files complete and a synchronise):

  no-save      eval_save_result does nothing: the loop alone;
  host-writer  eval_save_result copies the prediction back and calls flow_io.write_kitti_png_file on the thread that drives the
               GPU — all there was before Test_model(save_dir=...): a float64 copy, clip, cast, stack, deflate;
  save_dir     Test_model(save_dir=..., save=('kitti',), save_workers=4): ops.flow_export on the device, asynchronous copies into
               pinned buffers, deflate and write on the worker threads; the pass ends with flush();
  png=device   the same with png='device': ops.png_encode after ops.flow_export, the zlib streams copied instead of the samples,
               the IDAT chunk's CRC and the write on the worker threads.

The saving arms write the KITTI PNGs of the same predictions under one tmpfs directory; the files of the last pass of host-writer
and save_dir are compared byte for byte, those of png=device are decoded and compared sample for sample, and the mean file size of
both encoders is recorded.  Then the kernels alone: ops.flow_export, and ops.png_encode on a saved prediction's samples, back to
back on one stream between two device events (so launch gaps are in it), against their bytes over the HBM rate.

    python tools/eval_export_measure.py [--pairs 64] [--passes 2] [--windows 3] [--out profiles/eval_export.txt]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402

H, W = 375, 1242
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12            # bytes / s: a float4 copy on this part, and the data sheet


def kernel_times(lines, iters=200):
    from upflow_pytorch_amd import ops
    pred = torch.randn(1, 2, H, W, device='cuda') * 3.0
    valid = torch.ones(1, 1, H, W, device='cuda')
    n = H * W
    arms = [('kitti, one launch', dict(kitti=True), n * (12 + 6)),
            ('kitti + color + flo, given max_rad, one launch', dict(kitti=True, color=True, flo=True, max_rad=10.0), n * (12 + 6 + 3 + 8)),
            ('kitti + color + flo, per-item maximum, two launches', dict(kitti=True, color=True, flo=True), n * (8 + 12 + 6 + 3 + 8))]
    for name, kw, nbytes in arms:
        out = ops.flow_export(pred, valid, **kw)
        for _ in range(20):
            ops.flow_export(pred, valid, out=out, **{k: v for k, v in kw.items() if k == 'max_rad'})
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = []
        for _ in range(3):
            a.record()
            for _ in range(iters):
                ops.flow_export(pred, valid, out=out, **{k: v for k, v in kw.items() if k == 'max_rad'})
            b.record()
            b.synchronize()
            best.append(a.elapsed_time(b) / iters * 1e3)
        lines.append('  export, %-52s %.1f us per call (%.1f-%.1f; back to back, device events)  %.2f MB: %.2f us at %.2f TB/s measured copy rate, %.2f us at %.0f TB/s'
                     % (name + ':', sum(best) / 3, min(best), max(best), nbytes / 1e6, nbytes / HBM_MEASURED * 1e6, HBM_MEASURED / 1e12,
                        nbytes / HBM_SPEC * 1e6, HBM_SPEC / 1e12))


def png_kernel_times(lines, samples, iters=200):
    """ops.png_encode alone on the uint16 [H,W,3] samples of one saved prediction"""
    from upflow_pytorch_amd import ops
    img = torch.from_numpy(samples[None]).cuda()
    out = ops.png_encode(img)
    for _ in range(20):
        ops.png_encode(img, out=out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = []
    for _ in range(3):
        a.record()
        for _ in range(iters):
            ops.png_encode(img, out=out)
        b.record()
        b.synchronize()
        best.append(a.elapsed_time(b) / iters * 1e3)
    n = int(out[1][0])
    raw = samples.shape[0] * (samples.shape[1] * 6 + 1)
    nbytes = 2 * raw + raw + raw // 8 + out[0].shape[1] + raw + n          # samples read twice; filtered written, counts, slot zeroed; filtered read, stream
    lines.append('  png_encode, uint16 [1,%d,%d,3], three launches:       %.1f us per call (%.1f-%.1f; back to back, device events)  %.2f MB filtered -> %.2f MB stream; '
                 '%.2f MB moved: %.2f us at %.2f TB/s measured copy rate'
                 % (samples.shape[0], samples.shape[1], sum(best) / 3, min(best), max(best), raw / 1e6, n / 1e6, nbytes / 1e6, nbytes / HBM_MEASURED * 1e6, HBM_MEASURED / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--distinct', type=int, default=8)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_export_measure: needs the GPU (a timing from anywhere else says nothing)')
    from eval_score_measure import make_items
    from upflow_pytorch_amd.test import Test_model
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow
    from upflow_pytorch_amd.utils import flow_io

    tmp = tempfile.mkdtemp(prefix='upflow_export_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
    dirs = {k: os.path.join(tmp, k) for k in ('host', 'dev', 'devpng')}
    os.makedirs(os.path.join(dirs['host'], 'flow'))

    class Quiet(Test_model):
        def eval_save_result(self, save_name, predflow, *args, **kwargs):
            pass

    class HostWriter(Test_model):
        def eval_save_result(self, save_name, predflow, *args, **kwargs):
            flow = predflow[0].float().permute(1, 2, 0).cpu().numpy()
            mask = kwargs['occmask'][0, 0].cpu().numpy()
            flow_io.write_kitti_png_file(os.path.join(dirs['host'], 'flow', save_name.rsplit('__', 1)[1] + '.png'), flow, mask)

    class DeviceWriter(Test_model):
        def eval_save_result(self, save_name, predflow, *args, **kwargs):
            super(DeviceWriter, self).eval_save_result(save_name.rsplit('__', 1)[1], predflow, *args, **kwargs)

    try:
        torch.manual_seed(0)
        quiet = Quiet(pretrain_path=None, dtype=torch.bfloat16, streams=4)
        host = HostWriter(pretrain_path=None, dtype=None, net=quiet.net_work, streams=4)
        device = DeviceWriter(pretrain_path=None, dtype=None, net=quiet.net_work, streams=4, save_dir=dirs['dev'], save=('kitti',), save_workers=4)
        devpng = DeviceWriter(pretrain_path=None, dtype=None, net=quiet.net_work, streams=4, save_dir=dirs['devpng'], save=('kitti',), save_workers=4,
                              png='device')
        new, _ = make_items(a.distinct)
        ds = [new[i % a.distinct] for i in range(a.pairs)]
        bench = kitti_flow.Evaluation_bench('2015_train', batch_size=1, dataset=ds, device_score=True)

        def saved():
            bench(device)
            device.flush()
        def saved_png():
            bench(devpng)
            devpng.flush()
        arms = [('no-save', lambda: bench(quiet)), ('host-writer', lambda: bench(host)), ('save_dir', saved), ('png=device', saved_png)]
        for _, run in arms:                                                  # captures, allocator, pinned buffers
            run()
        torch.cuda.synchronize()
        t = {name: [] for name, _ in arms}
        for _ in range(a.windows):
            for name, run in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.passes):
                    run()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / (a.passes * a.pairs) * 1e3)
        device.close()
        devpng.close()
        names = sorted(os.listdir(os.path.join(dirs['host'], 'flow')))
        same = names == sorted(os.listdir(os.path.join(dirs['dev'], 'flow'))) and len(names) == a.pairs and all(
            open(os.path.join(dirs['host'], 'flow', n), 'rb').read() == open(os.path.join(dirs['dev'], 'flow', n), 'rb').read() for n in names)
        size = sum(os.path.getsize(os.path.join(dirs['dev'], 'flow', n)) for n in names) / max(len(names), 1)
        mean = {k: sum(v) / len(v) for k, v in t.items()}
        lines = ['evaluation loop with saving, %d pairs of %dx%d (%d distinct), batch 1, bf16, Test_model(streams=4), device_score=True, %s; '
                 '%d windows per arm, alternated, %d passes per window; ms per pair; KITTI PNGs under %s'
                 % (a.pairs, H, W, a.distinct, torch.cuda.get_device_name(0), a.windows, a.passes, os.path.dirname(tmp))]
        for name, _ in arms:
            lines.append('  %-12s %.3f ms/pair (%.3f-%.3f)  windows: %s' % (name, mean[name], min(t[name]), max(t[name]), ' '.join('%.3f' % v for v in t[name])))
        lines.append('  saving tail (arm - no-save): host-writer %+.3f ms, save_dir %+.3f ms; save_dir / host-writer = %.3f'
                     % (mean['host-writer'] - mean['no-save'], mean['save_dir'] - mean['no-save'], mean['save_dir'] / mean['host-writer']))
        lines.append('  files of the two arms byte-identical: %s (%d files, %.0f KB each on average)' % (same, len(names), size / 1e3))
        import numpy as np
        pnames = sorted(os.listdir(os.path.join(dirs['devpng'], 'flow')))
        decoded = pnames == names and all(np.array_equal(flow_io.read_png(os.path.join(dirs['devpng'], 'flow', n)), flow_io.read_png(os.path.join(dirs['dev'], 'flow', n)))
                                          for n in names)
        psize = sum(os.path.getsize(os.path.join(dirs['devpng'], 'flow', n)) for n in pnames) / max(len(pnames), 1)
        lines.append('  png=device: tail %+.3f ms over no-save; png=device / save_dir = %.3f, save_dir - png=device = %.3f ms per pair (spread of the windows: save_dir %.3f, png=device %.3f)'
                     % (mean['png=device'] - mean['no-save'], mean['png=device'] / mean['save_dir'], mean['save_dir'] - mean['png=device'],
                        max(t['save_dir']) - min(t['save_dir']), max(t['png=device']) - min(t['png=device'])))
        lines.append('  files of png=device decode to the samples of save_dir: %s (%d files, %.0f KB each on average; size ratio to the host writer %.3f)'
                     % (decoded, len(pnames), psize / 1e3, psize / max(size, 1)))
        kernel_times(lines)
        png_kernel_times(lines, flow_io.read_png(os.path.join(dirs['dev'], 'flow', names[0])))
        print('\n'.join(lines), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        if not same:
            raise SystemExit('eval_export_measure: the two arms wrote different files')
        if not decoded:
            raise SystemExit('eval_export_measure: the files of png=device do not decode to the samples of save_dir')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
