#!/usr/bin/env python3
"""Saving KITTI error maps, measured: tools/eval_export_measure.py's loop — kitti_flow.Evaluation_bench(device_score=True) over an
in-memory data set of 64 synthetic 375x1242 pairs (8 distinct items, each listed 8 times) with Test_model(streams=4,
pretrain_path=None) in bf16, one network with several models around it — arms alternated on one box, every window PASSES full
passes over the data set (host clock around a pass that ends with the files complete and a synchronise):

  no-save        eval_save_result does nothing: the loop alone;
  error host     Test_model(save_dir=..., save=('error',)): ops.flow_error_image on the device, an asynchronous copy of the bytes,
                 deflate and write on the worker threads;
  error device   the same with png='device': ops.png_encode behind it, the zlib stream copied;
  host route     what a user has without the 'error' kind: the hook copies the prediction and the two uint16 ground-truth tensors
                 back, decodes them, calls tools.flow_error_image_u8 and flow_io.write_png on the thread that drives the GPU;
  color device   save=('color',), png='device': the existing picture kind, for the question whether the error map costs more.

All arms write under one tmpfs directory.  The files of `error host` and `host route` are compared byte for byte, those of
`error device` are decoded and compared with them.  Then ops.flow_error_image alone, both colour modes at dilate 0, 1 and 4, back to back on one stream
between two device events (so launch gaps are in it), against its 23 bytes per pixel over the HBM rate.

    python tools/eval_error_map_measure.py [--pairs 64] [--passes 2] [--windows 3] [--out profiles/eval_error_map.txt]
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 375, 1242
HBM_MEASURED = 6.3e12                                  # bytes / s: a float4 copy on this part


def kernel_times(lines, item, iters=200):
    from upflow_pytorch_amd import ops
    pred = torch.randn(1, 2, H, W, device='cuda') * 3.0
    occ, noc = item[2][None].cuda(), item[3][None].cuda()
    nbytes = H * W * 23
    for log_colors in (True, False):
        for r in (0, 1, 4):
            out = ops.flow_error_image(pred, occ, noc, log_colors=log_colors, dilate=r)
            for _ in range(20):
                ops.flow_error_image(pred, occ, noc, log_colors=log_colors, dilate=r, out=out)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            best = []
            for _ in range(3):
                a.record()
                for _ in range(iters):
                    ops.flow_error_image(pred, occ, noc, log_colors=log_colors, dilate=r, out=out)
                b.record()
                b.synchronize()
                best.append(a.elapsed_time(b) / iters * 1e3)
            lines.append('  flow_error_image, log_colors=%-5s dilate=%d, one launch: %.1f us per call (%.1f-%.1f; back to back, device events)  '
                         '%.2f MB (23 bytes per pixel): %.2f us at %.1f TB/s measured copy rate'
                         % (log_colors, r, sum(best) / 3, min(best), max(best), nbytes / 1e6, nbytes / HBM_MEASURED * 1e6, HBM_MEASURED / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--distinct', type=int, default=8)
    ap.add_argument('--passes', type=int, default=2)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_error_map_measure: needs the GPU (a timing from anywhere else says nothing)')
    from eval_score_measure import make_items
    from upflow_pytorch_amd.test import Test_model
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow
    from upflow_pytorch_amd.utils import flow_io
    from upflow_pytorch_amd.utils.tools import tools

    tmp = tempfile.mkdtemp(prefix='upflow_errmap_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
    dirs = {k: os.path.join(tmp, k) for k in ('route', 'host', 'device', 'color')}
    os.makedirs(os.path.join(dirs['route'], 'error'))

    class Quiet(Test_model):
        def eval_save_result(self, save_name, predflow, *args, **kwargs):
            pass

    class HostRoute(Test_model):
        def eval_save_result(self, save_name, predflow, *args, **kwargs):
            flow = predflow[0].float().permute(1, 2, 0).cpu().numpy()
            occ, noc = kwargs['gt_occ_u16'][0].cpu().numpy(), kwargs['gt_noc_u16'][0].cpu().numpy()
            gt = ((occ[:, :, :2].astype(np.int32) - 32768).astype(np.float32) * np.float32(0.015625))
            m_occ, m_noc = (occ[:, :, 2:3] & 255).astype(np.float32), (noc[:, :, 2:3] & 255).astype(np.float32)
            flow_io.write_png(os.path.join(dirs['route'], 'error', save_name.rsplit('__', 1)[1] + '.png'), tools.flow_error_image_u8(flow, gt, m_occ, m_noc))

    class DeviceWriter(Test_model):
        def eval_save_result(self, save_name, predflow, *args, **kwargs):
            super(DeviceWriter, self).eval_save_result(save_name.rsplit('__', 1)[1], predflow, *args, **kwargs)

    try:
        torch.manual_seed(0)
        quiet = Quiet(pretrain_path=None, dtype=torch.bfloat16, streams=4)
        common = dict(pretrain_path=None, dtype=None, net=quiet.net_work, streams=4)
        route = HostRoute(**common)
        route.wants_gt_u16 = True                      # the bench hands the uint16 ground truth to this hook too
        host = DeviceWriter(save_dir=dirs['host'], save=('error',), save_workers=4, **common)
        device = DeviceWriter(save_dir=dirs['device'], save=('error',), save_workers=4, png='device', **common)
        color = DeviceWriter(save_dir=dirs['color'], save=('color',), save_workers=4, png='device', **common)
        new, _ = make_items(a.distinct)
        ds = [new[i % a.distinct] for i in range(a.pairs)]
        bench = kitti_flow.Evaluation_bench('2015_train', batch_size=1, dataset=ds, device_score=True)

        def saving(model):
            def run():
                bench(model)
                model.flush()
            return run
        arms = [('no-save', lambda: bench(quiet)), ('error host', saving(host)), ('error device', saving(device)),
                ('host route', lambda: bench(route)), ('color device', saving(color))]
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
        for m in (host, device, color):
            m.close()
        names = sorted(os.listdir(os.path.join(dirs['route'], 'error')))
        path = lambda k, n: os.path.join(dirs[k], 'error', n)               # noqa: E731
        same = names == sorted(os.listdir(os.path.join(dirs['host'], 'error'))) and len(names) == a.pairs and all(
            open(path('route', n), 'rb').read() == open(path('host', n), 'rb').read() for n in names)
        decoded = names == sorted(os.listdir(os.path.join(dirs['device'], 'error'))) and all(
            np.array_equal(flow_io.read_png(path('device', n)), flow_io.read_png(path('host', n))) for n in names)
        size = {k: sum(os.path.getsize(path(k, n)) for n in names) / max(len(names), 1) for k in ('host', 'device')}
        mean = {k: sum(v) / len(v) for k, v in t.items()}
        lines = ['evaluation loop saving error maps, %d pairs of %dx%d (%d distinct), batch 1, bf16, Test_model(streams=4), device_score=True, %s; '
                 '%d windows per arm, alternated, %d passes per window; ms per pair; 8-bit RGB PNGs under %s'
                 % (a.pairs, H, W, a.distinct, torch.cuda.get_device_name(0), a.windows, a.passes, os.path.dirname(tmp))]
        for name, _ in arms:
            lines.append('  %-13s %.3f ms/pair (%.3f-%.3f)  windows: %s' % (name, mean[name], min(t[name]), max(t[name]), ' '.join('%.3f' % v for v in t[name])))
        lines.append('  saving tail (arm - no-save): host route %+.3f ms, error host %+.3f ms, error device %+.3f ms, color device %+.3f ms'
                     % tuple(mean[k] - mean['no-save'] for k in ('host route', 'error host', 'error device', 'color device')))
        lines.append('  error device - color device = %+.3f ms per pair (spread of the windows: error device %.3f, color device %.3f)'
                     % (mean['error device'] - mean['color device'], max(t['error device']) - min(t['error device']),
                        max(t['color device']) - min(t['color device'])))
        lines.append('  files of `error host` and `host route` byte-identical: %s (%d files, %.0f KB each on average)' % (same, len(names), size['host'] / 1e3))
        lines.append('  files of `error device` decode to the bytes of `error host`: %s (%.0f KB each on average)' % (decoded, size['device'] / 1e3))
        kernel_times(lines, new[0])
        print('\n'.join(lines), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        if not same:
            raise SystemExit('eval_error_map_measure: the device and the host route wrote different files')
        if not decoded:
            raise SystemExit("eval_error_map_measure: the files of png='device' do not decode to the bytes of png='host'")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
