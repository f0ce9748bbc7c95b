#!/usr/bin/env python3
"""The evaluation loop's scoring tail, measured: kitti_flow.Evaluation_bench over an in-memory data set of 64 synthetic 375x1242
pairs (8 distinct items, each listed 8 times) with Test_model(streams=4, pretrain_path=None) in bf16, three arms alternated on one
box, three windows each, every window PASSES full passes over the data set (host clock around a pass that ends in a synchronise):

  host-score    the existing path: fp32 frames and the six fp32 planes of the decoded ground truth from pageable memory, ~30 ATen
                launches and four blocking reads per pair;
  device-score  device_score=True: uint8 frames, the uint16 PNG payload, one ops.kitti_score call per pair, rows read late;
  forward       Test_model.eval_forward_stream alone over the same pairs (uint8 frames resident on the device): no ground truth,
                no scoring, no hook.

The save hook is a no-op in both scoring arms.  The two arms' four numbers are printed; they agree to the fp32 summation of the
existing path.

    python tools/eval_score_measure.py [--pairs 64] [--passes 10] [--windows 3] [--out profiles/eval_device_score.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 375, 1242


def make_items(distinct):
    """-> (four-tuples with uint8 frames and uint16 ground truth, the same items as the default six-tuples of fp32 tensors)."""
    import _weights
    from upflow_pytorch_amd.dataset.kitti_dataset import img_func
    q = lambda im: ((im + 0.45) * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # noqa: E731
    new, old = [], []
    for i in range(distinct):
        f1, f2 = (q(t)[0] for t in _weights.make_smooth_images(300 + i, 1, H, W))
        g = np.random.default_rng(i)
        gts = []
        for sparse in (0.2, 0.45):                                           # occ, noc: KITTI's ground truth is sparse
            flow = np.rint(g.normal(size=(H, W, 2)) * 2.0 * 64.0) + 32768.0
            gts.append(np.concatenate([flow, (g.random((H, W, 1)) > sparse)], axis=-1).astype(np.uint16))
        gts[1][..., :2] = gts[0][..., :2]
        gts[1][..., 2] *= gts[0][..., 2]
        new.append((f1, f2, torch.from_numpy(gts[0]), torch.from_numpy(gts[1])))
        planes = []
        for gt in gts:                                                       # flow_io.read_kitti_png_flow + img_func.np_2_tensor
            planes += img_func.np_2_tensor(np.transpose((gt[:, :, 0:2].astype('float64') - 2 ** 15) / 64.0, [2, 0, 1]),
                                           np.transpose(np.uint8(gt[:, :, 2:3]), [2, 0, 1]))
        frames = img_func.np_2_tensor(*[img_func.get_process_img_only_img(f.numpy()) for f in (f1, f2)])
        old.append(tuple(frames + planes))
    return new, old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--distinct', type=int, default=8)
    ap.add_argument('--passes', type=int, default=10)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_score_measure: needs the GPU (a timing from anywhere else says nothing)')
    from upflow_pytorch_amd.test import Test_model
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow

    class Quiet(Test_model):
        def eval_save_result(self, save_name, predflow, *args, **kwargs):
            pass
    torch.manual_seed(0)
    tm = Quiet(pretrain_path=None, dtype=torch.bfloat16, streams=4)
    new, old = make_items(a.distinct)
    ds_new = [new[i % a.distinct] for i in range(a.pairs)]
    ds_old = [old[i % a.distinct] for i in range(a.pairs)]
    resident = [(it[0].unsqueeze(0).cuda(), it[1].unsqueeze(0).cuda()) for it in new]
    bench_old = kitti_flow.Evaluation_bench('2015_train', batch_size=1, dataset=ds_old)
    bench_new = kitti_flow.Evaluation_bench('2015_train', batch_size=1, dataset=ds_new, device_score=True)
    results = {}

    def forward():
        for flow in tm.eval_forward_stream(resident[i % a.distinct] for i in range(a.pairs)):
            pass

    arms = [('host-score', lambda: results.__setitem__('host-score', bench_old(tm))),
            ('device-score', lambda: results.__setitem__('device-score', bench_new(tm))),
            ('forward', forward)]
    for _, run in arms:                                                      # captures, allocator, pinned table
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
    mean = {k: sum(v) / len(v) for k, v in t.items()}
    lines = ['evaluation loop, %d pairs of %dx%d (%d distinct), batch 1, bf16, Test_model(streams=4), %s; %d windows per arm, alternated, '
             '%d passes per window; ms per pair' % (a.pairs, H, W, a.distinct, torch.cuda.get_device_name(0), a.windows, a.passes)]
    for name, _ in arms:
        lines.append('  %-13s %.3f ms/pair (%.3f-%.3f)  windows: %s' % (name, mean[name], min(t[name]), max(t[name]), ' '.join('%.3f' % v for v in t[name])))
    lines.append('  scoring tail (arm - forward): host-score %+.3f ms, device-score %+.3f ms; device-score / host-score = %.3f'
                 % (mean['host-score'] - mean['forward'], mean['device-score'] - mean['forward'], mean['device-score'] / mean['host-score']))
    for name in ('host-score', 'device-score'):
        lines.append('  %-13s EPE all %.6f  F1 %.6f  EPE noc %.6f  EPE occ %.6f' % ((name,) + tuple(results[name])))
    print('\n'.join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
