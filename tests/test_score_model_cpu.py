"""The device-side KITTI scoring, the parts that need no GPU: the numpy model of upf_kitti_score (tests/_score_model.py) against the
reference's recorded metrics and decode, the uint16 ground-truth items of kitti_flow.kitti_train(gt_u16=True) against the default
items, and the no-CPU-fallback rule of Evaluation_bench(device_score=True)."""
import math
import os

import numpy as np
import pytest
import torch

import _score_model as sm
from upflow_pytorch_amd.utils import flow_io
from upflow_pytorch_amd.utils.tools import tools
from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_edge.npz')


@pytest.fixture(scope='module')
def edge():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


def _core(gt, pred, mask):
    """The model's core with one ground truth and one mask in both roles (what the fixture's single-mask metrics are)."""
    m = mask[:, 0]
    return sm.core(gt[:, 0], gt[:, 1], m, gt[:, 0], gt[:, 1], m, pred[:, 0], pred[:, 1])


def test_model_reproduces_the_references_recorded_metrics(edge):
    """EPE within n * 2^-24 relative (n pixels: the a-priori bound of the reference's fp32 summation; observed 1e-7), F1 within
    1e-5, the empty mask EPE 0 and F1 nan."""
    gt, pred = edge['ev_gt'], edge['ev_pred']
    n = gt.shape[0] * gt.shape[2] * gt.shape[3]
    bound = n * 2.0 ** -24
    far = (gt + np.float32(100.0)).astype(np.float32)
    cases = [('rand', pred, edge['ev_mask_rand'], edge['ev_epe_rand'], edge['ev_f1_rand']),
             ('full', pred, edge['ev_mask_full'], edge['ev_epe_full'], edge['ev_f1_full']),
             ('all_outliers', far, edge['ev_mask_rand'], edge['ev_epe_all_outliers'], edge['ev_f1_all_outliers']),
             ('exact', gt, edge['ev_mask_rand'], None, edge['ev_f1_exact'])]
    for name, p, mask, want_epe, want_f1 in cases:
        epe, f1, epe_noc, _ = sm.values(_core(gt, p, mask))
        print(name, epe, f1, None if want_epe is None else float(want_epe[0]), float(want_f1[0]))
        if want_epe is not None:
            assert abs(epe - float(want_epe[0])) <= bound * abs(float(want_epe[0])), name
            assert epe_noc == epe, name
        assert abs(f1 - float(want_f1[0])) <= 1e-5, name
    epe, f1, _, _ = sm.values(_core(gt, pred, edge['ev_mask_empty']))
    assert epe == 0.0 == float(edge['ev_epe_empty'][0]) and math.isnan(f1) and math.isnan(float(edge['ev_f1_empty'][0]))


def test_model_decode_equals_the_png_reader(edge, tmp_path):
    raw = edge['png_raw_pypng']
    p = str(tmp_path / 'k.png')
    flow_io.write_png(p, raw)
    flow, mask = flow_io.read_kitti_png_flow(p)
    got_flow, got_mask = sm.decode(raw)
    assert got_flow.dtype == np.float32 and np.array_equal(np.transpose(got_flow, [2, 0, 1]), flow.astype(np.float32))
    assert np.array_equal(got_flow.astype(np.float64), np.transpose(flow, [1, 2, 0]))          # nothing was rounded away
    assert np.array_equal(got_mask, mask[0].astype(np.float32))
    # the valid channel wraps as np.uint8() does
    wrap = raw.copy()
    wrap[..., 2] = np.array([0, 1, 2, 256, 257, 511], dtype=np.uint16)[np.arange(raw[..., 2].size).reshape(raw.shape[:2]) % 6]
    assert np.array_equal(sm.decode(wrap)[1], np.uint8(wrap[..., 2]).astype(np.float32))


def _write_tree(tmp_path, four_channels=False):
    root = tmp_path / 'data_scene_flow' / 'training'
    for d in ('image_2', 'flow_occ', 'flow_noc'):
        os.makedirs(root / d)
    g = np.random.default_rng(11)
    for i, (h, w) in enumerate(((32, 64), (30, 62), (32, 64))):
        for k in (10, 11):
            flow_io.write_png(str(root / 'image_2' / ('%06d_%d.png' % (i, k))), g.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
        fl = np.round(g.normal(size=(h, w, 2)) * 10 * 64) / 64
        occ_mask = (g.random((h, w)) > 0.2).astype(np.uint8)
        noc_mask = occ_mask * (g.random((h, w)) > 0.3).astype(np.uint8)
        tools.write_kitti_png_file(str(root / 'flow_occ' / ('%06d_10.png' % i)), fl, occ_mask)
        tools.write_kitti_png_file(str(root / 'flow_noc' / ('%06d_10.png' % i)), fl, noc_mask)
    return root


def test_gt_u16_items_decode_to_the_default_items(tmp_path):
    root = _write_tree(tmp_path)
    default = kitti_flow.kitti_train('2015_train', root=str(tmp_path))
    for u8 in (False, True):
        ds = kitti_flow.kitti_train('2015_train', root=str(tmp_path), u8=u8, gt_u16=True)
        ref = kitti_flow.kitti_train('2015_train', root=str(tmp_path), u8=u8)
        assert len(ds) == len(default) == 3
        for i in range(len(ds)):
            im1, im2, gt_occ, gt_noc = ds[i]
            _, _, occ, occmask, noc, nocmask = default[i]
            assert torch.equal(im1, ref[i][0]) and torch.equal(im2, ref[i][1]) and im1.dtype == (torch.uint8 if u8 else torch.float32)
            for gt, flow, mask in ((gt_occ, occ, occmask), (gt_noc, noc, nocmask)):
                assert gt.dtype == torch.uint16 and tuple(gt.shape) == tuple(flow.shape[1:]) + (3,) and gt.is_contiguous()
                f, m = sm.decode(gt.numpy())
                assert np.array_equal(np.transpose(f, [2, 0, 1]), flow.numpy()) and flow.dtype == torch.float32
                assert np.array_equal(m[None], mask.numpy())
    # the collation the bench performs works on uint16
    a, b = ds[0][2], ds[2][2]
    assert torch.stack([a, b]).dtype == torch.uint16
    # a fourth channel is dropped on the host; a file that is not 16-bit RGB keeps the reader's error
    gt = flow_io.read_png(str(root / 'flow_occ' / '000000_10.png'))
    flow_io.write_png(str(root / 'flow_occ' / '000000_10.png'), np.concatenate([gt, gt[..., :1]], axis=-1))
    assert torch.equal(ds[0][2], torch.from_numpy(gt)) and tuple(ds[0][2].shape) == (32, 64, 3)
    flow_io.write_png(str(root / 'flow_occ' / '000000_10.png'), (gt >> 8).astype(np.uint8))
    with pytest.raises(ValueError, match='16-bit RGB'):
        ds[0]
    with pytest.raises(ValueError, match='16-bit RGB'):
        default[0]
    # the test split has no ground truth: gt_u16 changes nothing there
    os.makedirs(tmp_path / 'data_scene_flow' / 'testing' / 'image_2')
    for k in (10, 11):
        flow_io.write_png(str(tmp_path / 'data_scene_flow' / 'testing' / 'image_2' / ('000000_%d.png' % k)), np.zeros((8, 8, 3), dtype=np.uint8))
    assert len(kitti_flow.kitti_train('2015_test', root=str(tmp_path), gt_u16=True)[0]) == 3


def test_device_score_has_no_cpu_form():
    with pytest.raises(ValueError, match='no CPU fallback'):
        kitti_flow.Evaluation_bench('2015_train', if_gpu=False, dataset=[], device_score=True)
    # the default path is untouched by the new keywords
    bench = kitti_flow.Evaluation_bench('2015_train', if_gpu=False, dataset=[])
    assert bench.device_score is False and bench(tools.abs_test_model()) == (0, 0, 0, 0)
