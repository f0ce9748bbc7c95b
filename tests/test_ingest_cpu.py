"""The uint8 data edge without a GPU: dataset.kitti_train.kitti_data_u8 describes the SAME samples as kitti_data_with_start_point
(same random draws, in the same order), so a numpy model of ops.assemble_train_batch — a float64 table, reversed-index flip,
slicing — applied to its items reproduces the fp32 class's five tensors bit for bit; the default collate; kitti_flow.kitti_train
(u8=True); and the host-side argument checks of ops.assemble_train_batch."""
import os
import random

import numpy as np
import pytest
import torch

from upflow_pytorch_amd import ops
from upflow_pytorch_amd._lib import UpflowHipError
from upflow_pytorch_amd.dataset.kitti_dataset import img_func, kitti_flow, kitti_train
from upflow_pytorch_amd.utils import flow_io
from upflow_pytorch_amd.utils.tools import tools


def table(normalize=True):
    """[3,256] fp32: (u - MEAN[c]) / STDDEV in float64, rounded once."""
    u = np.arange(256, dtype=np.float64)
    if not normalize:
        return np.stack([u, u, u]).astype(np.float32)
    return np.stack([(u - m) / img_func.STDDEV for m in img_func.MEAN]).astype(np.float32)


def model_frames(u8, flip=None, normalize=True):
    """numpy model of the operator's un-cropped output: u8 [B,H,W,3] -> fp32 [B,3,H,W]."""
    u8 = np.asarray(u8)
    B, H, W, _ = u8.shape
    t = table(normalize)
    out = np.empty((B, 3, H, W), dtype=np.float32)
    for b in range(B):
        cols = np.arange(W - 1, -1, -1) if (flip is not None and int(flip[b]) != 0) else np.arange(W)
        for c in range(3):
            out[b, c] = t[c][u8[b][:, cols, c]]
    return out


def model_batch(f1, f2, aug, crop_size, normalize=True):
    """numpy model of ops.assemble_train_batch (x, y clamped like the kernel clamps a device aug)."""
    f1, f2, aug = np.asarray(f1), np.asarray(f2), np.asarray(aug)
    B, H, W, _ = f1.shape
    ph, pw = crop_size
    raw1, raw2 = model_frames(f1, aug[:, 2], normalize), model_frames(f2, aug[:, 2], normalize)
    xs = np.clip(aug[:, 0], 0, W - pw)
    ys = np.clip(aug[:, 1], 0, H - ph)
    c1 = np.stack([raw1[b, :, ys[b]:ys[b] + ph, xs[b]:xs[b] + pw] for b in range(B)])
    c2 = np.stack([raw2[b, :, ys[b]:ys[b] + ph, xs[b]:xs[b] + pw] for b in range(B)])
    start = np.stack([xs, ys], 1).astype(np.float32).reshape(B, 2, 1, 1)
    return {'im1': c1, 'im2': c2, 'im1_raw': raw1, 'im2_raw': raw2, 'start': start}


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope='module')
def mv_tree(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('mv_u8')
    root = tmp / 'stereo_flow_2015' / 'data_scene_flow_multiview' / 'training' / 'image_2'
    os.makedirs(root)
    g = np.random.default_rng(16)
    for k in range(0, 8):
        flow_io.write_png(str(root / ('000000_%02d.png' % k)), g.integers(0, 256, size=(96, 160, 3), dtype=np.uint8))
    return str(tmp)


@pytest.mark.parametrize('normalize', [True, False])
def test_same_draws_and_the_model_reproduces_the_fp32_item(mv_tree, normalize):
    conf = kitti_train.kitti_data_with_start_point.config(mv_type='2015', crop_size=(64, 128), data_root=mv_tree, normalize=normalize)
    ds32, ds8 = conf(), kitti_train.kitti_data_u8(conf)
    assert type(ds32) is kitti_train.kitti_data_with_start_point and len(ds8) == len(ds32) == 7
    seen = set()
    for seed in range(24):
        index = seed % len(ds32)
        random.seed(seed), np.random.seed(seed)
        im1, im2, c1, c2, start = ds32[index]
        random.seed(seed), np.random.seed(seed)
        f1, f2, aug = ds8[index]
        assert f1.dtype == torch.uint8 and f1.shape == (96, 160, 3) and f2.shape == f1.shape
        assert aug.dtype == torch.int32 and aug.shape == (3,)
        assert [int(aug[0]), int(aug[1])] == [int(start[0]), int(start[1])]
        m = model_batch(f1[None], f2[None], aug[None], (64, 128), normalize)
        for key, want in (('im1_raw', im1), ('im2_raw', im2), ('im1', c1), ('im2', c2), ('start', start)):
            assert np.array_equal(bits(m[key][0]), bits(want)), (seed, key)
        # which frame came first on disk (the swap) and whether it was mirrored, read off the data itself
        p1 = flow_io.read_image(ds8.filenames_extended[index][0])
        seen.add((bool(aug[2]), not np.array_equal(f1.numpy(), p1)))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


def test_no_flip_and_no_swap_draw_nothing_from_random(mv_tree):
    """The draws are conditional exactly like the fp32 class's: with both augmentations off `random` is not advanced."""
    conf = kitti_train.kitti_data_with_start_point.config(mv_type='2015', crop_size=(64, 128), data_root=mv_tree,
                                                          horizontal_flip_aug=False, swap_images=False)
    random.seed(3), np.random.seed(3)
    state = random.getstate()
    f1, f2, aug = kitti_train.kitti_data_u8(conf)[2]
    assert random.getstate() == state and int(aug[2]) == 0
    random.seed(3), np.random.seed(3)
    im1, im2, c1, c2, start = conf()[2]
    assert np.array_equal(bits(model_frames(f1[None])[0]), bits(im1)) and [int(aug[0]), int(aug[1])] == [int(start[0]), int(start[1])]


def test_default_collate(mv_tree):
    conf = kitti_train.kitti_data_with_start_point.config(mv_type='2015', crop_size=(64, 128), data_root=mv_tree)
    f1, f2, aug = next(iter(torch.utils.data.DataLoader(kitti_train.kitti_data_u8(conf), batch_size=2)))
    assert f1.dtype == torch.uint8 and tuple(f1.shape) == (2, 96, 160, 3) and tuple(f2.shape) == (2, 96, 160, 3)
    assert aug.dtype == torch.int32 and tuple(aug.shape) == (2, 3)


def test_kitti_flow_u8_items_normalise_to_the_default_items(tmp_path):
    root = tmp_path / 'data_scene_flow' / 'training'
    for d in ('image_2', 'flow_occ', 'flow_noc'):
        os.makedirs(root / d)
    g = np.random.default_rng(17)
    for i in range(2):
        for k in (10, 11):
            flow_io.write_png(str(root / 'image_2' / ('%06d_%d.png' % (i, k))), g.integers(0, 256, size=(32, 64, 3), dtype=np.uint8))
        fl = np.round(g.normal(size=(32, 64, 2)) * 10 * 64) / 64
        mask = (g.random((32, 64)) > 0.2).astype(np.uint8)
        tools.write_kitti_png_file(str(root / 'flow_occ' / ('%06d_10.png' % i)), fl, mask)
        tools.write_kitti_png_file(str(root / 'flow_noc' / ('%06d_10.png' % i)), fl, mask)
    ds32 = kitti_flow.kitti_train('2015_train', root=str(tmp_path))
    ds8 = kitti_flow.kitti_train('2015_train', root=str(tmp_path), u8=True)
    assert ds32.u8 is False and len(ds8) == len(ds32) == 2
    for i in range(2):
        want, got = ds32[i], ds8[i]
        assert len(got) == 6 and got[0].dtype == torch.uint8 and tuple(got[0].shape) == (32, 64, 3)
        for k in (0, 1):
            host = img_func.np_2_tensor(img_func.get_process_img_only_img(got[k].numpy()))[0]
            assert np.array_equal(bits(host), bits(want[k]))
            assert np.array_equal(bits(model_frames(got[k][None])[0]), bits(want[k]))
        for k in range(2, 6):
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k])


def test_cpu_aug_out_of_range_raises_value_error():
    f = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    ok = torch.tensor([[0, 0, 0], [30 - 16, 20 - 8, 1]], dtype=torch.int32)
    for bad in ([[-1, 0, 0], [0, 0, 0]], [[0, 0, 0], [30 - 16 + 1, 0, 0]], [[0, -1, 1], [0, 0, 0]], [[0, 20 - 8 + 1, 0], [0, 0, 0]]):
        with pytest.raises(ValueError):
            ops.assemble_train_batch(f, f, torch.tensor(bad, dtype=torch.int32), (8, 16))
    with pytest.raises(ValueError):
        ops.assemble_train_batch(f, f, ok, (21, 16))                    # crop taller than the frame
    # the numpy model states what the kernel does with such values when they arrive in device memory: it clamps
    m = model_batch(f, f, np.array([[-5, 99, 7], [99, -5, 0]]), (8, 16))
    assert m['start'].reshape(2, 2).tolist() == [[0.0, 12.0], [14.0, 0.0]]


def test_cpu_frames_raise_like_every_operator():
    f = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    ok = torch.tensor([[0, 0, 0], [30 - 16, 20 - 8, 1]], dtype=torch.int32)
    with pytest.raises(UpflowHipError):
        ops.assemble_train_batch(f, f, ok, (8, 16))
    with pytest.raises(UpflowHipError):
        ops.frames_from_u8(f)
    with pytest.raises(UpflowHipError):
        ops.frames_from_u8(f.float())


def test_trainer_checks_a_cpu_aug_before_anything_runs():
    """Trainer.step range-checks a CPU aug of a uint8 batch on the host (also on the replay path, where ops.assemble_train_batch is
    not called again), and hands the operator int32 aug and a plain tuple."""
    from upflow_pytorch_amd.train import Trainer
    tr = Trainer(torch.nn.Linear(2, 2), distributed=False)
    f = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    batch = {'frames1_u8': f, 'frames2_u8': f, 'aug': torch.tensor([[0, 0, 0], [15, 0, 1]]), 'crop_size': [8, 16]}
    with pytest.raises(ValueError):
        tr.step(batch)
    batch['aug'] = torch.tensor([[0, 0, 0], [14, 12, 1]])
    prepared = tr._u8_inputs(batch)
    assert prepared['aug'].dtype == torch.int32 and prepared['crop_size'] == (8, 16) and set(prepared) == set(Trainer.U8_KEYS)
    with pytest.raises(UpflowHipError):
        tr.step(batch)                                                  # CPU frames: no fallback
