"""upf_png_encode on the GPU (csrc/png.hip; ops.png_encode) and ResultSaver(png='device') built on it.

The yardstick is tests/_png_model.py, the encoder in Python integers, which test_png_model_cpu.py holds to zlib and to the PNG
reader: the kernels give its bytes, EQUAL, lengths included — there is no arithmetic in an encoder that could round."""
import os

import numpy as np
import pytest
import torch

import _png_model as pm

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32 = np.float32
GUARD = 0xEE


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def encode(batch):
    """batch [B,H,W,C] numpy -> (streams [B,cap] numpy, lengths [B] numpy)"""
    from upflow_pytorch_amd import ops
    streams, lengths = ops.png_encode(dev(batch))
    assert streams.dtype == torch.uint8 and lengths.dtype == torch.int32 and lengths.shape == (batch.shape[0],)
    return streams.cpu().numpy(), lengths.cpu().numpy()


@pytest.fixture(scope='module')
def runs():
    """{tag: (image, model stream, device slot, device length)}"""
    out = {}
    for tag, img in pm.cases().items():
        streams, lengths = encode(img[None])
        out[tag] = (img, pm.encode(img), streams[0], int(lengths[0]))
    return out


def test_streams_equal_the_model_byte_for_byte(runs):
    for tag, (img, want, slot, n) in runs.items():
        assert slot.size == pm.cap_bytes(pm.filtered(img).size), tag
        assert n == len(want), (tag, n, len(want))
        assert slot[:n].tobytes() == want, tag
        assert not slot[n:].any(), tag                                               # the rest of the slot is zero


def test_a_batch_has_one_table_per_image():
    imgs = np.stack([pm.smooth(37, 53, 3, np.uint16, 8), np.zeros((37, 53, 3), np.uint16),
                     np.random.default_rng(3).integers(0, 65536, (37, 53, 3)).astype(np.uint16)])
    streams, lengths = encode(imgs)
    want = [pm.encode(im) for im in imgs]
    assert len({w[:200] for w in want}) == 3                                         # three different block headers
    for i in range(3):
        assert int(lengths[i]) == len(want[i]) and streams[i, :lengths[i]].tobytes() == want[i], i
    one, n1 = encode(imgs[1:2])                                                      # an image alone: the same stream
    assert int(n1[0]) == int(lengths[1]) and np.array_equal(one[0], streams[1])


def test_two_runs_give_equal_bytes(runs):
    for tag in ('many chunks', 'smooth u8x3', 'fibonacci', 'chunk+1'):
        img, _, slot, n = runs[tag]
        streams, lengths = encode(img[None])
        assert int(lengths[0]) == n and np.array_equal(streams[0], slot), tag


def test_an_out_slice_leaves_the_guards_intact(runs):
    from upflow_pytorch_amd import ops
    for tag in ('many chunks', 'one pixel', 'chunk+0'):
        img = runs[tag][0]
        imgs = np.stack([img, img[::-1]])
        cap = pm.cap_bytes(pm.filtered(img).size)
        lead = 48
        big = torch.full((lead + 2 * cap + lead,), GUARD, dtype=torch.uint8, device=DEV)
        lens = torch.full((4,), -7, dtype=torch.int32, device=DEV)
        out = big[lead:lead + 2 * cap].view(2, cap)
        streams, lengths = ops.png_encode(dev(imgs), out=(out, lens[1:3]))
        assert streams.data_ptr() == out.data_ptr() and lengths.data_ptr() == lens[1:3].data_ptr()
        host, lens = big.cpu().numpy(), lens.cpu().numpy()
        assert (host[:lead] == GUARD).all() and (host[lead + 2 * cap:] == GUARD).all(), tag
        assert lens[0] == -7 and lens[3] == -7
        for i, im in enumerate(imgs):
            want = pm.encode(im)
            slot = host[lead + i * cap:lead + (i + 1) * cap]
            assert lens[1 + i] == len(want) and slot[:len(want)].tobytes() == want and not slot[len(want):].any(), (tag, i)


def test_arguments_are_checked():
    from upflow_pytorch_amd import ops
    from upflow_pytorch_amd.ops import UpflowHipError
    img = dev(pm.smooth(6, 10, 3, np.uint16))[None]
    cap = pm.cap_bytes(6 * (10 * 3 * 2 + 1))
    bad = [
        lambda: ops.png_encode(img.cpu()),                                                          # a CPU tensor
        lambda: ops.png_encode(torch.zeros(1, 6, 10, 3, dtype=torch.int16, device=DEV)),            # a wrong dtype
        lambda: ops.png_encode(torch.zeros(1, 6, 10, 3, device=DEV)),
        lambda: ops.png_encode(torch.zeros(1, 6, 10, 5, dtype=torch.uint8, device=DEV)),            # five channels
        lambda: ops.png_encode(torch.zeros(1, 6, 10, 6, dtype=torch.uint16, device=DEV)[..., ::2]),  # not contiguous
        lambda: ops.png_encode(img[0]),                                                             # three dimensions
        lambda: ops.png_encode(img, out=torch.empty(1, cap + 16, dtype=torch.uint8, device=DEV)),   # another pitch
        lambda: ops.png_encode(img, out=torch.empty(1, cap, dtype=torch.int8, device=DEV)),
        lambda: ops.png_encode(img, out=torch.empty(1, cap, dtype=torch.uint8)),                    # out on the CPU
        lambda: ops.png_encode(img, out=(torch.empty(1, cap, dtype=torch.uint8, device=DEV), torch.empty(1, dtype=torch.int64, device=DEV))),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(UpflowHipError):
            f()
            pytest.fail('case %d was accepted' % i)
    streams, lengths = ops.png_encode(img)
    assert tuple(streams.shape) == (1, cap) and int(lengths[0]) > 0


# ---- ResultSaver(png='device'), on the fake model of test_hip_export.py's saver tests ---------------------------------------------
def random_pred(seed, B, H, W):
    g = np.random.default_rng(seed)
    return (g.standard_normal((B, 2, H, W)) * (0.3, 3.0, 40.0)[seed % 3]).astype(F32)


def fake_model(preds, **kw):
    from upflow_pytorch_amd.test import Test_model

    class Fake(Test_model):
        def __init__(self):
            super(Fake, self).__init__(pretrain_path=None, net=torch.nn.Identity(), graph=False, **kw)
            self.calls = 0

        def eval_forward(self, im1, im2, gt, *args):
            assert im1.is_cuda
            self.calls += 1
            return preds[self.calls - 1].clone()

    return Fake()


def frames_of(n):
    sizes = ((32, 64), (40, 72), (32, 64), (25, 37))
    return [dev(random_pred(20 + i, 1, *sizes[i % 4])) for i in range(n)]


def read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_device_pngs_decode_to_the_host_writers_samples(tmp_path):
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow
    from upflow_pytorch_amd.utils import flow_io
    preds = frames_of(6)
    names = ['%06d_10' % i for i in range(6)]
    ds = [(torch.zeros(3, p.shape[2], p.shape[3]), torch.zeros(3, p.shape[2], p.shape[3]), n) for p, n in zip(preds, names)]
    dirs = {}
    for png in ('host', 'device'):
        dirs[png] = str(tmp_path / png)
        model = fake_model(preds, save_dir=dirs[png], save=('kitti', 'color', 'flo'), save_workers=2, png=png)
        assert model.saver.png == png
        assert kitti_flow.Evaluation_bench('2015_test', batch_size=1, dataset=ds)(model) is None
        mask = (torch.rand(1, 1, 32, 64, generator=torch.Generator().manual_seed(1)) > 0.4).float().to(DEV)
        model.eval_save_result('with a mask', preds[0], occmask=mask)                # the training sets' call: a validity plane
        model.close()
    for sub in ('flow', 'color', 'flo'):
        assert sorted(os.listdir(os.path.join(dirs['device'], sub))) == sorted(os.listdir(os.path.join(dirs['host'], sub)))
        assert len(os.listdir(os.path.join(dirs['device'], sub))) == 7
    for n in names + ['with a mask']:
        a, b = (os.path.join(dirs[k], 'flow', n + '.png') for k in ('host', 'device'))
        assert read(a) != read(b)                                                    # (another encoder: other bytes)
        fa, ma = flow_io.read_kitti_png_flow(a)
        fb, mb = flow_io.read_kitti_png_flow(b)
        assert np.array_equal(fa, fb) and np.array_equal(ma, mb), n
        assert np.array_equal(flow_io.read_png(a), flow_io.read_png(b)), n
        a, b = (os.path.join(dirs[k], 'color', n + '.png') for k in ('host', 'device'))
        pa, pb = flow_io.read_png(a), flow_io.read_png(b)
        assert pa.dtype == np.uint8 and pa.shape[2] == 3 and np.array_equal(pa, pb), n
        assert read(os.path.join(dirs['host'], 'flo', n + '.flo')) == read(os.path.join(dirs['device'], 'flo', n + '.flo')), n


def test_a_ring_of_one_slot_still_writes_everything(tmp_path):
    from upflow_pytorch_amd import ops
    from upflow_pytorch_amd.result_saver import ResultSaver
    from upflow_pytorch_amd.utils import flow_io
    preds = frames_of(9)
    saver = ResultSaver(str(tmp_path), save=('kitti', 'color'), workers=1, slots=1, max_rad=5.0, png='device')
    for i, p in enumerate(preds):                                                    # every submit but the first waits for the slot
        saver.submit('f%d' % i, p)
    saver.close()
    assert sorted(os.listdir(str(tmp_path))) == ['color', 'flow']
    for i, p in enumerate(preds):
        want = ops.flow_export(p, kitti=True, color=True, max_rad=5.0)
        assert np.array_equal(flow_io.read_png(str(tmp_path / 'flow' / ('f%d.png' % i))), want['kitti'][0].cpu().numpy()), i
        assert np.array_equal(flow_io.read_png(str(tmp_path / 'color' / ('f%d.png' % i))), want['color'][0].cpu().numpy()), i
    with pytest.raises(ValueError):
        ResultSaver(str(tmp_path), png='gpu')
