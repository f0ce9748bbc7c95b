"""upf_flow_export on the GPU (csrc/export.hip; ops.flow_export) and Test_model(save_dir=...) built on it.

The yardstick is the numpy model of tests/_export_model.py, which equals the reference's flow_to_image and the host writer's
encode exactly on the golden frames (test_export_model_cpu.py).  `kitti` and `flo` are integer / bit copies of exact arithmetic:
EQUAL.  `rgb` is exact arithmetic but for atan2, whose last bit can move a floor: every value within ONE level of the model, and
over all cases together at most 1 value in 10 000 different at all — a condition set in advance, not a measurement (the model
itself differs from the reference at none of these inputs; a wrong branch or wheel index is off by dozens of levels)."""
import os
import threading

import numpy as np
import pytest
import torch

import _export_model as em
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32 = np.float32
SHAPES = [(1, 1, 1), (1, 3, 5), (2, 7, 13), (1, 9, 70), (2, 33, 130), (1, 375, 1242)]
INF = F32(np.inf)
# planted values: the ends of the uint16 range and one ulp beyond, the largest value that still encodes below 65535 + 1, multiples
# of 1/64 and the values just below them, signed zero, denormals
TAME = [F32(512), np.nextafter(F32(512), INF), F32(-512), np.nextafter(F32(-512), -INF), F32(511.984375), F32(3.25),
        np.nextafter(F32(3.25), -INF), F32(-7.015625), np.nextafter(F32(-7.015625), -INF), F32(0.015625), np.nextafter(F32(0.015625), -INF),
        F32(-0.0), F32(1e-40), F32(-1e-42)]
# ... and the non-finite ones, the unknown threshold and one ulp above it
WILD = [INF, -INF, F32(np.nan), F32(1e7), np.nextafter(F32(1e7), INF), F32(-1e7), np.nextafter(F32(-1e7), -INF)]
VALID_VALUES = np.array([0, 1, 1.9, 2, 255, 300.5, 65535], dtype=F32)


def random_pred(seed, B, H, W, planted):
    """per-pixel random flow (scale 0.3 / 3 / 40 px by seed), `planted` values at seeded positions of either component"""
    g = np.random.default_rng(seed)
    pred = (g.standard_normal((B, 2, H, W)) * (0.3, 3.0, 40.0)[seed % 3]).astype(F32)
    flat = pred.reshape(-1)
    at = g.permutation(flat.size)[:len(planted)]
    flat[at] = np.array(planted, dtype=F32)[:at.size]
    return pred


def build_cases():
    """-> list of (tag, pred [B,2,H,W], valid [B,1,H,W])"""
    fr = em.golden_frames()
    chw = lambda *names: np.ascontiguousarray(np.stack([fr[n] for n in names]).transpose(0, 3, 1, 2))   # noqa: E731
    cases = [('golden/' + n, chw(n)) for n in fr if fr[n].shape[:2] in ((9, 70), (1, 8), (1, 4))]
    cases.append(('golden/33x130 pair', chw('motion_33x130_3', 'motion_33x130_40')))
    cases.append(('golden/33x130 pair2', chw('motion_33x130_0.3', 'motion_33x130_3')))
    for i, (B, H, W) in enumerate(SHAPES):
        cases.append(('random/%dx%dx%d plain' % (B, H, W), random_pred(3 * i + 2, B, H, W, [])))    # (planted 512 or 1e7 whiten a frame)
        cases.append(('random/%dx%dx%d tame' % (B, H, W), random_pred(3 * i, B, H, W, TAME)))
        cases.append(('random/%dx%dx%d wild' % (B, H, W), random_pred(3 * i + 1, B, H, W, TAME + WILD)))
    out = []
    for k, (tag, pred) in enumerate(cases):
        B, _, H, W = pred.shape
        valid = VALID_VALUES[np.random.default_rng(500 + k).integers(0, len(VALID_VALUES), size=(B, 1, H, W))]
        out.append((tag, pred, valid))
    return out


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def export(pred, valid=None, **kw):
    from upflow_pytorch_amd import ops
    res = ops.flow_export(dev(pred), dev(valid), **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


def bits(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


@pytest.fixture(scope='module')
def runs():
    """every case once, with and without its validity plane: {tag: (pred, valid, got, got_no_valid, want, want_no_valid)}"""
    out = {}
    for tag, pred, valid in build_cases():
        got = export(pred, valid, kitti=True, color=True, flo=True)
        got_nv = export(pred, None, kitti=True, color=True, flo=True)
        out[tag] = (pred, valid, got, got_nv, em.export(pred, valid), em.export(pred, None))
    return out


def test_the_cases_cover_the_listed_shapes_and_values(runs):
    shapes = {(p.shape[0],) + p.shape[2:] for p, *_ in runs.values()}
    assert set(SHAPES) <= shapes
    big = runs['random/1x375x1242 wild'][0]
    for v in TAME + WILD:
        assert (bits(big) == bits(np.array([v], dtype=F32))).any(), v


def test_kitti_and_flo_equal_the_model_bit_for_bit(runs):
    for tag, (pred, valid, got, got_nv, want, want_nv) in runs.items():
        for g, w, what in ((got, want, 'valid'), (got_nv, want_nv, 'no valid')):
            assert g['kitti'].dtype == np.uint16 and g['kitti'].shape == w['kitti'].shape, tag
            assert np.array_equal(g['kitti'], w['kitti']), (tag, what, int((g['kitti'] != w['kitti']).sum()))
            assert g['flo'].dtype == F32 and np.array_equal(bits(g['flo']), bits(w['flo'])), (tag, what)
        assert (got_nv['kitti'][..., 2][~np.isnan(pred).any(axis=1)] == 1).all(), tag
    # what the planted values encode to: the model is the host writer's expression, spelled out here once
    enc = lambda x: int(em.kitti(np.array([[[x, 0]]], dtype=F32))[0, 0, 0])       # noqa: E731
    assert [enc(v) for v in TAME[:5]] == [65535, 65535, 0, 0, 65535] and enc(F32(511.96875)) == 65534
    assert enc(F32(3.25)) == 32768 + 208 and enc(np.nextafter(F32(3.25), -INF)) == 32768 + 207
    assert enc(INF) == 65535 and enc(-INF) == 0 and enc(F32(-0.0)) == 32768
    assert enc(F32(-1e-42)) == 32768 and enc(F32(-1e-12)) == 32767                   # (32768 - 6.4e-41 rounds to 32768 in float64)


def test_rgb_is_within_one_level_and_differs_almost_nowhere(runs):
    rec = np.load(os.path.join(GOLDEN, 'export_rgb.npz'))
    differing = total = 0
    for tag, (pred, valid, got, got_nv, want, want_nv) in runs.items():
        assert np.array_equal(got['color'], got_nv['color']), tag                    # the validity plane does not colour anything
        d = np.abs(got['color'].astype(np.int32) - want['color'].astype(np.int32))
        print('%-28s values %8d  differing %4d  largest difference %d' % (tag, d.size, int((d > 0).sum()), int(d.max())))
        assert d.max() <= 1, (tag, int(d.max()), np.argwhere(d > 1)[:4])
        differing += int((d > 0).sum())
        total += d.size
        if tag.startswith('golden/') and tag[7:] in rec.files:                      # ... and of the reference's own picture
            assert np.abs(got['color'][0].astype(np.int32) - rec[tag[7:]]).max() <= 1, tag
    print('rgb values differing from the model: %d of %d' % (differing, total))
    assert total > 2_000_000 and differing * 10_000 <= total


def test_planted_pixels_are_exact(runs):
    rec = np.load(os.path.join(GOLDEN, 'export_rgb.npz'))
    assert (runs['golden/zero'][2]['color'] == 255).all()                           # no motion: white
    for name in ('axes8', 'axes4'):                                                 # the axis and diagonal colours
        assert np.array_equal(runs['golden/' + name][2]['color'][0], rec[name]), name
    unk = runs['golden/unknown'][2]['color'][0]
    assert all((unk[y, x] == 0).all() for y, x in ((0, 0), (1, 5), (2, 9), (3, 13), (8, 69)))
    for tag, (pred, valid, got, *_rest) in runs.items():                             # unknown and NaN pixels: black, all of them
        blk = em.black(pred[:, 0], pred[:, 1])
        assert (got['color'][blk] == 0).all(), tag
        nan = np.isnan(pred).any(axis=1)
        assert (got['kitti'][nan] == 0).all(), tag
    assert em.black(runs['random/1x375x1242 wild'][0][:, 0], runs['random/1x375x1242 wild'][0][:, 1]).sum() >= 5
    checked = 0
    for name, frame in em.golden_frames().items():                                  # the largest pixel, on the reference's side of rad <= 1
        tag = 'golden/' + name
        if tag in runs and name != 'zero':
            _, _, rad, _ = em.scaled(frame)
            y, x = np.unravel_index(np.argmax(rad), rad.shape)
            assert np.array_equal(runs[tag][2]['color'][0, y, x], rec[name][y, x]), (name, rad[y, x] - 1.0)
            checked += rad[y, x] > 1.0
    assert checked >= 3


def test_a_given_max_rad_equals_the_model_in_one_launch():
    from upflow_pytorch_amd import ops
    differing = total = 0
    for (B, H, W), max_rad in (((2, 33, 130), 2.5), ((1, 9, 70), 100.0), ((2, 7, 13), 0.1)):
        pred = random_pred(7, B, H, W, TAME)
        ws = ops.flow_export_workspace(DEV, B, H, W)
        ws.fill_(0xA5)
        got = ops.flow_export(dev(pred), color=True, kitti=True, max_rad=max_rad)
        ops.flow_export(dev(pred), kitti=True, flo=True)                            # no colours: no maximum either
        torch.cuda.synchronize()
        assert bool((ws == 0xA5).all())                                             # the partial-maxima launch did not run
        want = em.export(pred, max_rad=max_rad)
        d = np.abs(got['color'].cpu().numpy().astype(np.int32) - want['color'].astype(np.int32))
        assert d.max() <= 1 and np.array_equal(got['kitti'].cpu().numpy(), want['kitti'])
        differing += int((d > 0).sum())
        total += d.size
        assert not np.array_equal(want['color'], em.export(pred)['color'])
        for per_item in (None, 0.0, -1.0, float('nan')):                            # ... and these mean "per item": two launches
            ws.fill_(0xA5)
            own = ops.flow_export(dev(pred), color=True, max_rad=per_item)['color'].cpu().numpy()
            assert not bool((ws == 0xA5).all())
            assert np.abs(own.astype(np.int32) - em.export(pred)['color']).max() <= 1
    assert differing * 10_000 <= total


def test_two_runs_give_equal_bits(runs):
    for tag in ('random/2x33x130 wild', 'random/1x375x1242 tame'):
        pred, valid, got = runs[tag][:3]
        again = export(pred, valid, kitti=True, color=True, flo=True)
        for k in got:
            assert np.array_equal(bits(got[k]), bits(again[k])), (tag, k)


def test_the_maximum_is_per_item(runs):
    for tag in ('golden/33x130 pair', 'random/2x33x130 wild', 'random/2x7x13 tame'):
        pred, valid, got = runs[tag][:3]
        for i in range(2):
            one = export(pred[i:i + 1], valid[i:i + 1], kitti=True, color=True, flo=True)
            for k in got:
                assert np.array_equal(bits(got[k][i:i + 1]), bits(one[k])), (tag, i, k)
    a, b = runs['golden/33x130 pair'][0]
    assert em.maxrad(a.transpose(1, 2, 0)) != em.maxrad(b.transpose(1, 2, 0))


def test_outputs_into_slices_leave_the_guards_intact(runs):
    from upflow_pytorch_amd import ops
    specs = {'kitti': (torch.uint16, 3), 'color': (torch.uint8, 3), 'flo': (torch.float32, 2)}
    guard = 0xEE                                                                     # every byte outside the outputs
    for tag in ('random/2x7x13 wild', 'random/2x33x130 tame', 'random/1x3x5 tame', 'random/1x1x1 tame'):
        pred, valid, got = runs[tag][:3]
        B, _, H, W = pred.shape
        # items 1 .. B of a [B+2,...] tensor, and the middle of a flat buffer that starts 3 elements in: an address that is only
        # element-aligned, where the kernel must fall back to narrow stores
        for pad in (None, 3):
            big, out = {}, {}
            for k, (dt, last) in specs.items():
                n = B * H * W * last
                lead = H * W * last if pad is None else pad
                big[k] = torch.full(((n + 2 * lead) * dt.itemsize,), guard, dtype=torch.uint8, device=DEV).view(dt)
                out[k] = big[k][lead:lead + n].view(B, H, W, last)
            res = ops.flow_export(dev(pred), dev(valid), out=out)
            assert sorted(res) == ['color', 'flo', 'kitti'] and all(res[k].data_ptr() == out[k].data_ptr() for k in res)
            for k, (dt, last) in specs.items():
                n = B * H * W * last
                lead = H * W * last if pad is None else pad
                assert np.array_equal(bits(res[k].cpu().numpy()), bits(got[k])), (tag, pad, k)
                edges = (big[k][:lead].view(torch.uint8), big[k][lead + n:].view(torch.uint8))
                assert all(e.numel() == lead * dt.itemsize and bool((e == guard).all()) for e in edges), (tag, pad, k)
    only = ops.flow_export(dev(pred), flo=True)                                      # one output asked for: one returned
    assert list(only) == ['flo']


def test_arguments_are_checked():
    from upflow_pytorch_amd import ops
    B, H, W = 2, 6, 10
    pred = dev(random_pred(1, B, H, W, []))
    valid = torch.ones(B, 1, H, W, device=DEV)
    u16 = lambda *s: torch.empty(*s, dtype=torch.uint16, device=DEV)               # noqa: E731
    bad = [
        lambda: ops.flow_export(pred.cpu(), kitti=True),                                            # a CPU tensor
        lambda: ops.flow_export(pred, valid.cpu(), kitti=True),
        lambda: ops.flow_export(pred.half(), kitti=True),                                           # an fp16 prediction
        lambda: ops.flow_export(pred, valid.half(), kitti=True),
        lambda: ops.flow_export(pred.transpose(2, 3).contiguous().transpose(2, 3), kitti=True),     # not contiguous
        lambda: ops.flow_export(pred, valid.transpose(2, 3).contiguous().transpose(2, 3), kitti=True),
        lambda: ops.flow_export(pred[:, :1], kitti=True),                                           # one channel
        lambda: ops.flow_export(pred[0], kitti=True),                                               # three dimensions
        lambda: ops.flow_export(pred, valid[:1], kitti=True),                                       # another batch
        lambda: ops.flow_export(pred, valid[:, 0], kitti=True),                                     # [B,H,W]
        lambda: ops.flow_export(pred),                                                              # nothing asked for
        lambda: ops.flow_export(pred, out={'kitti': u16(B, H, W, 3).view(torch.int16)}),            # wrong out dtype
        lambda: ops.flow_export(pred, out={'color': u16(B, H, W, 3)}),
        lambda: ops.flow_export(pred, out={'flo': torch.empty(B, H, W, 2, dtype=torch.float64, device=DEV)}),
        lambda: ops.flow_export(pred, out={'kitti': u16(B, H, W, 2)}),                              # wrong out shape
        lambda: ops.flow_export(pred, out={'kitti': u16(B + 1, H, W, 3)}),
        lambda: ops.flow_export(pred, out={'flo': torch.empty(B, 2, H, W, device=DEV)}),
        lambda: ops.flow_export(pred, out={'kitti': u16(B, H, W, 6)[..., ::2]}),                    # a strided out
        lambda: ops.flow_export(pred, out={'kitti': torch.empty(B, H, W, 3, dtype=torch.uint16)}),  # out on the CPU
        lambda: ops.flow_export(pred, out={'png': u16(B, H, W, 3)}),                                # an unknown output
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail('case %d was accepted' % i)
    assert sorted(ops.flow_export(pred, valid, kitti=True, color=True, flo=True)) == ['color', 'flo', 'kitti']


# ---- Test_model(save_dir=...) ------------------------------------------------------------------------------------------------------
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
    return [dev(random_pred(20 + i, 1, *sizes[i % 4], TAME)) for i in range(n)]


def read(path):
    with open(path, 'rb') as f:
        return f.read()


def test_saved_files_are_the_host_writers(tmp_path):
    from upflow_pytorch_amd import ops
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow
    from upflow_pytorch_amd.utils import flow_io
    from upflow_pytorch_amd.utils.tools import tools
    preds = frames_of(6)
    names = ['%06d_10' % i for i in range(6)]
    ds = [(torch.zeros(3, p.shape[2], p.shape[3]), torch.zeros(3, p.shape[2], p.shape[3]), n) for p, n in zip(preds, names)]
    save_dir = str(tmp_path / 'out')
    model = fake_model(preds, save_dir=save_dir, save=('kitti', 'color', 'flo'), save_workers=2)
    assert model.saver.pool._max_workers == 2
    assert kitti_flow.Evaluation_bench('2015_test', batch_size=1, dataset=ds)(model) is None
    model.flush()                                                                    # from here on the files are complete
    assert sorted(os.listdir(save_dir)) == ['color', 'flo', 'flow']
    assert sorted(os.listdir(os.path.join(save_dir, 'flow'))) == [n + '.png' for n in names]
    assert sorted(os.listdir(os.path.join(save_dir, 'color'))) == [n + '.png' for n in names]
    assert sorted(os.listdir(os.path.join(save_dir, 'flo'))) == [n + '.flo' for n in names]
    host = str(tmp_path / 'host')
    for p, n in zip(preds, names):
        frame = np.ascontiguousarray(p[0].permute(1, 2, 0).cpu().numpy())
        flow_io.write_kitti_png_file(host, frame)
        assert read(os.path.join(save_dir, 'flow', n + '.png')) == read(host), n
        flow_io.write_flo(frame, host)
        assert read(os.path.join(save_dir, 'flo', n + '.flo')) == read(host), n
        # the picture: the file of the device's own payload byte for byte, and that within a level of the host renderer's
        flow_io.write_png(host, ops.flow_export(p, color=True)['color'][0].cpu().numpy())
        assert read(os.path.join(save_dir, 'color', n + '.png')) == read(host), n
        pic = flow_io.read_png(os.path.join(save_dir, 'color', n + '.png'))
        assert np.abs(pic.astype(np.int32) - tools.flow_to_image(frame)).max() <= 1
    # the training sets' call: a name with the metrics in it and the occlusion mask as the validity plane
    mask = (torch.rand(1, 1, 32, 64, device=DEV) > 0.4).float()
    model.eval_save_result('all_1.00 f1_2.0 noc_3.00 occ_4.00__0', preds[0], occmask=mask)
    model.close()
    flow_io.write_kitti_png_file(host, preds[0][0].permute(1, 2, 0).cpu().numpy(), mask[0, 0].cpu().numpy())
    assert read(os.path.join(save_dir, 'flow', 'all_1.00 f1_2.0 noc_3.00 occ_4.00__0.png')) == read(host)
    assert model.saver.pool is None and not [t for t in threading.enumerate() if t.name.startswith('upflow-save')]
    with pytest.raises(RuntimeError):
        model.eval_save_result('late', preds[0])


def test_a_small_ring_still_writes_everything_and_a_given_scale_reaches_the_kernel(tmp_path):
    from upflow_pytorch_amd.result_saver import ResultSaver
    from upflow_pytorch_amd.utils import flow_io
    preds = frames_of(9)
    saver = ResultSaver(str(tmp_path), save='color', workers=1, slots=1, max_rad=5.0)   # every submit but the first waits for the slot
    for i, p in enumerate(preds):
        saver.submit('f%d' % i, p)
    saver.close()
    assert sorted(os.listdir(str(tmp_path))) == ['color']
    for i, p in enumerate(preds):
        want = em.export(p.cpu().numpy(), max_rad=5.0)['color'][0]
        assert np.abs(flow_io.read_png(str(tmp_path / 'color' / ('f%d.png' % i))).astype(np.int32) - want).max() <= 1
    with pytest.raises(ValueError):
        ResultSaver(str(tmp_path), save=('jpeg',))
    with pytest.raises(ValueError):
        ResultSaver(str(tmp_path), workers=0)


def test_a_worker_exception_surfaces(tmp_path, monkeypatch):
    from upflow_pytorch_amd import result_saver
    preds = frames_of(3)
    model = fake_model(preds, save_dir=str(tmp_path), save=('kitti', 'flo'))

    def broken(fn, payload):
        raise OSError('disk full: ' + os.path.basename(fn))
    monkeypatch.setitem(result_saver._WRITERS, 'kitti', broken)
    for i, p in enumerate(preds):
        model.eval_save_result('n%d' % i, p)
    with pytest.raises(OSError, match='disk full: n0.png'):
        model.flush()
    model.flush()                                                                    # (raised once; the queue is empty again)
    monkeypatch.undo()
    model.eval_save_result('fine', preds[0])                                         # every slot came back: the saver still works
    model.close()
    assert os.path.exists(str(tmp_path / 'flow' / 'fine.png'))


def test_without_a_save_dir_the_name_is_printed(capsys, tmp_path):
    preds = frames_of(1)
    model = fake_model(preds)
    assert model.saver is None
    capsys.readouterr()
    model.eval_save_result('000003_10', preds[0], occmask=None)
    model.flush()
    model.close()
    assert capsys.readouterr().out == '000003_10\n'
    assert os.listdir(str(tmp_path)) == []
