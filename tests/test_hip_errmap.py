"""upf_flow_error_image on the GPU (csrc/errmap.hip; ops.flow_error_image) and the 'error' kind of ResultSaver / Test_model built on
it.  The yardstick is the numpy model of tests/_errmap_model.py, which gives the reference's bytes at every pixel of the fixture
(test_errmap_model_cpu.py).  Every step of the contract is a correctly rounded fp32 operation and every comparison is against an
fp32 constant, so the condition is EQUAL bytes — no tolerance.

Shapes: one pixel; 2x13x37 (odd everything, two items, the second at an odd offset); 1x5x4099 (rows of odd byte length, H*W not a
multiple of 4, beyond one workgroup of 256 lanes x 4 pixels, a scalar tail); 1x70x150 (beyond the dilate kernel's 32 x 64 tile in
both directions, ragged last tiles)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _errmap_model as M
import _score_model as S

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32 = np.float32
SHAPES = [(1, 1, 1), (2, 13, 37), (1, 5, 4099), (1, 70, 150)]
TH, TW = 32, 64                                                # the dilate kernel's tile (csrc/errmap.hip)
SPECIAL = [F32(np.nan), F32(np.inf), F32(-np.inf), F32(4e9), F32(2.9999e9), F32(-3e38)]
MASKS = np.array([0, 1, 1, 0, 1, 0, 0, 0, 2, 256, 257, 255], dtype=np.uint16)      # mostly {0, 1}; 2 and 255: valid, occluded; 256: 0


def planted_positions(H, W):
    """valid pixels that must be there: the corners, the last row and column, both sides of every tile edge"""
    pos = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    pos |= {(H - 1, x) for x in range(0, W, 7)} | {(y, W - 1) for y in range(0, H, 5)}
    for xe in range(TW, W, TW):
        pos |= {(y, x) for y in range(0, H, 3) for x in (xe - 1, xe)}
    for ye in range(TH, H, TH):
        pos |= {(y, x) for x in range(0, W, 3) for y in (ye - 1, ye)}
    return sorted(pos)


_cases = {}


def case(shape):
    """-> (pred fp32 [B,2,H,W], gt_occ, gt_noc uint16 [B,H,W,3]), made once per shape and never modified"""
    if shape not in _cases:
        B, H, W = shape
        g = np.random.default_rng(1000 * B + 10 * H + W)
        gt = g.integers(-90 * 64, 90 * 64 + 1, size=(B, H, W, 2)) / 64.0
        gt[g.random((B, H, W)) < 0.2] = 0                                             # |gt| = 0: the 1e-7 of the relative term
        ang = g.uniform(0, 2 * np.pi, (B, H, W))
        mag = np.exp(g.uniform(np.log(0.01), np.log(80.0), (B, H, W)))
        on = g.random((B, H, W)) < 0.3                                                # diff / 3 ON a bin bound (up to pred's rounding)
        mag = np.where(on, 3 * M.LO[g.integers(1, 10, (B, H, W))].astype(np.float64), mag)
        pred = np.stack([gt[..., 0] + mag * np.cos(ang), gt[..., 1] + mag * np.sin(ang)], axis=1).astype(F32)
        b_occ = np.where(g.random((B, H, W)) < 0.15, MASKS[g.integers(0, len(MASKS), (B, H, W))], 0).astype(np.uint16)
        b_noc = MASKS[g.integers(0, len(MASKS), (B, H, W))]
        for y, x in planted_positions(H, W):
            b_occ[:, y, x] = 1
        if B * H * W > 1:                                                             # the non-finite and huge values: anywhere, and
            flat = pred.reshape(-1)                                                   # in valid pixels (a black pixel that still paints)
            flat[g.permutation(flat.size)[:len(SPECIAL)]] = np.array(SPECIAL)
            vb, vy, vx = np.nonzero((b_occ & 255) != 0)
            for k, j in enumerate(g.permutation(len(vb))[:len(SPECIAL)]):
                pred[vb[j], k % 2, vy[j], vx[j]] = SPECIAL[k]
        q = (np.rint(gt * 64) + 32768).astype(np.uint16)
        gt_occ = np.concatenate([q, b_occ[..., None]], axis=-1)
        gt_noc = np.concatenate([g.integers(0, 65536, (B, H, W, 2)).astype(np.uint16), b_noc[..., None]], axis=-1)   # its flow is not read
        _cases[shape] = (pred, gt_occ, gt_noc)
    return _cases[shape]


_models = {}


def model(shape, log_colors, r):
    key = (shape, log_colors, r)
    if key not in _models:
        base = (shape, log_colors, 'plain')
        if base not in _models:
            _models[base] = M.render(*case(shape), log_colors)
        _models[key] = M.dilate(*_models[base], r)
    return _models[key]


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def differing(got, want):
    wrong = np.argwhere(np.any(got != want, axis=-1))
    return '%d of %d pixels differ, first at %s: got %s, want %s' % (
        len(wrong), want[..., 0].size, wrong[:3].tolist(), [got[tuple(w)].tolist() for w in wrong[:3]], [want[tuple(w)].tolist() for w in wrong[:3]])


def test_the_cases_hold_what_they_should():
    for shape in SHAPES[1:]:
        B, H, W = shape
        pred, gt_occ, gt_noc = case(shape)
        rgb, valid = M.render(pred, gt_occ, gt_noc, True)
        assert valid[:, 0, 0].all() and valid[:, 0, W - 1].all() and valid[:, H - 1, 0].all() and valid[:, H - 1, W - 1].all()
        assert 0.05 < valid.mean() < 0.6 and np.isnan(pred).any() and np.isinf(pred).any()
        m_occ, m_noc = S.decode(gt_occ)[1], S.decode(gt_noc)[1]
        assert {(0, 0), (0, 1), (1, 0), (1, 1)} <= {(int(a), int(b)) for a, b in zip(m_occ.ravel(), m_noc.ravel())}
        assert (m_occ > 1).any() and (m_noc > 1).any()                                # masks outside {0, 1} are there too
        # every colour of both tables (but for the smallest frame: most of them) and black among the valid pixels
        colours = {tuple(c) for c in rgb[valid]}
        assert (0, 0, 0) in colours and len(colours & ({tuple(c) for c in M.FULL} | {tuple(c) for c in M.HALF})) >= (20 if B * H * W > 2000 else 8)
        # two valid pixels compete for an invalid pixel's window, at r = 1 already: painting in REVERSE order gives another picture
        first_wins = M.dilate(rgb[:, ::-1, ::-1], valid[:, ::-1, ::-1], 1)[:, ::-1, ::-1]
        assert np.any(first_wins != M.dilate(rgb, valid, 1))
    B, H, W = SHAPES[3]
    assert H > 2 * TH and W > 2 * TW and H <= 128 and W <= 256 and H % TH and W % TW
    valid = M.render(*case(SHAPES[3]), True)[1]
    assert valid[0, :, TW - 1].any() and valid[0, :, TW].any() and valid[0, :, 2 * TW - 1].any() and valid[0, :, 2 * TW].any()
    assert valid[0, TH - 1].any() and valid[0, TH].any() and valid[0, 2 * TH - 1].any() and valid[0, 2 * TH].any()


@pytest.mark.parametrize('dilate', [0, 1, 4])
@pytest.mark.parametrize('log_colors', [True, False], ids=['log', 'linear'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_bytes_equal_the_model(shape, log_colors, dilate):
    from upflow_pytorch_amd import ops
    pred, gt_occ, gt_noc = dev(*case(shape))
    out = ops.flow_error_image(pred, gt_occ, gt_noc, log_colors=log_colors, dilate=dilate)
    assert out.dtype == torch.uint8 and tuple(out.shape) == shape + (3,) and out.is_cuda and out.is_contiguous()
    again = ops.flow_error_image(pred, gt_occ, gt_noc, log_colors=log_colors, dilate=dilate)
    got, want = out.cpu().numpy(), model(shape, log_colors, dilate)
    assert np.array_equal(got, want), differing(got, want)
    assert torch.equal(out, again)                                                     # two runs: the same bytes


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_minimum_alignment_out_and_guards(shape):
    """pred 8 bytes, the ground truth 4 bytes and rgb 1 byte off a fresh allocation — the least the contract admits, where the kernel
    must fall back to narrower accesses — and `out` in the middle of a guarded buffer: nothing but rgb is written."""
    from upflow_pytorch_amd import ops
    B, H, W = shape
    pred, gt_occ, gt_noc = case(shape)
    n = B * H * W

    def shifted(a, dtype, lead):
        buf = torch.zeros(a.size + lead + 8, dtype=dtype, device=DEV)
        assert buf.data_ptr() % 256 == 0
        view = buf[lead:lead + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        return buf, view

    keep_p, p = shifted(pred, torch.float32, 2)
    keep_o, o = shifted(gt_occ, torch.uint16, 2)
    keep_c, c = shifted(gt_noc, torch.uint16, 2)
    assert p.data_ptr() % 16 == 8 and o.data_ptr() % 8 == 4 and c.data_ptr() % 8 == 4
    guard = 0xEE
    for lead in (1, 2, 3, 64):
        for log_colors, r in ((True, 0), (False, 0), (True, 1), (False, 4), (True, 4)):
            big = torch.full((3 * n + 2 * lead,), guard, dtype=torch.uint8, device=DEV)
            out = big[lead:lead + 3 * n].view(B, H, W, 3)
            res = ops.flow_error_image(p, o, c, log_colors=log_colors, dilate=r, out=out)
            assert res.data_ptr() == out.data_ptr() == big.data_ptr() + lead
            got, want = res.cpu().numpy(), model(shape, log_colors, r)
            assert np.array_equal(got, want), ((lead, log_colors, r), differing(got, want))
            assert bool((big[:lead] == guard).all()) and bool((big[lead + 3 * n:] == guard).all()), (lead, log_colors, r)
    # the inputs are read only
    assert np.array_equal(p.cpu().numpy().view(np.uint32), pred.view(np.uint32)) and np.array_equal(o.cpu().numpy(), gt_occ) and np.array_equal(c.cpu().numpy(), gt_noc)


def test_items_are_rendered_on_their_own():
    """an item of a batch gives the bytes it gives alone (no window reaches into the neighbouring item)"""
    from upflow_pytorch_amd import ops
    shape = SHAPES[1]
    pred, gt_occ, gt_noc = case(shape)
    for r in (0, 4):
        want = model(shape, True, r)
        for b in range(shape[0]):
            got = ops.flow_error_image(*dev(pred[b:b + 1], gt_occ[b:b + 1], gt_noc[b:b + 1]), dilate=r).cpu().numpy()
            assert np.array_equal(got[0], want[b]), (r, b)


def test_the_fixture_on_the_device():
    """the reference's own bytes, straight from the fixture"""
    from conftest import ROOT
    from upflow_pytorch_amd import ops
    fx = np.load(os.path.join(ROOT, 'tests', 'golden', 'errmap.npz'))
    for log_colors, key in ((True, 'ref_log'), (False, 'ref_lin')):
        with np.errstate(invalid='ignore'):
            x = np.rint(255.0 * fx[key][:, :, ::-1])
        want = np.where(np.isnan(x), 0.0, x).astype(np.uint8)
        got = ops.flow_error_image(*dev(fx['pred'], fx['gt_occ'], fx['gt_noc']), log_colors=log_colors).cpu().numpy()[0]
        assert np.array_equal(got, want), differing(got, want)


def test_error_codes():
    from upflow_pytorch_amd import _lib
    L = _lib.lib()
    EINVAL, EALIGN, EUNSUPPORTED = -1, -3, -4
    B, H, W = 2, 6, 10
    pred, gt_occ, gt_noc = dev(*case(SHAPES[1]))
    rgb = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV)
    P, O, C, R = (_lib.ptr(t) for t in (pred, gt_occ, gt_noc, rgb))
    null = ctypes.c_void_p(0)
    stream = _lib.stream_ptr(pred.device)

    def call(p=P, o=O, c=C, r=R, lc=1, d=0, b=B, h=H, w=W):
        return L.upf_flow_error_image(p, o, c, r, lc, d, null, b, h, w, stream)
    assert call() == 0
    assert call(p=null) == EINVAL and call(o=null) == EINVAL and call(c=null) == EINVAL and call(r=null) == EINVAL
    assert call(b=0) == EINVAL and call(h=0) == EINVAL and call(w=-1) == EINVAL
    assert call(d=-1) == EINVAL and call(d=5) == EINVAL
    assert call(b=2, h=32768, w=32768) == EUNSUPPORTED and call(b=1, h=65536, w=32768, d=1) == EUNSUPPORTED
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)                              # noqa: E731
    assert call(p=off(pred, 4)) == EALIGN and call(o=off(gt_occ, 2)) == EALIGN and call(c=off(gt_noc, 2)) == EALIGN
    assert call(p=off(pred, 8), o=off(gt_occ, 4), c=off(gt_noc, 4), r=off(rgb, 1), b=1) == 0
    nbytes = ctypes.c_longlong(-1)
    assert L.upf_flow_error_image_workspace_bytes(B, H, W, 4, ctypes.byref(nbytes)) == 0 and nbytes.value == 0
    assert L.upf_flow_error_image_workspace_bytes(2, 32768, 32768, 0, ctypes.byref(nbytes)) == EUNSUPPORTED
    torch.cuda.synchronize()


def test_arguments_are_checked():
    from upflow_pytorch_amd import ops
    shape = SHAPES[1]
    B, H, W = shape
    pred, gt_occ, gt_noc = dev(*case(shape))
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device=DEV)                     # noqa: E731
    bad = [
        lambda: ops.flow_error_image(pred.cpu(), gt_occ, gt_noc),                                   # a CPU tensor
        lambda: ops.flow_error_image(pred, gt_occ.cpu(), gt_noc),
        lambda: ops.flow_error_image(pred.half(), gt_occ, gt_noc),                                  # callers promote, not the op
        lambda: ops.flow_error_image(pred, gt_occ.view(torch.int16), gt_noc),
        lambda: ops.flow_error_image(pred, gt_occ, gt_noc[..., :2]),
        lambda: ops.flow_error_image(pred, gt_occ[:1], gt_noc),
        lambda: ops.flow_error_image(pred[:, :1], gt_occ, gt_noc),
        lambda: ops.flow_error_image(pred.transpose(2, 3).contiguous().transpose(2, 3), gt_occ, gt_noc),
        lambda: ops.flow_error_image(pred, gt_occ, gt_noc, dilate=5),
        lambda: ops.flow_error_image(pred, gt_occ, gt_noc, dilate=-1),
        lambda: ops.flow_error_image(pred, gt_occ, gt_noc, dilate=1.0),
        lambda: ops.flow_error_image(pred, gt_occ, gt_noc, out=u8(B, H, W, 4)),
        lambda: ops.flow_error_image(pred, gt_occ, gt_noc, out=u8(B, H, W, 3).view(torch.int8)),
        lambda: ops.flow_error_image(pred, gt_occ, gt_noc, out=u8(B, H, W, 6)[..., ::2]),
        lambda: ops.flow_error_image(pred, gt_occ, gt_noc, out=torch.empty(B, H, W, 3, dtype=torch.uint8)),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            pytest.fail('case %d was accepted' % i)
    assert ops.flow_error_image(pred, gt_occ, gt_noc).shape == (B, H, W, 3)


# ---- the saving path ---------------------------------------------------------------------------------------------------------------
def small_dataset():
    g = torch.Generator().manual_seed(11)
    ds, preds = [], []
    for i in range(3):
        B, H, W = 1, 24, 40
        gg = np.random.default_rng(70 + i)
        gt = gg.integers(-60 * 64, 60 * 64 + 1, size=(H, W, 2)) / 64.0
        mag = np.exp(gg.uniform(np.log(0.02), np.log(40.0), (H, W)))
        ang = gg.uniform(0, 2 * np.pi, (H, W))
        pred = np.stack([gt[..., 0] + mag * np.cos(ang), gt[..., 1] + mag * np.sin(ang)], axis=0).astype(F32)[None]
        b_occ = (gg.random((H, W)) < 0.3).astype(np.uint16)
        b_noc = (b_occ * (gg.random((H, W)) < 0.7)).astype(np.uint16)
        q = (np.rint(gt * 64) + 32768).astype(np.uint16)
        gt_occ, gt_noc = np.concatenate([q, b_occ[..., None]], -1), np.concatenate([q, b_noc[..., None]], -1)
        ds.append((torch.randn(3, H, W, generator=g), torch.randn(3, H, W, generator=g), torch.from_numpy(gt_occ), torch.from_numpy(gt_noc)))
        preds.append(pred)
    return ds, preds


def fake_model(preds, **kw):
    from upflow_pytorch_amd.test import Test_model

    class Fake(Test_model):
        def __init__(self):
            super(Fake, self).__init__(pretrain_path=None, net=torch.nn.Identity(), graph=False, **kw)
            self.calls = 0

        def eval_forward(self, im1, im2, gt, *args):
            self.calls += 1
            return torch.from_numpy(preds[self.calls - 1]).to(DEV)

    return Fake()


def read(path):
    with open(path, 'rb') as f:
        return f.read()


def by_index(names):
    return sorted(names, key=lambda n: int(n.rsplit('.', 1)[0].rsplit('__', 1)[1]))


def test_evaluation_saves_error_maps(tmp_path):
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow
    from upflow_pytorch_amd.utils import flow_io
    ds, preds = small_dataset()

    def run(tag, **kw):
        model_ = fake_model(preds, save_dir=str(tmp_path / tag), **kw)
        try:
            scores = kitti_flow.Evaluation_bench('2015_train', batch_size=1, dataset=ds, device_score=True)(model_)
        finally:
            model_.close()
        return scores

    plain = run('plain', save=('kitti',))
    results = {}
    for tag, kw in (('host', {}), ('device', {'png': 'device'}), ('dilated', {'png': 'device', 'error_dilate': 2, 'error_log_colors': False})):
        results[tag] = run(tag, save=('kitti', 'error'), **kw)
        assert sorted(os.listdir(str(tmp_path / tag))) == ['error', 'flow']
        flows, errors = by_index(os.listdir(str(tmp_path / tag / 'flow'))), by_index(os.listdir(str(tmp_path / tag / 'error')))
        assert flows == errors and len(errors) == 3 and flows == by_index(os.listdir(str(tmp_path / 'plain' / 'flow')))
        lc, r = (False, 2) if tag == 'dilated' else (True, 0)
        for i, name in enumerate(errors):
            pic = flow_io.read_png(str(tmp_path / tag / 'error' / name))
            want = M.flow_error_image(preds[i], ds[i][2].numpy()[None], ds[i][3].numpy()[None], lc, r)[0]
            assert pic.dtype == np.uint8 and np.array_equal(pic, want), (tag, name)
            if tag == 'host':                                                          # the flow files: the bytes of a run without 'error'
                assert read(str(tmp_path / tag / 'flow' / name)) == read(str(tmp_path / 'plain' / 'flow' / name)), name
        if tag == 'host':                                                              # ... and the file of the host route, byte for byte
            for i, name in enumerate(errors):
                flow_io.write_png(str(tmp_path / 'one.png'), M.flow_error_image(preds[i], ds[i][2].numpy()[None], ds[i][3].numpy()[None])[0])
                assert read(str(tmp_path / 'host' / 'error' / name)) == read(str(tmp_path / 'one.png'))
    assert results['host'] == results['device'] == results['dilated'] == plain         # the four scores, to the bit
    # png='device' changes the flow file's bytes for every kind, with or without 'error': compared among themselves
    only_flow = run('device_plain', save=('kitti',), png='device')
    assert only_flow == plain
    for name in os.listdir(str(tmp_path / 'device' / 'flow')):
        assert read(str(tmp_path / 'device' / 'flow' / name)) == read(str(tmp_path / 'device_plain' / 'flow' / name))


def test_other_hooks_see_the_calls_they_always_saw():
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow
    from upflow_pytorch_amd.utils.tools import tools
    ds, preds = small_dataset()

    class Model(tools.abs_test_model):
        wants = None

        def __init__(self):
            super(Model, self).__init__()
            self.seen, self.calls = [], 0
            if self.wants is not None:
                self.wants_gt_u16 = self.wants

        def eval_forward(self, im1, im2, gt, *args):
            self.calls += 1
            return torch.from_numpy(preds[self.calls - 1]).to(DEV)

        def eval_save_result(self, save_name, predflow, *args, **kwargs):
            self.seen.append((args, kwargs))

    for wants in (None, False, True):
        Model.wants = wants
        m = Model()
        kitti_flow.Evaluation_bench('2015_train', batch_size=1, dataset=ds, device_score=True)(m)
        assert len(m.seen) == 3
        for i, (args, kwargs) in enumerate(m.seen):
            assert args == ()
            if not wants:
                assert sorted(kwargs) == ['occmask']
            else:
                assert sorted(kwargs) == ['gt_noc_u16', 'gt_occ_u16', 'occmask']
                assert kwargs['gt_occ_u16'].is_cuda and kwargs['gt_occ_u16'].dtype == torch.uint16
                assert torch.equal(kwargs['gt_occ_u16'].cpu(), ds[i][2][None]) and torch.equal(kwargs['gt_noc_u16'].cpu(), ds[i][3][None])


def test_error_without_ground_truth_raises(tmp_path, monkeypatch):
    from upflow_pytorch_amd import ops
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow
    from upflow_pytorch_amd.result_saver import ResultSaver
    ds, preds = small_dataset()
    model_ = fake_model(preds, save_dir=str(tmp_path / 'a'), save=('kitti', 'error'))
    assert model_.wants_gt_u16 and not fake_model(preds, save_dir=str(tmp_path / 'b'), save=('kitti',)).wants_gt_u16
    with pytest.raises(ValueError, match='device_score=True'):
        model_.eval_save_result('000000_10', torch.from_numpy(preds[0]).to(DEV))
    test_set = [(it[0], it[1], '%06d_10' % i) for i, it in enumerate(ds)]
    with pytest.raises(ValueError, match='device_score=True'):                         # the _test sets: at the first submit
        kitti_flow.Evaluation_bench('2015_test', batch_size=1, dataset=test_set)(model_)
    model_.close()
    assert os.listdir(str(tmp_path / 'a' / 'error')) == [] and os.listdir(str(tmp_path / 'a' / 'flow')) == []
    with pytest.raises(ValueError):
        ResultSaver(str(tmp_path / 'c'), save=('error',), error_dilate=5)
    # 'error' alone: ops.flow_export is not called
    monkeypatch.setattr(ops, 'flow_export', lambda *a, **k: pytest.fail('flow_export was called'))
    saver = ResultSaver(str(tmp_path / 'd'), save='error', error_dilate=1)
    occ, noc = ds[0][2][None].to(DEV), ds[0][3][None].to(DEV)
    saver.submit('only', torch.from_numpy(preds[0]).to(DEV).bfloat16(), gt_occ_u16=occ, gt_noc_u16=noc)
    saver.close()
    from upflow_pytorch_amd.utils import flow_io
    want = M.flow_error_image(torch.from_numpy(preds[0]).bfloat16().float().numpy(), ds[0][2].numpy()[None], ds[0][3].numpy()[None], True, 1)[0]
    assert os.listdir(str(tmp_path / 'd')) == ['error'] and np.array_equal(flow_io.read_png(str(tmp_path / 'd' / 'error' / 'only.png')), want)
