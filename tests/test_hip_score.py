"""upf_kitti_score on the GPU (csrc/score.hip; ops.kitti_score) and the evaluation loop built on it
(kitti_flow.Evaluation_bench(device_score=True)).

The exact yardstick is the numpy model of tests/_score_model.py — correctly rounded fp32 steps, float64 / integer sums — never
torch's CPU spelling, whose fp32 sqrt is off by one ulp often enough to move the F1 count of pixels that sit on their threshold.
Bounds: counts are integers and must be EQUAL; a float64 sum of n terms taken in another order differs by at most
2 * (n - 1) * 2^-53 * sum|term| <= n * 2^-52 * sum|term| (sum|term| is the sum itself for the non-negative S_occ and S_noc); the four
values are two or three float64 operations on the sums: 4 ulp.  Against the product's own torch spelling (fp32 tensors, fp32
summation) the bound is the spelling's: n * 2^-24 relative."""
import math
import re

import numpy as np
import pytest
import torch

import _score_model as sm
import _weights

pytestmark = pytest.mark.gpu

DEV = 'cuda'
VALID = np.array([0, 1, 2, 256, 257], dtype=np.uint16)        # weights 0, 1, 2, 0, 1
KINDS = ('subset', 'not_subset', 'full', 'empty')


def make_case(seed, B, H, W, kind, gap=False, reach=60):
    """-> (pred fp32 [B,2,H,W], gt_occ, gt_noc uint16 [B,H,W,3]).  Ground truth random within +-reach px; the error of every pixel
    is thr / weight * scale * (cos a, sin a): scale = 1 (ON the pixel's own threshold to within fp32 rounding) for half of the
    pixels and uniform in [0, 2] for the rest — or, gap=True, uniform in [0, 0.9) u [1.1, 2) for all."""
    g = np.random.default_rng(seed)
    q = g.integers(-reach * 64, reach * 64 + 1, size=(B, H, W, 2))
    qn = np.where(g.random((B, H, W, 1)) < 0.1, g.integers(-reach * 64, reach * 64 + 1, size=(B, H, W, 2)), q)   # noc file: its own flow
    if kind == 'full':
        v_occ = v_noc = np.ones((B, H, W), dtype=np.uint16)
    elif kind == 'empty':
        v_occ = v_noc = VALID[g.integers(0, 2, size=(B, H, W)) * 3]                                    # 0 and 256: weight 0
    else:
        v_occ = VALID[g.integers(0, 5, size=(B, H, W))]
        v_noc = np.where(g.random((B, H, W)) < 0.6, v_occ, 0).astype(np.uint16) if kind == 'subset' else VALID[g.integers(0, 5, size=(B, H, W))]
    gt_occ = np.concatenate([(q + 32768).astype(np.uint16), v_occ[..., None]], axis=-1)
    gt_noc = np.concatenate([(qn + 32768).astype(np.uint16), v_noc[..., None]], axis=-1)
    flow, m = sm.decode(gt_occ)
    thr = sm.threshold(flow[..., 0], flow[..., 1]).astype(np.float64)
    if gap:
        u = g.uniform(0.0, 1.8, size=(B, H, W))
        scale = np.where(u < 0.9, u, u + 0.2)
    else:
        scale = np.where(g.random((B, H, W)) < 0.5, 1.0, g.uniform(0.0, 2.0, size=(B, H, W)))
    a = g.uniform(0.0, 2.0 * np.pi, size=(B, H, W))
    err = thr * scale / np.where(m > 0, m, 1.0)
    pred = np.stack([flow[..., 0] - err * np.cos(a), flow[..., 1] - err * np.sin(a)], axis=1).astype(np.float32)
    return pred, gt_occ, gt_noc


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def run(pred, gt_occ, gt_noc, **kw):
    from upflow_pytorch_amd import ops
    row = ops.kitti_score(*dev(pred, gt_occ, gt_noc), **kw)
    assert row.dtype == torch.float64 and tuple(row.shape) == (12,) and row.is_cuda
    return row.cpu().numpy()


def same_value(got, want):
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= 4 * np.spacing(abs(want))


def check_row(row, pred, gt_occ, gt_noc, tag):
    s, want_row = sm.score(pred, gt_occ, gt_noc)
    n = pred.shape[0] * pred.shape[2] * pred.shape[3]
    got_counts = [row[5], row[6], row[8], row[10]]
    want_counts = [s['N_occ'], s['C_out'], s['N_noc'], s['N_oo']]
    print(tag, 'counts', got_counts, want_counts, 'sums', row[[4, 7, 9]], [s['S_occ'], s['S_noc'], s['S_oo']])
    assert all(float(g).is_integer() and int(g) == w for g, w in zip(got_counts, want_counts)), (tag, got_counts, want_counts)
    for i, key, scale in ((4, 'S_occ', s['S_occ']), (7, 'S_noc', s['S_noc']), (9, 'S_oo', s['A_oo'])):
        assert abs(row[i] - s[key]) <= n * 2.0 ** -52 * scale, (tag, key, row[i], s[key])
    own = sm.values({'S_occ': row[4], 'N_occ': row[5], 'C_out': row[6], 'S_noc': row[7], 'N_noc': row[8], 'S_oo': row[9], 'N_oo': row[10]})
    assert all(same_value(float(g), w) for g, w in zip(row[:4], own)), (tag, row[:4], own)
    assert row[11] == pred.shape[0]
    return s


# the shapes: one pixel; an odd pixel count (a scalar tail, odd planes); two items; several workgroups with an odd count and batch
# offsets; the KITTI frame (910 workgroups: a lane takes a pixel PAIR); and two KITTI frames, the one shape beyond the
# 1024-workgroup cap, where the stride loop runs
@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 3, 5), (2, 7, 66), (3, 37, 129), (1, 375, 1242), (2, 375, 1242)], ids=lambda s: '%dx%dx%d' % s)
def test_rows_equal_the_model(shape):
    B, H, W = shape
    for k, kind in enumerate(KINDS):
        pred, gt_occ, gt_noc = make_case(100 * k + H, B, H, W, kind)
        row = run(pred, gt_occ, gt_noc)
        s = check_row(row, pred, gt_occ, gt_noc, (shape, kind))
        if kind == 'empty':
            assert row[0] == 0.0 and math.isnan(row[1]) and row[2] == 0.0 and row[3] == 0.0 and s['N_occ'] == 0
        elif kind == 'full':
            assert s['N_occ'] == B * H * W == s['N_noc'] and s['N_oo'] == 0
        elif kind == 'not_subset' and B * H * W > 100:
            w = (gt_occ[..., 2] & 255).astype(np.int64) - (gt_noc[..., 2] & 255)
            assert w.min() < 0 < w.max()                                          # negative weights are really there
        if kind != 'empty' and B * H * W > 100:
            on = np.abs(s['d_occ'].astype(np.float64) / s['thr'] - 1.0) < 1e-5      # (the rounding of pred to fp32: ~1e-6 of thr)
            assert on.sum() > 0.2 * np.count_nonzero(gt_occ[..., 2] & 255)        # the generator does put pixels on the threshold


def test_a_nan_in_the_prediction():
    B, H, W = 2, 7, 66
    pred, gt_occ, gt_noc = make_case(7, B, H, W, 'subset', gap=True)
    clean, _ = sm.score(pred, gt_occ, gt_noc)
    out = clean['d_occ'] > clean['thr']
    b, y, x = [int(v[0]) for v in np.nonzero(out & ((gt_noc[..., 2] & 255) > 0))]      # a masked (occ and noc) outlier pixel
    pred[b, 0, y, x] = np.nan
    row = run(pred, gt_occ, gt_noc)
    assert math.isnan(row[4]) and math.isnan(row[7]) and math.isnan(row[0]) and math.isnan(row[2])
    assert row[6] == clean['C_out'] - 1 and row[5] == clean['N_occ'] and row[8] == clean['N_noc']
    assert row[1] == (clean['C_out'] - 1) / clean['N_occ'] * 100.0


def test_rows_are_reproducible_and_confined():
    from upflow_pytorch_amd import ops
    for shape in ((3, 37, 129), (1, 375, 1242)):
        pred, gt_occ, gt_noc = dev(*make_case(3, *shape, 'not_subset'))
        table = torch.full((5, 12), -7.25, dtype=torch.float64, device=DEV)
        r = ops.kitti_score(pred, gt_occ, gt_noc, out=table[2])
        assert r.data_ptr() == table[2].data_ptr()
        first = table.clone()
        assert bool((first[[0, 1, 3, 4]] == -7.25).all()) and not bool((first[2] == -7.25).any())
        again = ops.kitti_score(pred, gt_occ, gt_noc)
        assert torch.equal(again.view(torch.int64), first[2].view(torch.int64))
        ops.kitti_score(pred, gt_occ, gt_noc, out=table[2])
        assert torch.equal(table.view(torch.int64), first.view(torch.int64))


def decode_dev(gt):
    """uint16 [B,H,W,3] on the device -> (flow fp32 [B,2,H,W], mask fp32 [B,1,H,W]), torch spelling of the host decode."""
    flow = ((gt[..., :2].to(torch.int32) - 32768).to(torch.float32) * 0.015625).permute(0, 3, 1, 2).contiguous()
    return flow, (gt[..., 2].to(torch.int32) & 255).to(torch.float32).unsqueeze(1)


def test_against_the_torch_spelling_on_the_gpu():
    """Evaluation_bench.flow_error_avg / outlier_pct on device tensors decoded from the same arrays.  Condition (asserted): no masked
    pixel lies within 1e-5 relative of its threshold, so a 1-ulp difference in a square root cannot move the count."""
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow
    E = kitti_flow.Evaluation_bench
    B, H, W = 2, 37, 129
    n = B * H * W
    pred, gt_occ, gt_noc = make_case(5, B, H, W, 'subset', gap=True)
    flow, m = sm.decode(gt_occ)
    f64 = np.float64
    e = np.sqrt((flow[..., 0].astype(f64) - pred[:, 0]) ** 2 + (flow[..., 1].astype(f64) - pred[:, 1]) ** 2) * m
    thr = np.maximum(3.0, np.sqrt(flow[..., 0].astype(f64) ** 2 + flow[..., 1].astype(f64) ** 2) * f64(np.float32(0.05)))
    assert np.all(np.abs(e - thr)[m > 0] > 1e-5 * thr[m > 0])
    row = run(pred, gt_occ, gt_noc)
    p, o, c = dev(pred, gt_occ, gt_noc)
    (occ, occmask), (noc, nocmask) = decode_dev(o), decode_dev(c)
    want = [float(v) for v in (E.flow_error_avg(occ, p, occmask), E.outlier_pct(occ, p, occmask), E.flow_error_avg(noc, p, nocmask),
                               E.flow_error_avg(occ, p, occmask - nocmask))]
    print('device row', row[:4], 'torch spelling', want)
    assert round(want[1] * row[5] / 100.0) == row[6] and 0 < row[6] < row[5]
    for i in (0, 2, 3):
        assert abs(row[i] - want[i]) <= n * 2.0 ** -24 * abs(want[i]), (i, row[i], want[i])


def test_arguments_are_checked():
    from upflow_pytorch_amd import ops
    pred, gt_occ, gt_noc = dev(*make_case(1, 2, 6, 10, 'subset'))
    bad = [
        lambda: ops.kitti_score(pred.cpu(), gt_occ, gt_noc),                                        # a CPU tensor
        lambda: ops.kitti_score(pred, gt_occ.cpu(), gt_noc),
        lambda: ops.kitti_score(pred.half(), gt_occ, gt_noc),                                       # an fp16 prediction
        lambda: ops.kitti_score(pred, gt_occ.view(torch.int16), gt_noc),                            # int16 ground truth
        lambda: ops.kitti_score(pred, gt_occ, torch.zeros(2, 6, 10, 4, dtype=torch.uint16, device=DEV)),   # [B,H,W,4]
        lambda: ops.kitti_score(pred.transpose(2, 3), gt_occ.transpose(1, 2), gt_noc.transpose(1, 2)),   # transposed
        lambda: ops.kitti_score(pred.transpose(2, 3).contiguous().transpose(2, 3), gt_occ, gt_noc),
        lambda: ops.kitti_score(pred, gt_occ[:1], gt_noc),                                          # another batch
        lambda: ops.kitti_score(pred[:, :1], gt_occ, gt_noc),                                       # one channel
        lambda: ops.kitti_score(pred, gt_occ, gt_noc, out=torch.empty(12, device=DEV)),             # an fp32 row
        lambda: ops.kitti_score(pred, gt_occ, gt_noc, out=torch.empty(2, 12, dtype=torch.float64, device=DEV)),
        lambda: ops.kitti_score(pred, gt_occ, gt_noc, out=torch.empty(12, dtype=torch.float64)),
    ]
    for f in bad:
        with pytest.raises(RuntimeError):
            f()
    assert ops.kitti_score(pred, gt_occ, gt_noc).shape == (12,)                                     # (the operands themselves are fine)


# ---- the evaluation loop ---------------------------------------------------------------------------------------------------------
NAME = re.compile(r'^all_(\S+) f1_(\S+) noc_(\S+) occ_(\S+)__(\d+)$')


def six_tuple(item):
    """(im1, im2, gt_occ u16, gt_noc u16) -> the default item (im1, im2, occ, occmask, noc, nocmask) as the host path decodes it."""
    im1, im2, gt_occ, gt_noc = item
    out = [im1, im2]
    for gt in (gt_occ, gt_noc):
        f, m = sm.decode(gt.numpy())
        out += [torch.from_numpy(np.ascontiguousarray(np.transpose(f, [2, 0, 1]))), torch.from_numpy(m[None].copy())]
    return tuple(out)


def close(got, want, n):
    return all(abs(g - w) <= n * 2.0 ** -24 * abs(w) for g, w in zip(got, want))


def test_evaluation_bench_device_score_with_a_fake_model():
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow
    from upflow_pytorch_amd.utils.tools import tools
    g = torch.Generator().manual_seed(3)
    ds = []
    for i, (H, W) in enumerate(((32, 64), (40, 72), (32, 64), (32, 64), (40, 72))):
        _, gt_occ, gt_noc = make_case(40 + i, 1, H, W, 'subset', reach=80)
        # the model's error is exactly 4 px: keep |gt| away from 80 px, where 5 % of it is 4 (a pixel ON its threshold belongs to
        # the exact tests above, not to a comparison with the torch spelling)
        flow, _ = sm.decode(gt_occ)
        near = np.abs(np.hypot(flow[..., 0].astype(np.float64), flow[..., 1]) - 80.0) < 1.0
        gt_occ[..., :2][near] = 32768
        gt_occ[..., 2] &= 255                   # (weights 0, 1, 2; the wrap of 256 / 257 is the exact tests' business)
        gt_noc[..., 2] &= 255
        ds.append((torch.randn(3, H, W, generator=g), torch.randn(3, H, W, generator=g), torch.from_numpy(gt_occ[0]), torch.from_numpy(gt_noc[0])))

    class Model(tools.abs_test_model):
        def __init__(self):
            super(Model, self).__init__()
            self.saved = []

        def eval_forward(self, im1, im2, gt, *args):
            flow = decode_dev(gt)[0] if gt.dtype == torch.uint16 else gt
            assert flow.is_cuda
            return flow + torch.tensor([4.0, 0.0], device=flow.device).view(1, 2, 1, 1)

        def eval_save_result(self, save_name, predflow, *args, **kwargs):
            self.saved.append((save_name, predflow, kwargs['occmask']))

    old = Model()
    want = kitti_flow.Evaluation_bench('2015_train', batch_size=1, dataset=[six_tuple(it) for it in ds])(old)
    results = []
    for lag in (1, 100, 8):
        new = Model()
        kw = {} if lag == 8 else {'save_lag': lag}
        got = kitti_flow.Evaluation_bench('2015_train', batch_size=1, dataset=ds, device_score=True, **kw)(new)
        print('lag', lag, got, want)
        assert close(got, want, 40 * 72) and 0.0 < got[1] < 100.0
        assert len(new.saved) == 5
        for i, ((name, predflow, occmask), (old_name, old_pred, old_mask)) in enumerate(zip(new.saved, old.saved)):
            a, b = NAME.match(name), NAME.match(old_name)
            assert a and b and int(a.group(5)) == i == int(b.group(5)), (name, old_name)
            assert all(abs(float(a.group(k)) - float(b.group(k))) <= 0.006 for k in (1, 2, 3, 4)), (name, old_name)
            assert occmask.dtype == torch.float32 and tuple(occmask.shape) == (1, 1) + tuple(ds[i][2].shape[:2])
            assert torch.equal(occmask.cpu(), six_tuple(ds[i])[3][None]) and torch.equal(occmask, old_mask)
            assert torch.equal(predflow, old_pred)
        results.append((got, [s[0] for s in new.saved]))
    assert results[0] == results[1] == results[2]


def test_evaluation_bench_device_score_with_the_network():
    """Six synthetic uint8 pairs of two sizes through Test_model(streams=4): the pipelined and the sequential loop give the same
    bits with device_score=True, and the existing path's numbers within its fp32 summation bound."""
    from upflow_pytorch_amd.test import Test_model
    from upflow_pytorch_amd.dataset.kitti_dataset import kitti_flow, img_func
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    conf = UPFlow_net.config()
    conf.update({'if_norm_before_cost_volume': True, 'norm_moments_across_channels': False, 'norm_moments_across_images': False,
                 'if_sgu_upsample': True, 'warp_mask_mode': 'robust'}, verbose=False)
    net = conf()
    net.load_state_dict(_weights.make_state_dict(0, head_scale=0.1))
    net = net.cuda().to(torch.bfloat16).eval()
    tm = Test_model(pretrain_path=None, dtype=torch.bfloat16, net=net, streams=4)
    q = lambda im: ((im + 0.45) * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # noqa: E731
    ds, ds6 = [], []
    for i, (H, W) in enumerate(((64, 128), (72, 136), (64, 128), (72, 136), (64, 128), (64, 128))):
        a, b = (q(t) for t in _weights.make_smooth_images(200 + i, 1, H, W))
        with torch.no_grad():
            flow = net({'frames1_u8': a.cuda(), 'frames2_u8': b.cuda(), 'if_loss': False})['flow_f_out'][0].float().cpu().numpy()
        valid = (np.random.default_rng(i).random((H, W)) > 0.2).astype(np.uint16)
        gt_occ = sm.encode(np.transpose(flow, [1, 2, 0]) + 0.5, valid)
        gt_noc = sm.encode(np.transpose(flow, [1, 2, 0]) + 0.5, valid * (np.random.default_rng(50 + i).random((H, W)) > 0.3))
        item = (a[0], b[0], torch.from_numpy(gt_occ), torch.from_numpy(gt_noc))
        ds.append(item)
        f32 = [img_func.np_2_tensor(img_func.get_process_img_only_img(t.numpy()))[0] for t in item[:2]]
        ds6.append(six_tuple((f32[0], f32[1], item[2], item[3])))
    seq_model = Test_model(pretrain_path=None, dtype=torch.bfloat16, net=net)
    par = kitti_flow.Evaluation_bench('2015_train', batch_size=1, dataset=ds, device_score=True)(tm)
    seq = kitti_flow.Evaluation_bench('2015_train', batch_size=1, dataset=ds, device_score=True)(seq_model)
    old = kitti_flow.Evaluation_bench('2015_train', batch_size=1, dataset=ds6)(seq_model)
    print('pipelined', par, 'sequential', seq, 'existing path', old)
    assert par == seq
    assert close(par, old, 72 * 136) and par[1] == 0.0 == old[1]
    assert abs(par[0] - 0.5 * 2 ** 0.5) < 2e-2 and par[3] > 0.0              # the offset, to the 1/64 grid of the format
