#!/usr/bin/env python3
"""Generate tests/golden/errmap.npz by IMPORTING the reference (as make_golden_export.py does; build container only).

The fixture records one 24 x 40 pair — seeded inputs, built here — and what the reference's
tools.lib_to_show_flow.flow_error_image_np (utils/tools.py:702-758) returns for it:
    pred      fp32   [1,2,H,W]    the prediction
    gt_occ    uint16 [1,H,W,3]    the payload of the flow_occ PNG (R = u*64 + 2^15, G = v*64 + 2^15, B = valid)
    gt_noc    uint16 [1,H,W,3]    the payload of the flow_noc PNG
    ref_log   float64 [H,W,3]     the reference's image, log_colors=True  (B, G, R as it returns it)
    ref_lin   float64 [H,W,3]     the reference's image, log_colors=False
    table_full, table_half  uint8 [10,3]   rint(255 * image) R, G, B of one probe pixel per bin, not occluded / occluded
The reference gets float32 flows (the decoded ground truth is exact in fp32) and float64 masks [H,W,1], so that its non-log image is
the float64 product and 255 * image is evaluated in float64, as the contract of upf_flow_error_image states it.

The inputs hold (asserted below, on tests/_errmap_model.py's fp32 arithmetic):
    row 0      ground truth 0, pred = (3 * bound, 0) for the nine inner bounds: diff / 3 is the bound itself -> the upper bin
    row 1      the fp32 number below 3 * bound: diff / 3 rounds to the fp32 number below the bound -> the lower bin
    row 2      |gt| = 80 > 60: 20 * diff / |gt| is the smaller term; errors across the bins
    row 3      pred 4e9, +inf, -inf, NaN (u, v, both): black in the log map; 2.9999e9: the last bin; each not occluded and occluded
    row 4      the four (m_occ, m_noc) pairs of {0,1}^2 on identical flows, "noc but not occ" among them
    the rest   seeded: ground truth on the 1/64 grid, errors log-uniform in 0.01 .. 60 px, the four mask pairs

Usage:  python tests/golden/make_golden_errmap.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _errmap_model as M  # noqa: E402
import _score_model as S  # noqa: E402

f32 = np.float32
H, W = 24, 40
INNER = [0.0625, 0.125, 0.25, 0.5, 1, 2, 4, 8, 16]


def inputs():
    rng = np.random.RandomState(20150702)
    gt = np.round(rng.uniform(-90, 90, (H, W, 2)) * 64) / 64
    ang = rng.uniform(0, 2 * np.pi, (H, W))
    mag = np.exp(rng.uniform(np.log(0.01), np.log(60.0), (H, W)))
    pred = (gt + np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)).astype(f32)
    pair = rng.randint(0, 4, (H, W))
    m_occ, m_noc = (pair >> 1) & 1, pair & 1
    gt[0:2], m_occ[0:2], m_noc[0:2] = 0, 1, 1
    pred[0:2] = 0
    for k, b in enumerate(INNER):
        for j in range(4):                                                         # four copies: the tail of the row is used too
            if k + 9 * j < W:
                pred[0, k + 9 * j, 0] = f32(3 * b)
                pred[1, k + 9 * j, 0] = np.nextafter(f32(3 * b), f32(0))
    gt[2], m_occ[2] = (80.0, 0.0), 1
    m_noc[2] = np.arange(W) % 2
    pred[2, :, 0] = (80.0 + np.exp(np.linspace(np.log(0.05), np.log(120.0), W))).astype(f32)
    pred[2, :, 1] = 0
    gt[3], m_occ[3] = 0, 1
    pred[3] = 0
    special = [4e9, np.inf, -np.inf, np.nan, 2.9999e9]
    for k, v in enumerate(special):
        for j in range(2):
            pred[3, 2 * k + j, 0] = v
            m_noc[3, 2 * k + j] = 1 - j
    pred[3, 10:12, 1] = np.nan                                                     # a NaN in v alone
    pred[3, 12:14] = np.nan                                                        # and in both
    m_noc[3, 10:14] = [1, 0, 1, 0]
    gt[4], pred[4] = (12.5, -3.25), (14.0, -2.0)
    m_occ[4], m_noc[4] = (np.arange(W) >> 1) & 1, np.arange(W) & 1
    gt_occ = S.encode(gt, m_occ)[None]
    gt_noc = S.encode(gt, m_noc)[None]                                             # (the same flow: only its B channel is read)
    return np.ascontiguousarray(pred.transpose(2, 0, 1)[None]), gt_occ, gt_noc


def check_inputs(pred, gt_occ, gt_noc):
    flow, m_occ = S.decode(gt_occ)
    _, m_noc = S.decode(gt_noc)
    diff, mag = M.error(pred[:, 0], pred[:, 1], flow[..., 0], flow[..., 1])
    third, rel = M.div32(diff, f32(3.0)), M.div32(S.mul32(np.full_like(diff, 20.0), diff), S.add32(mag, np.full_like(mag, 1e-7)))
    for k, b in enumerate(INNER):
        assert third[0, 0, k] == f32(b) and third[0, 1, k] == np.nextafter(f32(b), f32(0)), (b, third[0, 0, k], third[0, 1, k])
        assert rel[0, 0, k] > third[0, 0, k] and rel[0, 1, k] > third[0, 1, k]
    assert mag[0, 2].min() > 60 and np.all(rel[0, 2] < third[0, 2])
    assert set(zip(m_occ.ravel().astype(int), m_noc.ravel().astype(int))) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert set(zip(m_occ[0, 4].astype(int), m_noc[0, 4].astype(int))) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    rgb, _ = M.render(pred, gt_occ, gt_noc, True)
    assert not rgb[0, 3, 0:8].any() and not rgb[0, 3, 10:14].any()                 # 4e9, +-inf, NaN: black
    assert tuple(rgb[0, 3, 8]) == tuple(M.FULL[9]) and tuple(rgb[0, 3, 9]) == tuple(M.HALF[9])   # 2.9999e9: the last bin


def reference_images(ref_fn, pred, gt_occ, gt_noc):
    flow, m_occ = S.decode(gt_occ[0])
    _, m_noc = S.decode(gt_noc[0])
    args = (np.ascontiguousarray(pred[0].transpose(1, 2, 0)), flow, m_occ.astype(np.float64)[..., None], m_noc.astype(np.float64)[..., None])
    with np.errstate(all='ignore'):
        return [np.ascontiguousarray(ref_fn(*args, log_colors=lc), dtype=np.float64) for lc in (True, False)]


def reference_tables(ref_fn):
    """one probe pixel per bin (diff / 3 = the bin's lower bound, ground truth 0), not occluded and occluded"""
    lo = np.array([0] + INNER, dtype=f32)
    pred = np.zeros((2, 10, 2), dtype=f32)
    pred[:, :, 0] = 3 * lo
    noc = np.stack([np.ones(10), np.zeros(10)])[..., None]
    with np.errstate(all='ignore'):
        im = ref_fn(pred, np.zeros_like(pred), np.ones((2, 10, 1)), noc, log_colors=True)
    t = np.rint(255 * im[:, :, ::-1])
    assert t.min() >= 0 and t.max() <= 255
    return t[0].astype(np.uint8), t[1].astype(np.uint8)


def main():
    pred, gt_occ, gt_noc = inputs()
    check_inputs(pred, gt_occ, gt_noc)
    from make_golden import REF, import_reference
    if not os.path.isdir(REF):
        raise SystemExit('the reference is not present at %s: tests/golden/errmap.npz is left as it is' % REF)
    _, _, ref_tools, _ = import_reference()
    ref_fn = ref_tools.lib_to_show_flow.flow_error_image_np
    ref_log, ref_lin = reference_images(ref_fn, pred, gt_occ, gt_noc)
    full, half = reference_tables(ref_fn)
    assert np.array_equal(full, M.FULL) and np.array_equal(half, M.HALF) and np.array_equal(half, (full.astype(int) + 1) // 2)
    for lc, ref in ((True, ref_log), (False, ref_lin)):                            # the fixture's own confirmation of the model
        want = np.rint(255 * ref[:, :, ::-1])
        want = np.where(np.isnan(want), 0, want).astype(np.uint8)
        got = M.render(pred, gt_occ, gt_noc, lc)[0][0]
        print('log_colors=%-5s pixels where the model differs from rint(255 * reference): %d of %d' % (lc, int(np.any(got != want, -1).sum()), H * W))
    path = os.path.join(HERE, 'errmap.npz')
    np.savez_compressed(path, pred=pred, gt_occ=gt_occ, gt_noc=gt_noc, ref_log=ref_log, ref_lin=ref_lin, table_full=full, table_half=half)
    print('errmap.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
