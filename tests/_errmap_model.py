"""The numpy model of upf_flow_error_image (include/upflow_hip.h): every per-pixel step an explicit, correctly rounded fp32
operation (the square root and the decode are tests/_score_model.py's; numpy's fp32 divide is the IEEE division), the bins and the
two colour tables as the contract lists them, and `dilate` as a literal painting: every valid pixel, in raster order, paints its
colour over the invalid pixels of its window, so that the last painter — the valid pixel with the greatest y', then x' — stays.
The exact yardstick of the kernel; written from the contract and not from the kernel."""
import numpy as np

import _score_model as S

f32 = np.float32
LO = np.array([0, 0.0625, 0.125, 0.25, 0.5, 1, 2, 4, 8, 16, 1e9], dtype=f32)
FULL = np.array([[49, 54, 149], [69, 117, 180], [116, 173, 209], [171, 217, 233], [224, 243, 248],
                 [254, 224, 144], [253, 174, 97], [244, 109, 67], [215, 48, 39], [165, 0, 38]], dtype=np.uint8)
HALF = np.array([[25, 27, 75], [35, 59, 90], [58, 87, 105], [86, 109, 117], [112, 122, 124],
                 [127, 112, 72], [127, 87, 49], [122, 55, 34], [108, 24, 20], [83, 0, 19]], dtype=np.uint8)


def div32(a, b):
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        return (np.asarray(a, dtype=f32) / np.asarray(b, dtype=f32)).astype(f32)


def error(pu, pv, gu, gv):
    """(diff, mag) in fp32"""
    with np.errstate(invalid='ignore', over='ignore'):
        du, dv = S.sub32(pu, gu), S.sub32(pv, gv)
        diff = S.sqrt32(S.add32(S.mul32(du, du), S.mul32(dv, dv)))
        mag = S.sqrt32(S.add32(S.mul32(gu, gu), S.mul32(gv, gv)))
    return diff, mag


def render(pred, gt_occ, gt_noc, log_colors=True):
    """pred fp32 [B,2,H,W], gt_occ / gt_noc uint16 [B,H,W,3] -> (rgb uint8 [B,H,W,3], valid bool [B,H,W]): the plain map"""
    pred = np.asarray(pred)
    assert pred.dtype == f32 and pred.ndim == 4 and pred.shape[1] == 2
    flow, m_occ = S.decode(gt_occ)
    _, m_noc = S.decode(gt_noc)
    valid, noc = m_occ != 0, m_noc == 1
    diff, mag = error(pred[:, 0], pred[:, 1], flow[..., 0], flow[..., 1])
    rgb = np.zeros(pred.shape[:1] + pred.shape[2:] + (3,), dtype=np.uint8)
    with np.errstate(invalid='ignore', over='ignore'):
        if log_colors:
            err = np.minimum(div32(diff, f32(3.0)), div32(S.mul32(f32(20.0) * np.ones_like(diff), diff), S.add32(mag, f32(1e-7) * np.ones_like(mag))))
            for i in range(10):                                            # (disjoint bins: at most one matches)
                hit = (err >= LO[i]) & (err < LO[i + 1])
                rgb[hit & noc] = FULL[i]
                rgb[hit & ~noc] = HALF[i]
        else:
            e = div32(np.minimum(diff, f32(5.0)), f32(5.0))
            b = np.rint(e.astype(np.float64) * 255.0)
            b = np.where(np.isnan(b), 0.0, b).astype(np.uint8)
            rgb[..., 0] = b
            rgb[..., 1] = np.where(noc, b, 0)
            rgb[..., 2] = np.where(noc, b, 0)
    rgb[~valid] = 0
    return rgb, valid


def dilate(rgb, valid, r):
    """the literal painting of one batch: rgb uint8 [B,H,W,3], valid bool [B,H,W] -> uint8 [B,H,W,3]"""
    if r == 0:
        return rgb.copy()
    B, H, W, _ = rgb.shape
    out = np.zeros_like(rgb)
    for b in range(B):
        for y, x in zip(*np.nonzero(valid[b])):                             # raster order: later painters overwrite
            out[b, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = rgb[b, y, x]
        out[b][valid[b]] = rgb[b][valid[b]]                                 # a valid pixel keeps its own colour
    return out


def flow_error_image(pred, gt_occ, gt_noc, log_colors=True, dilate_r=0):
    rgb, valid = render(pred, gt_occ, gt_noc, log_colors)
    return dilate(rgb, valid, dilate_r)
