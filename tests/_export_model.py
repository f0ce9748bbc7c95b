"""Numpy model of upf_flow_export (include/upflow_hip.h), written from the formulas: the exact yardstick of the
kernel's `kitti` and `flo` outputs and — up to the last bit of atan2 — of `rgb`.  Also the frames of the golden fixtures
(tests/golden/make_golden_export.py records what the reference's flow_to_image and the host writer's encode give for them), so
that the fixtures hold results only and the inputs are regenerated from integers.

Frames are float32 [H,W,2]; batches [B,2,H,W] as the network returns them."""
import numpy as np

EPS = 2.0 ** -52


def wheel():
    """The 55-entry Middlebury wheel, integer [55,3]."""
    w = np.zeros((55, 3), dtype=np.int64)
    i = lambda n: (255 * np.arange(n)) // n                           # noqa: E731  floor(255 * i / n)
    w[0:15, 0], w[0:15, 1] = 255, i(15)                               # red -> yellow
    w[15:21, 0], w[15:21, 1] = 255 - i(6), 255                        # yellow -> green
    w[21:25, 1], w[21:25, 2] = 255, i(4)                              # green -> cyan
    w[25:36, 1], w[25:36, 2] = 255 - i(11), 255                       # cyan -> blue
    w[36:49, 2], w[36:49, 0] = 255, i(13)                             # blue -> magenta
    w[49:55, 2], w[49:55, 0] = 255 - i(6), 255                        # magenta -> red
    return w


WHEEL = wheel()


def black(u, v):
    """unknown (|u| or |v| > 1e7, in fp32) or NaN: rendered black, (0,0) for the maximum"""
    with np.errstate(invalid='ignore'):
        return (np.abs(u) > np.float32(1e7)) | (np.abs(v) > np.float32(1e7)) | np.isnan(u) | np.isnan(v)


def maxrad(frame):
    """fp32 maximum of sqrt(u*u + v*v), every step a correctly rounded fp32 operation (numpy's float32 ufuncs are)"""
    u, v = frame[..., 0].astype(np.float32), frame[..., 1].astype(np.float32)
    b = black(u, v)
    u, v = np.where(b, np.float32(0), u), np.where(b, np.float32(0), v)
    r = np.sqrt(u * u + v * v)
    assert r.dtype == np.float32
    return r.max()


def scaled(frame, max_rad=None):
    """-> (u, v, rad float64 after the division, black mask)"""
    u, v = frame[..., 0].astype(np.float32), frame[..., 1].astype(np.float32)
    b = black(u, v)
    m = np.float32(max_rad) if max_rad is not None and max_rad > 0 else maxrad(frame)
    d = np.float64(m) + EPS
    u, v = np.where(b, 0.0, u.astype(np.float64)) / d, np.where(b, 0.0, v.astype(np.float64)) / d
    return u, v, np.sqrt(u * u + v * v), b


def rgb(frame, max_rad=None, angle_ulps=0):
    """frame float32 [H,W,2] -> uint8 [H,W,3].  angle_ulps: move atan2's result by that many ulps (the sensitivity of the result
    to the one inexact operation)."""
    u, v, rad, b = scaled(frame, max_rad)
    ang = np.arctan2(-v, -u)
    for _ in range(abs(angle_ulps)):
        ang = np.nextafter(ang, np.inf if angle_ulps > 0 else -np.inf)
    fk = (ang / np.pi + 1.0) / 2.0 * 54.0 + 1.0
    k0 = np.clip(np.floor(fk).astype(np.int64), 1, 55)
    k1 = np.where(k0 == 55, 1, k0 + 1)
    f = fk - np.floor(fk)
    out = np.zeros(frame.shape[:-1] + (3,), dtype=np.uint8)
    for c in range(3):
        col = (1.0 - f) * (WHEEL[k0 - 1, c] / 255.0) + f * (WHEEL[k1 - 1, c] / 255.0)
        col = np.where(rad <= 1.0, 1.0 - rad * (1.0 - col), col * 0.75)
        out[..., c] = np.where(b, 0, np.floor(255.0 * col)).astype(np.uint8)
    return out


def kitti(frame, valid=None):
    """frame float32 [H,W,2], valid [H,W] or None -> uint16 [H,W,3]; a NaN component: (0,0,0)"""
    frame = frame.astype(np.float32)
    nan = np.isnan(frame).any(axis=-1)
    with np.errstate(invalid='ignore'):
        enc = np.clip(np.where(np.isnan(frame), 0.0, frame.astype(np.float64)) * 64.0 + 32768.0, 0.0, 65535.0).astype(np.uint16)
    third = np.ones(frame.shape[:-1], dtype=np.uint16) if valid is None else np.asarray(valid).astype(np.uint16)
    out = np.concatenate([enc, third[..., None]], axis=-1)
    out[nan] = 0
    return out


def flo(frame):
    return np.ascontiguousarray(frame.astype(np.float32))


def export(pred, valid=None, max_rad=None):
    """pred float32 [B,2,H,W], valid [B,1,H,W] or None -> dict of 'kitti' uint16 [B,H,W,3], 'color' uint8 [B,H,W,3],
    'flo' float32 [B,H,W,2]; the colour scale is per item"""
    frames = np.ascontiguousarray(np.transpose(pred, [0, 2, 3, 1]))
    return {'kitti': np.stack([kitti(f, None if valid is None else valid[i, 0]) for i, f in enumerate(frames)]),
            'color': np.stack([rgb(f, max_rad) for f in frames]),
            'flo': frames.copy()}


def top_pixel_rad(frame):
    """float64 rad of the frame's largest pixel (the one whose fp32 radius is the maximum): > 1 for about a frame in three"""
    _, _, rad, _ = scaled(frame)
    return rad.max()


# ---- the frames of the fixtures --------------------------------------------------------------------------------------------------
def motion(seed, H, W, scale, block=4):
    """Flow constant over block x block cells (ragged at the edges), components scale * k / 2^20 with k a seeded integer in
    [-2^20, 2^20]: built from integers, so the same bits wherever it is generated; cells keep the fixtures small."""
    g = np.random.default_rng(seed)
    k = g.integers(-2 ** 20, 2 ** 20 + 1, size=((H + block - 1) // block, (W + block - 1) // block, 2))
    cells = (k.astype(np.float64) * (scale / 2.0 ** 20)).astype(np.float32)
    return np.ascontiguousarray(np.repeat(np.repeat(cells, block, axis=0), block, axis=1)[:H, :W])


SIZES = ((9, 70), (33, 130), (64, 257))
SCALES = (0.3, 3.0, 40.0)


def _find_radgt1(n, start=1000):
    """the first n seeds from `start` of 9x70 frames whose largest pixel has float64 rad > 1 (a deterministic search)"""
    seeds, s = [], start
    while len(seeds) < n:
        if top_pixel_rad(motion(s, 9, 70, 3.0)) > 1.0:
            seeds.append(s)
        s += 1
    return tuple(seeds)


def golden_frames():
    """name -> float32 [H,W,2], in a fixed order"""
    frames = {}
    for i, (H, W) in enumerate(SIZES):
        for j, s in enumerate(SCALES):
            frames['motion_%dx%d_%g' % (H, W, s)] = motion(10 * i + j, H, W, s)
    frames['zero'] = np.zeros((9, 70, 2), dtype=np.float32)
    r = np.float32(1.0)
    frames['axes8'] = np.array([[[r, 0], [r, r], [0, r], [-r, r], [-r, 0], [-r, -r], [0, -r], [r, -r]]], dtype=np.float32)
    frames['axes4'] = np.array([[[r, 0], [0, r], [-r, 0], [0, -r]]], dtype=np.float32)
    unk = motion(77, 9, 70, 3.0)
    unk[0, 0, 0] = np.nextafter(np.float32(1e7), np.float32(np.inf))
    unk[1, 5, 1] = -1e8
    unk[2, 9, 0] = np.inf
    unk[3, 13, 1] = -np.inf
    unk[8, 69] = (np.inf, -np.inf)
    frames['unknown'] = unk
    for s in _find_radgt1(3):
        frames['radgt1_%d' % s] = motion(s, 9, 70, 3.0)
    return frames
