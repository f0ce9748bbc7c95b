"""The numpy model of upf_kitti_score (include/upflow_hip.h): every per-pixel step an explicit, correctly rounded fp32 operation,
the square root taken as float32(sqrt(float64(s))) — correctly rounded, since a 53-bit root rounds to 24 bits without a double
rounding error — and the sums in float64 / exact integers.  The exact yardstick of the kernel; never torch's CPU spelling, whose
vectorised fp32 sqrt is off by one ulp on a fraction of a percent of its inputs."""
import numpy as np

f32 = np.float32
REL = f32(0.05)


def sqrt32(s):
    return np.sqrt(s.astype(np.float64)).astype(f32)


def mul32(a, b):
    return (a.astype(f32) * b.astype(f32)).astype(f32)


def add32(a, b):
    return (a.astype(f32) + b.astype(f32)).astype(f32)


def sub32(a, b):
    return (a.astype(f32) - b.astype(f32)).astype(f32)


def decode(gt_u16):
    """uint16 [...,3] -> (flow fp32 [...,2], weight fp32 [...]): the host path's float64 decode rounded to fp32 (exact either
    way), and its np.uint8() of the valid channel."""
    g = np.asarray(gt_u16)
    assert g.dtype == np.uint16 and g.shape[-1] == 3
    flow = mul32((g[..., 0:2].astype(np.int32) - 32768).astype(f32), f32(0.015625))
    return flow, (g[..., 2] & 255).astype(f32)


def epe(gu, gv, pu, pv):
    du, dv = sub32(gu, pu), sub32(gv, pv)
    return sqrt32(add32(mul32(du, du), mul32(dv, dv)))


def threshold(gu, gv):
    return np.maximum(f32(3.0), mul32(sqrt32(add32(mul32(gu, gu), mul32(gv, gv))), REL))


def core(gu_o, gv_o, m_occ, gu_n, gv_n, m_noc, pu, pv):
    """The seven sums from decoded fp32 arrays of one shape (any): a dict with float64 S_* and Python-int N_* / C_out, plus the
    per-pixel fp32 arrays d_occ and thr (for a test's distance-to-threshold condition)."""
    with np.errstate(invalid='ignore'):
        e_occ = epe(gu_o, gv_o, pu, pv)
        e_noc = epe(gu_n, gv_n, pu, pv)
        thr = threshold(gu_o, gv_o)
        d_occ = mul32(e_occ, m_occ)
        w_oo = sub32(m_occ, m_noc)
        out = d_occ > thr
        t_oo = mul32(e_occ, w_oo)
        return {
            'A_oo': float(np.sum(np.abs(t_oo).astype(np.float64))),         # sum |term| of S_oo: what a bound on its error scales with
            'S_occ': float(np.sum(d_occ.astype(np.float64))), 'N_occ': int(np.sum(m_occ.astype(np.int64))),
            'C_out': int(np.sum(out)),
            'S_noc': float(np.sum(mul32(e_noc, m_noc).astype(np.float64))), 'N_noc': int(np.sum(m_noc.astype(np.int64))),
            'S_oo': float(np.sum(t_oo.astype(np.float64))), 'N_oo': int(np.sum(w_oo.astype(np.int64))),
            'd_occ': d_occ, 'thr': thr,
        }


def values(s):
    """(EPE all, F1 %, EPE noc, EPE occluded-only) of the sums, in float64 as the finishing kernel computes them."""
    with np.errstate(invalid='ignore', divide='ignore'):
        n_occ, n_noc, n_oo, c = (np.float64(s[k]) for k in ('N_occ', 'N_noc', 'N_oo', 'C_out'))
        return (float(np.float64(s['S_occ']) / (n_occ + 1e-6)), float(c / n_occ * 100.0),
                float(np.float64(s['S_noc']) / (n_noc + 1e-6)), float(np.float64(s['S_oo']) / (n_oo + 1e-6)))


def score(pred, gt_occ, gt_noc):
    """pred fp32 [B,2,H,W], gt_occ / gt_noc uint16 [B,H,W,3] -> (sums dict, the row of 12 float64)."""
    pred = np.asarray(pred)
    assert pred.dtype == f32 and pred.ndim == 4 and pred.shape[1] == 2
    fo, mo = decode(gt_occ)
    fn, mn = decode(gt_noc)
    s = core(fo[..., 0], fo[..., 1], mo, fn[..., 0], fn[..., 1], mn, pred[:, 0], pred[:, 1])
    row = np.array(list(values(s)) + [s['S_occ'], s['N_occ'], s['C_out'], s['S_noc'], s['N_noc'], s['S_oo'], s['N_oo'], pred.shape[0]],
                   dtype=np.float64)
    return s, row


def encode(flow, valid):
    """flow fp32 [...,2] on the 1/64 grid within the format's range, valid integer [...] -> uint16 [...,3]."""
    q = np.rint(np.asarray(flow, dtype=np.float64) * 64.0) + 32768.0
    assert q.min() >= 0 and q.max() <= 65535
    return np.concatenate([q.astype(np.uint16), np.asarray(valid).astype(np.uint16)[..., None]], axis=-1)
