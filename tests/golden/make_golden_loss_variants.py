#!/usr/bin/env python3
"""Generate tests/golden/lossvar_*.npz by IMPORTING the reference (like make_golden.py: build container only).

The reference's own network_tools.edge_aware_smoothness_order2 / flow_smooth_delta / photo_loss_multi_type ('charbonnier', 'L1',
'SSIM') / weighted_ssim run on the CPU in fp32 and in fp64 on the same seeded inputs, with autograd; inputs, values and
gradients are stored (data only).

Usage:  python tests/golden/make_golden_loss_variants.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _lossvar as lv  # noqa: E402
from make_golden import import_reference, save  # noqa: E402


def run(fn, inputs, diff, dtype):
    """fn(*inputs in dtype) -> scalar; -> (value, [gradient of each input named in diff])."""
    xs = [None if t is None else t.to(dtype).clone().requires_grad_(i in diff) for i, t in enumerate(inputs)]
    v = fn(*xs)
    grads = torch.autograd.grad(v, [xs[i] for i in diff])
    return v.detach(), [g.detach() for g in grads]


def both(out, key, fn, inputs, diff, names):
    for tag, dtype in (('32', torch.float32), ('64', torch.float64)):
        v, gs = run(fn, inputs, diff, dtype)
        out['%s_val%s' % (key, tag)] = v
        for n, g in zip(names, gs):
            out['%s_g%s%s' % (key, n, tag)] = g


def main():
    upflow = import_reference()[0]
    nt = upflow.network_tools
    for i, shape in enumerate(lv.FIXTURE_SHAPES):
        B, C, H, W = shape
        # A: second-order edge-aware smoothness
        img, pred = lv.textured(shape, 10 + i), lv.flow_inputs((B, 2 if C > 1 else 1, H, W), 20 + i)
        out = {'img': img, 'pred': pred}
        both(out, 'edge2', lambda a, b: nt.edge_aware_smoothness_order2(a, b), [img, pred], [1], ['pred'])
        save('lossvar_edge2_%d' % i, **out)
        # B: delta smoothness, both orders, on a random and on a piecewise-constant flow
        flow, pc = lv.flow_inputs((B, 2 if C > 1 else 1, H, W), 30 + i), lv.piecewise_constant((B, 2 if C > 1 else 1, H, W), 40 + i)
        out = {'flow': flow, 'pc': pc}
        for name, f in (('flow', flow), ('pc', pc)):
            for order in (1, 2):
                both(out, '%s_o%d' % (name, order), lambda a, o=order: nt.flow_smooth_delta(a, o == 2), [f], [0], ['flow'])
        save('lossvar_delta_%d' % i, **out)
        # C: point-wise photometric kinds
        x, y = lv.textured(shape, 50 + i), lv.textured(shape, 60 + i)
        occs = {'none': None, 'binary': lv.binary_mask(shape, 70 + i), 'zero': torch.zeros(B, 1, H, W)}
        out = {'x': x, 'y': y, 'occ_binary': occs['binary']}
        for kind in ('charbonnier', 'L1'):
            for oname, occ in occs.items():
                def fn(a, b, kind=kind, occ=occ):
                    o = torch.ones(B, 1, H, W, dtype=a.dtype) if occ is None else occ.to(a.dtype)
                    return nt.photo_loss_multi_type(a, b, o, photo_loss_type=kind, photo_loss_delta=0.4, photo_loss_use_occ=occ is not None)
                both(out, '%s_%s' % (kind, oname), fn, [x, y], [0, 1], ['x', 'y'])
        save('lossvar_pointwise_%d' % i, **out)
        # D: weighted SSIM — the map under a random upstream gradient G, and the two photometric forms
        x, y, w = lv.ssim_inputs(shape, 80 + i)
        G = torch.randn(B, C, H - 2, W - 2, generator=lv.gen(90 + i))
        out = {'x': x, 'y': y, 'weight': w, 'G': G}
        for tag, dtype in (('32', torch.float32), ('64', torch.float64)):
            m, wa = nt.weighted_ssim(x.to(dtype), y.to(dtype), w.to(dtype))
            out['map%s' % tag], out['wavg%s' % tag] = m, wa
        both(out, 'map', lambda a, b: (nt.weighted_ssim(a, b, w.to(a.dtype))[0] * G.to(a.dtype)).sum(), [x, y], [0, 1], ['x', 'y'])
        for use_occ in (True, False):
            both(out, 'photo_occ%d' % use_occ,
                 lambda a, b, u=use_occ: nt.photo_loss_multi_type(a, b, w.to(a.dtype), photo_loss_type='SSIM', photo_loss_use_occ=u),
                 [x, y], [0, 1], ['x', 'y'])
        save('lossvar_ssim_%d' % i, **out)


if __name__ == '__main__':
    main()
