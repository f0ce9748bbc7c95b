"""The flow-resize kernels (csrc/sgu_blend.hip: upsample_fwd_kernel with 4 and 1 pixels per thread; the five backward kernels
upsample_bwd_group_kernel<1 / 4 / 16>, upsample_bwd_wg_kernel, upsample_bwd_band_kernel, each with and without its weight tables)
against the resize model of tests/_exact_model.py (lerp32 = make_lerp of csrc/sampling.hpp step by step in fp32; values and the
exact adjoint in fp64).  tests/test_exact_model_cpu.py checks the guards and that every route below has a case.

  dyadic    (in-1)/(out-1) a power of two or 0, data multiples of 1/4 within +-4: every weight, product and partial sum is exact in
            fp32 in any order and any grouping, so all five backward kernels and both forward forms must give the fp64 value,
            (multiplied by fp32(W/w) / fp32(H/h) and) rounded once.  No tolerance.
  general   forward within gamma_4 (+1 with the rate) * sum |terms| of the fp64 evaluation; backward within gamma_n * sum |gy wy wx|,
            n = (non-zero weights of the footprint) + 8 (the deepest reduction tree, 256 -> 1) + 2 (+1 with the rate).

Routes (tests/_exact_model.py upsample_bwd_route, read off launch_upsample_backward): footprint estimate fp = (2 ceil(H/h) + 2) *
(2 ceil(W/w) + 2); band kernel for fp > 200 with w > 1 and W > 1 (column bands of NB inputs; no row table beyond 1024 footprint
rows); else workgroup kernel for fp > 512 (no tables beyond 160 rows or columns); else 16 / 4 / 1 lanes per input pixel for
fp > 200 / > 16 / else (no column table beyond 24 footprint columns)."""
import numpy as np
import pytest
import torch

import _exact_model as em

pytestmark = pytest.mark.gpu

F32 = em.F32
OUTSIDE = 'stored outside the output'


def cid(c):
    return '%dx%d_to_%dx%d' % (c[0] + c[1])


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def stream():
    from upflow_pytorch_amd import _lib
    return _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))


def arena32(nblocks, numel):
    return em.Arena32('cuda', nblocks * (numel + em.Arena.MARGIN + 64) + em.Arena.MARGIN + 64)


def compare(got, ref, bound, what):
    """bound None: the dyadic regime — the fp64 value rounded once, as a value; else |got - ref| <= bound per element."""
    g = got.cpu()
    if bound is None:
        want = em.rne(ref, F32)
        bad = g != want
        assert not bool(bad.any()), '%s: %d of %d elements differ from the exact value (first %s: got %r, want %r)' % (
            what, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), float(g[bad][0]), float(want[bad][0]))
    else:
        over = np.abs(g.double().numpy() - ref) - bound
        assert np.all(over <= 0), '%s: %d elements outside their bound, by up to %.3g' % (what, int((over > 0).sum()), float(over.max()))


def run_forward(case, BC, dyadic):
    from upflow_pytorch_amd import _lib
    (h, w), (H, W) = case
    x_np, _ = em.resize_case(case[0], case[1], BC, dyadic)
    B = BC // 2
    combos = [(rate, mis) for rate in (0, 1) for mis in (0, 1)]          # mis = 1: y 4-byte but not 16-byte aligned (one pixel per thread)
    A = arena32(1 + len(combos), max(x_np.size, B * 2 * H * W) + 8)
    x = A.block(B, 2, h, w, fill=t_(x_np))
    ys = [A.block(B, 2, H, W, misalign=mis) for _, mis in combos]
    snap = A.snapshot()
    for (rate, _), y in zip(combos, ys):
        _lib.call('upf_flow_upsample_forward', _lib.ptr(x), _lib.ptr(y), B, 2, h, w, H, W, rate, stream())
    torch.cuda.synchronize()
    for (rate, mis), y in zip(combos, ys):
        ref, ra = em.resize_forward_ref(x_np, H, W, bool(rate))
        compare(y, ref, None if dyadic else em.gamma(4 + rate) * ra, 'resize %s BC %d rate %d misaligned %d' % (cid(case), BC, rate, mis))
    assert A.untouched(snap, *ys), OUTSIDE


@pytest.mark.parametrize('case', em.RESIZE_FWD_DYADIC, ids=cid)
def test_resize_forward_dyadic(case):
    for BC in em.RESIZE_BC:
        run_forward(case, BC, True)


@pytest.mark.parametrize('case', em.RESIZE_FWD_GENERAL, ids=cid)
def test_resize_forward_general(case):
    for BC in em.RESIZE_BC:
        run_forward(case, BC, False)


def run_backward(case, BC, dyadic, route=None):
    from upflow_pytorch_amd import _lib
    (h, w), (H, W) = case
    if route is not None:
        assert em.upsample_bwd_route(h, w, H, W, BC) == route
    _, gy_np = em.resize_case(case[0], case[1], BC, dyadic)
    B = BC // 2
    A = arena32(3, max(gy_np.size, B * 2 * h * w) + 8)
    gy = A.block(B, 2, H, W, fill=t_(gy_np))
    gxs = [A.block(B, 2, h, w) for _ in (0, 1)]
    snap = A.snapshot()
    for rate, gx in enumerate(gxs):
        _lib.call('upf_flow_upsample_backward', _lib.ptr(gy), _lib.ptr(gx), B, 2, h, w, H, W, rate, stream())
    torch.cuda.synchronize()
    for rate, gx in enumerate(gxs):
        ref, ra, nnz = em.resize_backward_ref(gy_np, h, w, bool(rate))
        bound = None if dyadic else em.gamma(nnz + em.RESIZE_TREE_DEPTH + 2 + rate)[None, None] * ra
        compare(gx, ref, bound, 'resize backward %s (%s) BC %d rate %d' % (cid(case), route or em.upsample_bwd_route(h, w, H, W, BC), BC, rate))
    assert A.untouched(snap, *gxs), OUTSIDE


@pytest.mark.parametrize('route,case', em.RESIZE_BWD_ROUTES, ids=['%s-%s' % (r, cid(c)) for r, c in em.RESIZE_BWD_ROUTES])
def test_resize_backward_every_route_is_exact(route, case):
    for BC in em.RESIZE_BC:
        run_backward(case, BC, True, route)


@pytest.mark.parametrize('case', em.RESIZE_BWD_GENERAL, ids=cid)
def test_resize_backward_general(case):
    for BC in em.RESIZE_BC:
        run_backward(case, BC, False)
