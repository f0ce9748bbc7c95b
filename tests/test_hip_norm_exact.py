"""The feature-normalisation kernels (csrc/misc.hip: normalize_stats_wave_kernel, normalize_stats_kernel with its segmented rows merged
by norm_merge_add, normalize_apply_kernel, normalize_bwd_kernel) against the fp64 model of tests/_exact_model.py — a reference, not
another kernel.  tests/test_exact_model_cpu.py checks every route name, cap and count without a GPU.  DESIGN.md 4.12.

General regime only (the statistics are long fp32 sums).  The reference: mean, unbiased variance and std = sqrt(var + float32(1e-16)) in
fp64 from the STORED operand.  Bounds, from the reference alone, gamma_k with k the fp32 roundings along the route's longest path
(k = V ceil(seglen / (threads V)) + 9 + 8 (nseg - 1)):
  mean   within gamma_k sum |x - K| / n + u |mean|          (K: the pivot — the first element of each segment; 0 for fp32's two sweeps)
  rstd   within gamma_k kappa + 3 u, relative                (kappa = 1 + sum_seg n_seg (mean_seg - K_seg)^2 / M2; 1 for fp32)
  y      fp32 inside ref +- b, 16-bit RNE of one end of it (accept_y), b = |y| (b_rstd + 2 u) + b_mean / std
  y      16-bit, in addition: bit for bit RNE(fl(fl(x - mean) rstd)) of the mean and rstd the SAME call returned — apply1's two fp32
         operations; no tolerance (the statistics' bounds above carry the rest)
The spike rows (first element 512 standard-deviations-and-more off the row) run under the same bounds, wide there because kappa is in
the thousands; their messages record kappa and the observed error.

Every operand and output is a block of a NaN-filled arena; `untouched` is asserted after every call."""
import numpy as np
import pytest
import torch

import _exact_model as em

pytestmark = pytest.mark.gpu

F32 = em.F32
OUTSIDE = 'stored outside the output'
CASES = [pytest.param(n, d, id='%s-%s' % (n, em.SAMP_NAMES[d])) for n in em.NORM_CASES for d in em.norm_dtypes(n)]
SDT = [pytest.param(d, id=em.SAMP_NAMES[d]) for d in em.SAMP_DTYPES]


def arena(dtype, nblocks, numel):
    elems = nblocks * (numel + em.Arena.MARGIN + 64) + em.Arena.MARGIN + 64
    return em.Arena32('cuda', elems) if dtype == F32 else em.Arena(dtype, 'cuda', elems)


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def stream():
    from upflow_pytorch_amd import _lib
    return _lib.stream_ptr(torch.device('cuda', torch.cuda.current_device()))


def forward(x_np, dtype, misalign=0):
    """upf_normalize_forward on a [N, HW] operand in the arena -> (route, mean, rstd, y) on the CPU; asserts nothing is stored outside."""
    from upflow_pytorch_amd import _lib
    N, HW = x_np.shape
    A, A32 = arena(dtype, 4, N * HW + 8), arena(F32, 2, N)
    x = A.block(1, 1, N, HW, misalign=misalign, fill=t_(x_np))
    y = A.block(1, 1, N, HW, misalign=misalign)
    stats = [A32.block(1, 1, 1, N) for _ in range(2)] if dtype != F32 else [A.block(1, 1, 1, N) for _ in range(2)]
    ws = torch.empty(_lib.lib().upf_normalize_workspace_bytes(N, HW), dtype=torch.uint8, device='cuda')
    aligned = x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    assert aligned == (misalign == 0)
    snap, snap32 = A.snapshot(), A32.snapshot()
    _lib.call('upf_normalize_forward', _lib.ptr(x), _lib.ptr(y), _lib.ptr(stats[0]), _lib.ptr(stats[1]), _lib.ptr(ws), N, HW, _lib._DTYPES[dtype], stream())
    torch.cuda.synchronize()
    written = [y] + (stats if dtype == F32 else [])
    assert A.untouched(snap, *written) and A32.untouched(snap32, *(stats if dtype != F32 else [])), OUTSIDE
    return em.normalize_route(N, HW, dtype, aligned), stats[0].cpu().reshape(N), stats[1].cpu().reshape(N), y.cpu().reshape(N, HW)


@pytest.mark.parametrize('name,dtype', CASES)
def test_normalize_forward(name, dtype):
    c = em.norm_case(name, dtype)
    route, mean, rstd, y = forward(c['x'], dtype, c['misalign'])
    ref = em.norm_forward_ref(c['x'], route, dtype)
    what = '%s %s %s' % (name, em.SAMP_NAMES[dtype], route)
    mean64, rstd64 = mean.double().numpy(), rstd.double().numpy()
    e_mean = np.abs(mean64 - ref['mean'])
    e_rstd = np.abs(rstd64 - ref['rstd']) / ref['rstd']
    note = '%s: kappa up to %.3g, mean off by up to %.3g (bound %.3g), rstd by up to %.3g relative (bound %.3g)' % (
        what, ref['kappa'].max(), e_mean.max(), ref['b_mean'][e_mean.argmax()], e_rstd.max(), ref['b_rstd'][e_rstd.argmax()])
    print(note)
    assert np.all(e_mean <= ref['b_mean']), note
    assert np.all(e_rstd <= ref['b_rstd']), note
    ok = em.accept_y(y, ref['y'], ref['b_y'], dtype)
    assert ok.all(), '%s: %d of %d values of y outside their bound (first at %s)' % (note, int((~ok).sum()), ok.size, tuple(np.argwhere(~ok)[0]))
    if dtype != F32:
        x32 = np.asarray(c['x'], dtype=np.float32)
        want = t_((x32 - mean.numpy()[:, None]) * rstd.numpy()[:, None]).to(dtype)
        bad = y != want
        assert not bool(bad.any()), '%s: y is not RNE((x - mean) * rstd) of the returned statistics at %d of %d elements' % (what, int(bad.sum()), bad.numel())


@pytest.mark.parametrize('name', ['hw63_9rows', 'seg2_2052', 'seg2_ragged', 'seg4_ragged'])
@pytest.mark.parametrize('dtype', SDT)
def test_normalize_pair_equals_one_call_over_the_concatenated_rows(dtype, name):
    """ops.normalize_pair's two calls and ONE upf_normalize_forward over the rows of both tensors: the same bits wherever normalize_nseg
    agrees (a row's statistics never depend on its neighbours)."""
    from upflow_pytorch_amd import ops
    shape = em.NORM_CASES[name][0]
    B, C, H, W = shape
    a, b = em.norm_case(name, dtype)['x'], em.norm_case(name, dtype)['x'][::-1].copy()
    N, HW = a.shape
    both = np.concatenate([a, b], 0)
    assert em.normalize_route(N, HW, dtype) == em.normalize_route(2 * N, HW, dtype)
    ya, yb = ops.normalize_pair(t_(a).to(dtype).cuda().view(B, C, H, W), t_(b).to(dtype).cuda().view(B, C, H, W))
    _, _, _, y = forward(both, dtype)
    got = torch.cat([ya.reshape(-1, HW), yb.reshape(-1, HW)], 0).cpu()
    assert torch.equal(got.view(torch.int32 if dtype == F32 else torch.int16), y.view(torch.int32 if dtype == F32 else torch.int16))


@pytest.mark.parametrize('HW', em.NORM_BWD_HW)
@pytest.mark.parametrize('dtype', SDT)
def test_normalize_backward(dtype, HW):
    """upf_normalize_backward with operands of the test's choosing: gx = r (g - mean(g) - y sum(g y) / (HW - 1)) in fp64, within gamma_k on
    sum |g| / HW + |y| sum |g y| / (HW - 1) + |g|, times |r|, k = ceil(HW / 512) + 9 + 4."""
    from upflow_pytorch_amd import _lib
    y_np, gy_np, r_np = em.norm_bwd_case(HW, dtype)
    N = y_np.shape[0]
    A, A32 = arena(dtype, 3 + (dtype == F32), N * HW), arena(F32, 1, N)
    y, gy = A.block(1, 1, N, HW, fill=t_(y_np)), A.block(1, 1, N, HW, fill=t_(gy_np))
    gx = A.block(1, 1, N, HW)
    rstd = (A if dtype == F32 else A32).block(1, 1, 1, N, fill=t_(r_np))
    snap, snap32 = A.snapshot(), A32.snapshot()
    _lib.call('upf_normalize_backward', _lib.ptr(y), _lib.ptr(gy), _lib.ptr(rstd), _lib.ptr(gx), N, HW, _lib._DTYPES[dtype], stream())
    torch.cuda.synchronize()
    assert A.untouched(snap, gx) and A32.untouched(snap32), OUTSIDE
    ref, bound = em.norm_backward_ref(y_np, gy_np, r_np)
    ok = em.accept_y(gx.cpu().reshape(N, HW), ref, bound, dtype)
    assert ok.all(), 'HW %d %s: %d of %d gradients outside their bound' % (HW, em.SAMP_NAMES[dtype], int((~ok).sum()), ok.size)
