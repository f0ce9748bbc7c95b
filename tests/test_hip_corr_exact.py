"""The cost-volume kernels (csrc/corr81_fwd.hip: corr81_allc_kernel.hpp in its four tile geometries, aligned and ragged form,
corr81_mfma_kernel.hpp single- and multi-chunk, corr81_fwd_kernel.hpp aligned and unaligned, 16-bit and fp32, the general-parameter
kernel; csrc/corr81_bwd.hip: the tiled kernel aligned and ragged, the gather kernel, the general-parameter gradients) against an
fp64 reference BIT FOR BIT, every route of the host dispatch.

The operands sit on grids for which every partial sum of every summation order is exact in fp32 (tests/_exact_model.py, the
cost-volume section; tests/test_exact_model_cpu.py checks the conditions without a GPU).  What a correct kernel stores is then
determined by the exact fp64 sum S alone: for a power-of-two C the exact S / C, rounded once (RNE) for a 16-bit output.  For any
other C include/upflow_hip.h states the value as (1/C) * sum and the general kernel divides, so the expected fp32 value is ONE OF
TWO, both computed here from S: fp32(S / C) or fp32(S * fp32(1 / C)); a 16-bit output is one RNE of one of them (the two round to
the same 16-bit value in all but < 0.1 % of the elements — checked on the CPU — so this is no tolerance).  The LeakyReLU acts on
the fp32 value before that rounding: slope 0 = none, 0.125 exact, and the model's 0.1 once per kernel family in the epilogue's own
order (_exact_model.slope01_ref).  Values are compared as values (signed zeros are equal); there is no tolerance in this file.

Every operand is a contiguous block of a NaN-filled arena and so is every output an entry point lets the caller pass: whatever a
kernel reads outside its operands is NaN, whatever it writes outside its output shows in `untouched`.

Routes (what selects each is read off route() in csrc/corr81_fwd.hip and upf_corr81_backward):
  all-channels kernel, geometry 0..3 (8x32, 4x32, 2x32, 4x16 tiles)   corr_set_option('variant', v) where C fits, else the default pick
    aligned form: W % 8 == 0, 16-byte aligned f1 / f2 / out, out_batch_stride % 8 == 0; ragged form: anything else with W >= 4
  MFMA kernel   old_path = 1 on the aligned form's conditions (one chunk: C <= 32); no option: C > 208, or C > 40 on >= 160 8x32 tiles
  chunked kernel   old_path = 1 on ragged rows; UPF_CORR_NO_MFMA on aligned rows; W < 4; C > 208 on ragged rows; every fp32 launch
  tiled backward   W >= 4: aligned form for W % 4 == 0 and aligned pointers, ragged form otherwise
  gather backward   W < 4, or UPF_CORR_BWD_GATHER set"""
import contextlib
import os

import pytest
import torch

import _exact_model as em
from oracle import ops as oops
from test_hip_ops import GENERAL_SETS

pytestmark = pytest.mark.gpu

F32 = torch.float32
DT = [pytest.param(d, id=em.DTYPE_NAMES[d]) for d in em.DTYPES]
# (storage type, grid): fp32 runs on both 16-bit grids
ST = DT + [pytest.param((F32, d), id='fp32_on_%s_grid' % em.DTYPE_NAMES[d]) for d in em.DTYPES]
OUTSIDE = 'stored outside the output'
SLOPES = (0.0, em.SLOPE)


def split(st):
    """-> (storage dtype, grid dtype)"""
    return st if isinstance(st, tuple) else (st, st)


def arena(dtype, *numels):
    elems = sum(numels) + (len(numels) + 1) * (em.Arena.MARGIN + 16)
    return em.Arena32('cuda', elems) if dtype == F32 else em.Arena(dtype, 'cuda', elems)


@contextlib.contextmanager
def route(name):
    """'default', 'v0'..'v3' (tile geometry), 'old' (old_path = 1), 'nomfma' (UPF_CORR_NO_MFMA), 'gather' (UPF_CORR_BWD_GATHER):
    the library reads its options and environment per launch; everything is restored."""
    from upflow_pytorch_amd import ops
    opts = {'old': {'old_path': 1}}.get(name, {'variant': int(name[1])} if name[0] == 'v' else {})
    env = {'nomfma': 'UPF_CORR_NO_MFMA', 'gather': 'UPF_CORR_BWD_GATHER'}.get(name)
    assert opts or env or name == 'default', name
    prev, prev_env = {}, os.environ.get(env) if env else None
    try:
        for k, v in opts.items():
            prev[k] = ops.corr_set_option(k, v)
        if env:
            os.environ[env] = '1'
        yield
    finally:
        for k, v in prev.items():
            ops.corr_set_option(k, v)
        if env:
            if prev_env is None:
                os.environ.pop(env, None)
            else:
                os.environ[env] = prev_env


def either(got, cands, what):
    """Every element of `got` equals that element of one of `cands` (as a value; NaN matches NaN)."""
    g = got.detach().cpu()
    ok = torch.zeros(g.shape, dtype=torch.bool)
    for c in cands:
        assert c.dtype == g.dtype and c.shape == g.shape, (what, c.dtype, g.dtype, c.shape, g.shape)
        ok |= (g == c) | (torch.isnan(g) & torch.isnan(c))
    bad = int((~ok).sum())
    assert bad == 0, '%s: %d of %d elements are neither spelling of the exact value (first at %s: got %r, want %r); %d unexpected NaN' % (
        what, bad, g.numel(), tuple((~ok).nonzero()[0].tolist()), float(g[~ok][0]), [float(c[~ok][0]) for c in cands],
        int((torch.isnan(g) & ~torch.isnan(cands[0])).sum()))


def run_forward(f1, f2, S, dtype, slopes=SLOPES, mis=(0, 0, 0), channels=81, what=''):
    """ops.corr81_forward_raw per slope on arena blocks (mis: misalignment in elements of f1, f2, out; channels = 115: `out` is the
    first 81 channels of the estimator's input buffer) -> the outputs, compared with the reference and watched."""
    from upflow_pytorch_amd import ops
    B, C, H, W = f1.shape
    A = arena(dtype, f1.numel() + 8, f2.numel() + 8, *[B * channels * H * W + 8] * len(slopes))
    a, b = A.block(B, C, H, W, mis[0], fill=f1), A.block(B, C, H, W, mis[1], fill=f2)
    outs = [A.block(B, channels, H, W, mis[2])[:, :81] for _ in slopes]
    snap = A.snapshot()
    for slope, out in zip(slopes, outs):
        assert ops.corr81_forward_raw(a, b, out, slope) is out
    torch.cuda.synchronize()
    for slope, out in zip(slopes, outs):
        either(out, em.corr_expected(S, C, slope, dtype), '%s %s slope %g' % (what, tuple(f1.shape), slope))
    assert A.untouched(snap, *outs), OUTSIDE
    return outs


def forward_case(shape, st, slopes=SLOPES, **kw):
    dtype, gd = split(st)
    f1, f2, _, S = em.corr_case(tuple(shape), gd)
    return run_forward(f1, f2, S, dtype, slopes, **kw)


# ---- forward, 16-bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('variant', ['default', 'v0', 'v1', 'v2', 'v3'])
@pytest.mark.parametrize('shape', em.CORR_ALLC + em.CORR_SMALL, ids=str)
def test_forward_every_tile_geometry(shape, variant, dtype):
    """The four all-channels geometries and the default pick, aligned (W = 40) and ragged (35, 20, 13, 4) rows, C = 5 ... 208, B = 2."""
    with route(variant):
        forward_case(shape, dtype, what=variant)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('shape', em.CORR_OLD, ids=str)
def test_forward_old_path(shape, dtype):
    """old_path = 1: the MFMA kernel on aligned rows (one chunk C <= 32, several C = 33, 96), the chunked kernel elsewhere (W = 35
    unaligned, W = 20 its 4-pixel-aligned form)."""
    with route('old'):
        forward_case(shape, dtype, what='old_path')


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('shape', [(2, 32, 9, 40), (1, 33, 9, 40), (1, 96, 9, 40)], ids=str)
def test_forward_chunked_kernel_on_aligned_rows(shape, dtype):
    with route('nomfma'):
        forward_case(shape, dtype, what='UPF_CORR_NO_MFMA')


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('shape', em.CORR_DEEP + em.CORR_SHORT, ids=str)
def test_forward_beyond_the_all_channels_kernel(shape, dtype):
    """No option set: C = 212, 256 (nothing fits LDS: the multi-chunk MFMA kernel on aligned rows, the chunked kernel on ragged
    ones) and W = 1, 3 (rows shorter than a staging quad: the chunked kernel)."""
    forward_case(shape, dtype)


@pytest.mark.parametrize('dtype', DT)
def test_forward_many_tiles_route(dtype):
    """C > 40 on >= 160 8x32 tiles (route() leaves these to the chunked kernels): the MFMA kernel by default; (8, 48, 40, 128) is the smallest such grid."""
    B, C, H, W = em.CORR_BIG
    assert C > 40 and B * -(-H // 8) * -(-W // 32) >= 160
    forward_case(em.CORR_BIG, dtype)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('which', [0, 1, 2], ids=['f1', 'f2', 'out'])
def test_forward_ragged_form_from_a_misaligned_pointer(which, dtype):
    """W % 8 == 0 but f1 / f2 / out starts one element past a 16-byte boundary: the ragged form."""
    mis = [0, 0, 0]
    mis[which] = 1
    forward_case((2, 32, 9, 40), dtype, mis=tuple(mis))
    forward_case((1, 96, 9, 40), dtype, mis=tuple(mis))


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('shape', [(2, 32, 9, 35), (2, 32, 9, 40), (2, 5, 5, 4)], ids=str)
def test_forward_into_the_115_channel_buffer(shape, dtype):
    """`out` = the first 81 of 115 channels.  H * W odd: out_batch_stride % 8 != 0, the ragged form; H * W * 115 % 8 == 0 with
    W % 8 == 0: the aligned form.  Channels 81 ... 114 keep their bits (`untouched`)."""
    B, C, H, W = shape
    assert (W % 8 == 0 and (H * W * 115) % 8 == 0) or (H * W * 115) % 8 != 0
    forward_case(shape, dtype, channels=115)
    with route('old'):
        forward_case(shape, dtype, channels=115, what='old_path')


FAMILIES = [('default', (2, 32, 9, 40)), ('default', (2, 32, 9, 35)), ('old', (2, 32, 9, 40)), ('old', (1, 96, 9, 40)), ('old', (1, 33, 9, 35)),
            ('old', (1, 33, 6, 20)), ('nomfma', (1, 33, 9, 40)), ('default', (1, 212, 9, 40)), ('default', (2, 33, 5, 3))]


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('family', FAMILIES, ids=lambda f: '%s-%s' % (f[0], 'x'.join(map(str, f[1]))))
def test_forward_slope_01_once_per_kernel_family(family, dtype):
    """The model's slope: fp32 multiply by float32(0.1), the maximum, then the one rounding."""
    with route(family[0]):
        forward_case(family[1], dtype, slopes=(0.1,), what=family[0])


# ---- forward, fp32 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('st', ST[2:])
@pytest.mark.parametrize('shape', em.CORR_F32, ids=str)
def test_forward_fp32(shape, st):
    """fp32 (the parity mode) on the same grids: exactly one of the two fp32 spellings; W % 4 == 0 and not."""
    forward_case(shape, st, slopes=(0.0, em.SLOPE, 0.1))


@pytest.mark.parametrize('st', ST[2:])
def test_forward_fp32_misaligned_and_into_the_115_channel_buffer(st):
    for mis in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        forward_case((2, 32, 9, 40), st, mis=mis)
    for shape in ((2, 32, 9, 40), (1, 33, 5, 13), (1, 5, 9, 35)):
        forward_case(shape, st, channels=115)


# ---- forward, non-finite operands -------------------------------------------------------------------------------------------------------
NF_FAMILIES = [('default', 0), ('default', 1), ('old', 0), ('old', 1), ('nomfma', 0)]
# (the options select among the 16-bit kernels only: fp32 runs its one kernel, on both widths)
NF_RUNS = [pytest.param(f, d, id='%s-%s-%s' % (f[0], ('aligned', 'ragged')[f[1]], em.DTYPE_NAMES[d])) for f in NF_FAMILIES for d in em.DTYPES] + \
          [pytest.param(('default', w), (F32, torch.float16), id='fp32-%s' % ('aligned', 'ragged')[w]) for w in (0, 1)]


@pytest.mark.parametrize('kind', em.CORR_NF_FWD, ids='-'.join)
@pytest.mark.parametrize('family,st', NF_RUNS)
def test_forward_nonfinite_operand_reaches_exactly_its_window(family, st, kind):
    """One NaN in f2 reaches exactly the outputs whose window covers it (the zero padding comes from buffer descriptors and halo
    staging: nothing else may turn non-finite, nothing may stay finite); one +inf in f1 the 81 channels of its pixel, with the
    reference's NaN / +-inf pattern.  Everything else keeps the reference's bits.  Families: all-channels aligned / ragged, MFMA,
    chunked unaligned / aligned, fp32."""
    dtype, gd = split(st)
    shape = em.CORR_NF_SHAPES[family[1]]
    f1, f2, S, count = em.corr_nonfinite_fwd(shape, gd, kind)
    with route(family[0]):
        outs = run_forward(f1, f2, S, dtype, what='%s %s' % (family[0], kind))
    for out in outs:
        assert int((~torch.isfinite(out)).sum()) == count


# ---- backward -------------------------------------------------------------------------------------------------------------------------
def run_backward(f1, f2, go, G1, G2, dtype, mis=(0, 0, 0), what=''):
    """ops.corr81_backward_raw on arena blocks, g1 / g2 carved from the arena too (mis: misalignment of grad_out, f1, g1)."""
    from upflow_pytorch_amd import ops
    B, C, H, W = f1.shape
    A = arena(dtype, *[f1.numel() + 8] * 4 + [go.numel() + 8])
    a, b = A.block(B, C, H, W, mis[1], fill=f1), A.block(B, C, H, W, fill=f2)
    g = A.block(B, 81, H, W, mis[0], fill=go)
    g1, g2 = A.block(B, C, H, W, mis[2]), A.block(B, C, H, W)
    snap = A.snapshot()
    r1, r2 = ops.corr81_backward_raw(a, b, g, g1, g2)
    torch.cuda.synchronize()
    assert r1 is g1 and r2 is g2
    either(g1, em.corr_expected(G1, C, 0.0, dtype), '%s g1 %s' % (what, tuple(f1.shape)))       # (an element left unwritten is still NaN)
    either(g2, em.corr_expected(G2, C, 0.0, dtype), '%s g2 %s' % (what, tuple(f1.shape)))
    assert A.untouched(snap, g1, g2), OUTSIDE
    return g1, g2


@pytest.mark.parametrize('st', ST[:3])
@pytest.mark.parametrize('kernel', ['default', 'gather'])
@pytest.mark.parametrize('shape', em.CORR_BWD, ids=str)
def test_backward(shape, kernel, st):
    """The tiled kernel in its aligned (W % 4 == 0: 68 crosses the 64-pixel tile, H = 17 the 16-row tile, C = 5, 33, B = 2) and
    ragged form (W = 5, 13, 26, 67), the gather kernel where it is the only one (W = 1, 2, 3) and forced onto all the others (C = 5
    and 33: the host splits the channels over blockIdx.y and the last block is short).  Both equal the one reference, hence each other."""
    dtype, gd = split(st)
    f1, f2, go, G1, G2 = em.corr_grad_case(tuple(shape), gd)
    with route(kernel):
        run_backward(f1, f2, go, G1, G2, dtype, what=kernel)


@pytest.mark.parametrize('st', ST[:3])
@pytest.mark.parametrize('which', [0, 1, 2], ids=['grad_out', 'f1', 'g1'])
def test_backward_ragged_form_from_a_misaligned_pointer(which, st):
    dtype, gd = split(st)
    mis = [0, 0, 0]
    mis[which] = 1
    f1, f2, go, G1, G2 = em.corr_grad_case((1, 8, 6, 12), gd)
    run_backward(f1, f2, go, G1, G2, dtype, mis=tuple(mis))


@pytest.mark.parametrize('st', ST[:3])
@pytest.mark.parametrize('kind', em.CORR_NF_BWD, ids='-'.join)
@pytest.mark.parametrize('kernel', [('default', 0), ('default', 1), ('gather', 0), ('gather', 1), ('default', 2)],
                         ids=['tiled-aligned', 'tiled-ragged', 'gather-forced-w12', 'gather-forced-w13', 'gather-w3'])
def test_backward_single_nonfinite_grad_out_element(kernel, kind, st):
    """One NaN / +inf element of grad_out, interior and border, in all three kernels: the exact non-finite pattern of the reference
    (g1: the pixel's C channels — also where the displacement points outside the image, where f2 is the zero the header states and
    gO times it is NaN; g2: the C channels of the target pixel, if it exists) and its bits everywhere else."""
    dtype, gd = split(st)
    f1, f2, go, G1, G2, n1, n2 = em.corr_nonfinite_bwd(em.CORR_NF_BWD_SHAPES[kernel[1]], gd, kind)
    with route(kernel[0]):
        g1, g2 = run_backward(f1, f2, go, G1, G2, dtype, what='%s %s' % (kernel[0], kind))
    assert int((~torch.isfinite(g1)).sum()) == n1 and int((~torch.isfinite(g2)).sum()) == n2


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('shape', em.CORR_AUTOGRAD, ids=str)
def test_autograd_masks_with_the_output_and_zeros_take_the_slope(shape, dtype):
    """ops.corr81(f1, f2, 0.125) under autograd: the gradient is masked with out > 0 ? 1 : slope before the backward kernels; H = 4
    makes the dy = -4 / +4 channels exact zeros everywhere, so the convention at zero shapes g1 and g2."""
    from upflow_pytorch_amd import ops
    B, C, H, W = shape
    f1, f2, go, S = em.corr_case(tuple(shape), dtype)
    _, _, gm, G1, G2 = em.corr_grad_case(tuple(shape), dtype, em.SLOPE)
    A = arena(dtype, f1.numel() + 8, f2.numel() + 8, go.numel() + 8)
    a, b = A.block(B, C, H, W, fill=f1).requires_grad_(True), A.block(B, C, H, W, fill=f2).requires_grad_(True)
    g = A.block(B, 81, H, W, fill=go)
    snap = A.snapshot()
    out = ops.corr81(a, b, em.SLOPE)
    g1, g2 = torch.autograd.grad(out, (a, b), g)
    either(out, em.corr_expected(S, C, em.SLOPE, dtype), 'out')
    either(g1, em.corr_expected(G1, C, 0.0, dtype), 'g1')
    either(g2, em.corr_expected(G2, C, 0.0, dtype), 'g2')
    assert A.untouched(snap), OUTSIDE


# ---- the general parameter list ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('st', ST[:3])
@pytest.mark.parametrize('params', GENERAL_SETS, ids=lambda p: '_'.join(map(str, p)))
def test_general_parameters(params, st):
    """correlation_forward_general (divides by k * k * C) and, where the backward is defined, correlation_backward_general;
    (4,1,4,1,1) routes to the tuned kernels and gives their bits."""
    from upflow_pytorch_amd import ops
    dtype, gd = split(st)
    pad, k, md, s1, s2 = params
    f1, f2, go, S, G1, G2 = em.corr_general_case(tuple(params), gd)
    B, C, H, W = f1.shape
    A = arena(dtype, *[f1.numel() + 8] * 4 + [S.numel() + 8] * 2)
    a, b = A.block(B, C, H, W, fill=f1), A.block(B, C, H, W, fill=f2)
    out = A.block(*S.shape)
    written = [out]
    snap = A.snapshot()
    assert ops.correlation_forward_general(a, b, pad, k, md, s1, s2, out=out) is out
    either(out, em.corr_expected(S, k * k * C, 0.0, dtype), 'forward %s' % (params,))
    if oops.correlation_backward_supported(pad, k, md, s1, s2):
        assert go is not None
        g, g1, g2 = A.block(*S.shape, fill=go), A.block(B, C, H, W), A.block(B, C, H, W)
        written += [g, g1, g2]
        ops.correlation_backward_general(a, b, g, pad, k, md, s1, s2, g1=g1, g2=g2)
        either(g1, em.corr_expected(G1, C, 0.0, dtype), 'g1 %s' % (params,))
        either(g2, em.corr_expected(G2, C, 0.0, dtype), 'g2 %s' % (params,))
        if tuple(params) == (4, 1, 4, 1, 1):
            t1, t2 = ops.corr81_backward_raw(a, b, g)
            assert torch.equal(out, ops.corr81_forward_raw(a, b)) and torch.equal(g1, t1) and torch.equal(g2, t2)
    else:
        assert go is None
    assert A.untouched(snap, *written), OUTSIDE
