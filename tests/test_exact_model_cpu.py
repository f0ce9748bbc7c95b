"""The conditions tests/test_hip_conv_exact.py rests on, checked on tests/_exact_model.py alone (no GPU, nothing from the code under
test): the guard holds for every case list, torch's fp32 kernels in their own summation order reproduce the fp64 reference bit for
bit (the order independence the GPU file relies on), the operands make enough outputs round / tie / hit zero for bit equality to
mean something, and the fp16 range cases are what they claim to be.  The last section does the same for the sampling model
(tests/test_hip_warp_exact.py, tests/test_hip_resize_exact.py): the fp32 position chain against the golden mask bits, the guards of
the dyadic regime, the caps of the general one, route coverage, and what each backward case claims to contain — and for the
normalisation, blend, occlusion and census models (tests/test_hip_norm_exact.py, tests/test_hip_blend_exact.py): route names, caps,
counts, the NaN pixel of the occlusion oracle, the census adjoint against fp64 autograd."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _exact_model as em
import _lossvar as lv
from conftest import GOLDEN, load_golden, unpack_mask

DT = [pytest.param(d, id=em.DTYPE_NAMES[d]) for d in em.DTYPES]


@pytest.mark.parametrize('dtype', DT)
def test_guard_holds_for_every_training_case(dtype):
    for layer in em.TRAIN + em.NONFINITE_LAYERS:
        variants = [(em.SLOPE, True, layer in em.NONFINITE_LAYERS)]
        if layer.name in em.MATRIX_LAYERS:
            variants += [(0.0, True, False), (em.SLOPE, False, False), (0.0, False, False)]
        for slope, bias, nonzero in variants:
            g = em.train_case(layer.name, dtype, slope, bias, nonzero)[3]
            assert set(g) == {'y', 'gx', 'gw', 'gb'} and max(g.values()) < em.LIMIT
    for name in em.SCALE_LAYERS:
        for k in em.SCALE_K[dtype]:
            em.train_case(name, dtype, em.SLOPE, True, False, k, em.SCALE_GY[dtype])


@pytest.mark.parametrize('dtype', DT)
def test_guard_holds_for_the_weight_gradient_and_forward_lists(dtype):
    for conv, n in em.WG_CASES:
        Cin, Cout, k, d = em.WG_CONVS[conv]
        uses, st = em.wgrad_operands(conv, n, dtype)
        em.guard_wgrad(uses, (Cout, Cin, k, k), d, 1, st['x'], st['gy'])
        em.guard_bias([g for _, g in uses], st['gy'])
    for name in [l.name for l in em.FWD] + list(em.C8) + list(em.C8_NARROW):
        em.forward_case(name, dtype)
    for name, cfg in em.PAIR.items():
        for sa, sb in ((em.SLOPE, em.SLOPE), (em.SLOPE, 0.0)):
            em.pair_ref(em.pair_operands(name, dtype), cfg[6], sa, sb, dtype)
    for layer in em.GATED:
        em.gated_case(layer, dtype)
    for shape in em.ACT_SHAPES:
        em.act_case(shape, dtype)
        parts = em.bias_parts_case(shape, dtype)
        assert len(parts) == 9 and len({float(t.double().sum()) for t in parts}) == 9
    for geom in em.TAIL:
        em.tail_case(geom, dtype)
    for geom in em.DUAL:
        em.dual_case(geom, dtype)
    em.shared_case(dtype)


def test_guard_refuses_what_it_must():
    layer = em.Layer('t', 1, 8, 4, 5, 8)
    o = em.operands(layer, torch.bfloat16)
    with pytest.raises(AssertionError):                                  # an operand off its grid
        em.guard_forward(o['x'] + 0.5, o['w'], o['b'], 3, 1, 1, o['steps'])
    with pytest.raises(AssertionError):                                  # too many quanta: the same operands on a 2^-22 finer grid
        em.guard_forward(o['x'], o['w'], o['b'], 3, 1, 1, dict(o['steps'], w=2.0 ** -24))
    with pytest.raises(AssertionError):
        em.guard_bias([torch.full((1, 1, 4096, 4096), 1.0)], 0.5)


@pytest.mark.parametrize('dtype', DT)
def test_torch_fp32_in_its_own_order_reproduces_the_fp64_reference(dtype):
    """The CPU demonstration of order independence: another implementation, another summation order, fp32 accumulation — the
    same bits."""
    for layer in em.TRAIN:
        _, o, ref, _ = em.train_case(layer.name, dtype)
        gm = em.geom(layer.k, layer.d, layer.s)
        pre = F.conv2d(o['x'], o['w'], o['b'], **gm)
        assert torch.equal(pre.double(), ref['pre']), layer
        gpre = o['gy'] * em.act_mask(pre, em.SLOPE)
        assert torch.equal(gpre.double(), ref['gpre']), layer
        assert torch.equal(torch.nn.grad.conv2d_input(o['x'].shape, o['w'], gpre, **gm).double(), ref['gx']), layer
        assert torch.equal(torch.nn.grad.conv2d_weight(o['x'], o['w'].shape, gpre, **gm).double(), ref['gw']), layer
        assert torch.equal(gpre.sum((0, 2, 3)).double(), ref['gb']), layer
        for n in ('pre', 'y', 'gx', 'gw', 'gb'):                         # every reference value IS an fp32 value: one rounding to 16 bits
            assert torch.equal(ref[n].float().double(), ref[n]), (layer, n)
        assert torch.equal(ref['gpre'].to(dtype).double(), ref['gpre']), layer        # the 16-bit tensor the kernels store holds it exactly


@pytest.mark.parametrize('dtype', DT)
def test_operands_make_the_16_bit_stores_round(dtype):
    """Over the training list: >= 1 % of the 16-bit outputs and of the data gradients are exact RNE ties, >= 5 % need rounding
    (by the bit pattern of the exact fp32 value); every activated case has >= 20 exact-zero pre-activations."""
    for key in ('y', 'gx'):
        ties = rounded = total = 0
        for layer in em.TRAIN:
            ref = em.train_case(layer.name, dtype)[2]
            v = ref[key].float()
            ties += int(em.is_tie(v, dtype).sum())
            rounded += int(em.needs_rounding(v, dtype).sum())
            total += v.numel()
        print('%s %s: %.2f %% ties, %.2f %% rounded of %d' % (em.DTYPE_NAMES[dtype], key, 100.0 * ties / total, 100.0 * rounded / total, total))
        assert ties >= 0.01 * total and rounded >= 0.05 * total, (key, ties, rounded, total)
    for layer in em.TRAIN:
        ref = em.train_case(layer.name, dtype)[2]
        assert int((ref['pre'] == 0).sum()) >= 20, layer
    # the helpers themselves, on values whose rounding is known
    one = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, 3.0 * 2.0 ** -20])
    assert em.is_tie(one, torch.bfloat16).tolist() == [False, True, False, False, False, False]
    assert em.needs_rounding(one, torch.bfloat16).tolist() == [False, True, True, True, True, False]
    assert em.is_tie(one, torch.float16).tolist() == [False, False, False, True, False, False]
    assert em.needs_rounding(one, torch.float16).tolist() == [False, False, False, True, True, False]


def test_fp16_overflow_and_subnormal_cases_are_what_they_claim():
    name, k = em.FP16_OVERFLOW
    ref = em.train_case(name, torch.float16, em.SLOPE, True, False, k)[2]
    over = ref['gx'].abs() > 65504
    assert bool(over.any()) and bool((~over).any()) and bool(torch.isinf(ref['gx'].to(torch.float16)).any())
    assert bool(torch.isfinite(ref['gx'].to(torch.float16)).any())
    name, gg = em.FP16_SUBNORMAL
    _, o, ref, _ = em.train_case(name, torch.float16, em.SLOPE, True, False, 0, gg)
    for g in (o['gy'], ref['gpre'].float()):
        assert float(g.abs().max()) < 2.0 ** -14 and em.on_grid(g, 2.0 ** -24) and torch.equal(g.half().float(), g)
    assert float(ref['gw'].abs().max()) > 0 and int((ref['gw'] != 0).sum()) > ref['gw'].numel() // 2


@pytest.mark.parametrize('dtype', DT)
def test_power_of_two_scaling_stays_in_the_normal_range(dtype):
    """grad_y * 2^k: every non-zero element of the scaled operands and of the scaled 16-bit results is a normal number of the
    dtype, so the scaled run must give the clean run's bits times 2^k."""
    lo, hi = (2.0 ** -14, 65504.0) if dtype == torch.float16 else (2.0 ** -126, 3.0e38)
    for name in em.SCALE_LAYERS:
        clean = em.train_case(name, dtype, em.SLOPE, True, False, 0, em.SCALE_GY[dtype])[2]
        for k in em.SCALE_K[dtype]:
            _, o, ref, _ = em.train_case(name, dtype, em.SLOPE, True, False, k, em.SCALE_GY[dtype])
            for n in ('gx', 'gw', 'gb', 'gpre'):
                assert torch.equal(ref[n], clean[n] * 2.0 ** k), (name, k, n)
            for t in (o['gy'].double(), ref['gpre'], ref['gx'].to(dtype).double()):
                nz = t[t != 0].abs()
                assert float(nz.min()) >= lo and float(nz.max()) <= hi, (name, k)


def test_arena_poisons_and_watches_everything_outside_the_views():
    a = em.Arena(torch.bfloat16, 'cpu', 1 << 18)
    x = a.nchw(2, 3, 4, 13, before=2, after=1, pitch=16, fill=torch.ones(2, 3, 4, 13))
    y = a.nchw(2, 5, 4, 13)
    x8 = a.c8(1, 11, 4, 6, fill=torch.ones(1, 11, 4, 6))
    assert x.shape == (2, 3, 4, 13) and x.stride() == (6 * 4 * 16, 4 * 16, 16, 1) and bool((x == 1).all())
    assert x8.shape == (1, 2, 4, 6, 8) and x8.data_ptr() % 16 == 0
    assert bool((em.from_c8(x8)[:, :11] == 1).all()) and bool((em.from_c8(x8)[:, 11:] == 0).all())       # padding channels: zeros
    assert bool(torch.isnan(y).all())
    for v in (x, y, x8):
        off = v.storage_offset() - a.buf.storage_offset()
        assert off >= a.MARGIN and bool(torch.isnan(a.buf[off - a.MARGIN:off]).all())                     # >= 4 KiB of NaN in front
    total = int(torch.isnan(a.buf).sum())
    assert total == a.buf.numel() - x.numel() - x8.numel()
    snap = a.snapshot()
    y.fill_(2.0)
    assert a.untouched(snap, y) and not a.untouched(snap)
    a.buf[y.storage_offset() - 1] = 0.0                                  # one element in front of the output slice
    assert not a.untouched(snap, y)


# ---- the cost volume: the conditions tests/test_hip_corr_exact.py rests on -------------------------------------------------------------
def _general_sets():
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_hip_ops.py')).read()
    node = [n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], 'id', None) == 'GENERAL_SETS'][0]
    return ast.literal_eval(node.value)                                  # (the GPU module itself cannot be imported without a GPU package)


GENERAL_SETS = _general_sets()


@pytest.mark.parametrize('dtype', DT)
def test_corr_guard_holds_for_every_case(dtype):
    tops = [em.guard_corr(*em.corr_case(s, dtype)[:2], dtype) for s in em.CORR_FWD]
    print('%s forward: at most %.3g quanta' % (em.DTYPE_NAMES[dtype], max(tops)))
    assert max(tops) < em.LIMIT
    for s in em.CORR_BWD + em.CORR_AUTOGRAD:
        for slope in (0.0, em.SLOPE):                                    # (corr_grad_case guards; the masked gradient sits on the slope-times-finer grid)
            f1, f2, gm, G1, G2 = em.corr_grad_case(s, dtype, slope)
            assert G1.shape == f1.shape and G2.shape == f2.shape
    for params in GENERAL_SETS:
        em.corr_general_case(tuple(params), dtype)
    with pytest.raises(AssertionError):                                  # the guard refuses features off their grid
        em.guard_corr(em.corr_case(em.CORR_SMALL[0], dtype)[0] + 2.0 ** -9, em.corr_case(em.CORR_SMALL[0], dtype)[1], dtype)


@pytest.mark.parametrize('dtype', DT)
def test_corr_torch_fp32_in_its_own_order_reproduces_the_fp64_sums(dtype):
    """Another formulation (unfold + batched matrix product; autograd for the gradients), fp32 accumulation in torch's own order:
    the same bits as the fp64 shifted sums.  (The 6.6 MB case runs the shifted sums in fp32 instead: its unfolded f2 is 640 MB.)"""
    for s in em.CORR_FWD + em.CORR_BWD:
        B, C, H, W = s
        f1, f2, go, S = em.corr_case(s, dtype)
        if s == em.CORR_BIG:
            f2p = F.pad(f2, (4,) * 4)
            got = torch.stack([(f1 * f2p[:, :, dy:dy + H, dx:dx + W]).sum(1) for dy in range(9) for dx in range(9)], 1)
            assert torch.equal(got.double(), S), s
            continue
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        u = F.unfold(b, 9, padding=4).view(B, C, 81, H * W)              # u[n,c,d,p] = f2[n,c,p + d]
        got = torch.einsum('ncp,ncdp->ndp', a.view(B, C, H * W), u).view(B, 81, H, W)
        assert torch.equal(got.detach().double(), S), s
        if s in em.CORR_BWD:
            _, _, gm, G1, G2 = em.corr_grad_case(s, dtype)
            g1, g2 = torch.autograd.grad(got, (a, b), gm)
            assert torch.equal(g1.double(), G1) and torch.equal(g2.double(), G2), s
    # the general parameter list: the shifted sums at (4,1,4,1,1) ARE the 81-neighbour sums, and fp32 reproduces every set
    f1, f2, go, S = em.corr_case(em.CORR_SMALL[0], dtype)
    assert torch.equal(em.corr_general_sums(f1, f2, 4, 1, 4, 1, 1), S)
    G = em.corr_grad_sums(f1, f2, go)
    for want, got in zip(G, em.corr_general_grad_sums(f1, f2, go, 4, 1, 4, 1, 1)):
        assert torch.equal(got, want)
    for params in GENERAL_SETS:
        f1, f2, go, S, G1, G2 = em.corr_general_case(tuple(params), dtype)
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        pad, k, md, s1, s2 = params
        kr, dr = (k - 1) // 2, md // s2
        p1, p2 = F.pad(a, (pad,) * 4), F.pad(b, (pad,) * 4)
        oH, oW = S.shape[2:]
        chans = []
        for tj in range(-dr, dr + 1):
            for ti in range(-dr, dr + 1):
                y0, x0 = md - kr, md - kr                                 # fp32, strided slices instead of index tensors, patch summed last
                pa = torch.stack([p1[:, :, y0 + j:y0 + j + (oH - 1) * s1 + 1:s1, x0 + i:x0 + i + (oW - 1) * s1 + 1:s1] for j in range(k) for i in range(k)])
                pb = torch.stack([p2[:, :, y0 + tj * s2 + j:y0 + tj * s2 + j + (oH - 1) * s1 + 1:s1, x0 + ti * s2 + i:x0 + ti * s2 + i + (oW - 1) * s1 + 1:s1]
                                  for j in range(k) for i in range(k)])
                chans.append((pa * pb).sum(2).sum(0))
        got = torch.stack(chans, 1)
        assert torch.equal(got.detach().double(), S), params
        if go is not None:
            g1, g2 = torch.autograd.grad(got, (a, b), go)
            assert torch.equal(g1.double(), G1) and torch.equal(g2.double(), G2), params


@pytest.mark.parametrize('dtype', DT)
def test_corr_operands_make_the_stores_round_and_the_two_quotients_agree_in_16_bits(dtype):
    """Power-of-two C: >= 1 % of the outputs are exact RNE ties.  All cases: >= 5 % need rounding (forward and both gradients).
    Per case: the two fp32 spellings of S / C (IEEE quotient; product with the rounded reciprocal) round to DIFFERENT 16-bit values
    in at most 0.1 % of the elements — "either of the two" is no tolerance."""
    ties = pow2 = rounded = total = grounded = gtotal = 0
    for s in em.CORR_FWD:
        C = s[1]
        S = em.corr_case(s, dtype)[3]
        qd, qm = em.corr_quotients(S, C)
        differ16 = float((qd.to(dtype) != qm.to(dtype)).float().mean())
        differ32 = float((qd != qm).float().mean())
        if s != em.CORR_BIG:
            print('%s %s: fp32 spellings differ in %.1f %%, their 16-bit roundings in %.3f %%' % (em.DTYPE_NAMES[dtype], s, 100 * differ32, 100 * differ16))
        assert differ16 <= 0.001, (s, differ16)
        if C & (C - 1) == 0:
            assert differ32 == 0.0 and torch.equal(qd.double() * C, S), s
            ties += int(em.is_tie(qd, dtype).sum())
            pow2 += S.numel()
        rounded += int(em.needs_rounding(qd, dtype).sum())
        total += S.numel()
    for s in em.CORR_BWD:
        for G in em.corr_grad_case(s, dtype)[3:]:
            q = em.corr_quotients(G, s[1])
            assert float((q[0].to(dtype) != q[1].to(dtype)).float().mean()) <= 0.001, s
            grounded += int(em.needs_rounding(q[0], dtype).sum())
            gtotal += G.numel()
    print('%s: %.1f %% ties over power-of-two C, %.1f %% of outputs and %.1f %% of gradients need rounding'
          % (em.DTYPE_NAMES[dtype], 100.0 * ties / pow2, 100.0 * rounded / total, 100.0 * grounded / gtotal))
    assert ties >= 0.01 * pow2 and rounded >= 0.05 * total and grounded >= 0.05 * gtotal
    for params in GENERAL_SETS:
        S = em.corr_general_case(tuple(params), dtype)[3]
        qd, qm = em.corr_quotients(S, params[1] * params[1] * em.CORR_GENERAL_SHAPE[1])
        assert float((qd.to(dtype) != qm.to(dtype)).float().mean()) <= 0.001, params


@pytest.mark.parametrize('dtype', DT)
def test_corr_autograd_cases_have_exact_zeros_and_whole_zero_channels(dtype):
    s = em.CORR_AUTOGRAD[0]
    f1, f2, gm, G1, G2 = em.corr_grad_case(s, dtype, em.SLOPE)
    S = em.corr_case(s, dtype)[3]
    assert s[2] == 4 and bool((S[:, :9] == 0).all()) and bool((S[:, 72:] == 0).all()) and bool((S[:, 9:72] != 0).any())
    go = em.corr_case(s, dtype)[2]
    assert torch.equal(gm[:, :9], go[:, :9] * em.SLOPE) and torch.equal(gm[S > 0], go[S > 0])          # zeros take the slope
    for s in em.CORR_FWD:                                                # the sign of the 16-bit output is the sign of the sum
        S = em.corr_case(s, dtype)[3]
        for q in em.corr_expected(S, s[1], 0.0, dtype):
            assert torch.equal(q == 0, S == 0), s


@pytest.mark.parametrize('dtype', DT)
def test_corr_nonfinite_references_are_what_they_claim(dtype):
    for s in em.CORR_NF_SHAPES:
        B, C, H, W = s
        for kind in em.CORR_NF_FWD:
            f1, f2, S, count = em.corr_nonfinite_fwd(s, dtype, kind)
            bad = ~torch.isfinite(S)
            assert int(bad.sum()) == count and count == {'in': 81, 'corner': 81 if kind[0] == 'f1' else 25}[kind[2]], (s, kind)
            assert int(bad.sum(1).max()) == (81 if kind[0] == 'f1' else 1)               # f2: at most one pixel per displacement channel
            if kind[0] == 'f1':
                assert int(bad.any(1).sum()) == 1                                       # one pixel, all its channels
                assert bool(torch.isnan(S).any()) or kind[2] == 'in'                    # the corner's padding zeros: inf * 0
    for s in em.CORR_NF_BWD_SHAPES:
        for kind in em.CORR_NF_BWD:
            f1, f2, go, G1, G2, n1, n2 = em.corr_nonfinite_bwd(s, dtype, kind)
            assert int((~torch.isfinite(G1)).sum()) == n1 == s[1], (s, kind)
            assert int((~torch.isfinite(G2)).sum()) == n2, (s, kind)
            assert n2 == (0 if kind[1] == 'edge_out' or (kind[1] == 'in' and s[3] == 3) else s[1]), (s, kind)
            if kind[1] == 'edge_out':
                assert bool(torch.isnan(G1[-1, :, 0, s[3] - 1]).all())                    # gO times the zero outside: NaN for inf too


def test_arena_block_is_contiguous_misaligned_and_watched():
    a = em.Arena(torch.float16, 'cpu', 1 << 16)
    x = a.block(2, 3, 5, 7, misalign=1, fill=torch.ones(2, 3, 5, 7))
    y = a.block(2, 115, 3, 5)
    assert x.is_contiguous() and x.data_ptr() % 16 == 2 and y.data_ptr() % 16 == 0 and bool((x == 1).all()) and bool(torch.isnan(y).all())
    for v in (x, y):
        off = v.storage_offset() - a.buf.storage_offset()
        assert bool(torch.isnan(a.buf[off - a.MARGIN:off]).all()) and bool(torch.isnan(a.buf[off + v.numel():off + v.numel() + a.MARGIN]).all())
    snap = a.snapshot()
    y[:, :81].fill_(1.0)
    assert a.untouched(snap, y[:, :81]) and not a.untouched(snap)
    y[1, 81, 0, 0] = 0.0                                                 # the first channel behind the output slice
    assert not a.untouched(snap, y[:, :81])
    b = em.Arena32('cpu', 1 << 15)
    z = b.block(1, 2, 3, 5, misalign=1)
    assert z.dtype == torch.float32 and z.data_ptr() % 16 == 4
    snap = b.snapshot()
    z.fill_(0.0)
    assert b.untouched(snap, z) and not b.untouched(snap)
    b.buf[z.storage_offset() + z.numel()] = 1.0
    assert not b.untouched(snap, z)


# ---- sampling: what tests/test_hip_warp_exact.py and tests/test_hip_resize_exact.py rest on -------------------------------------------
SDT = [pytest.param(d, id=em.SAMP_NAMES[d]) for d in em.SAMP_DTYPES]
WARP_GOLDEN = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'warp_*.npz')))


def shifts_of(B):
    return (0,) if B == 1 else (0, B // 2)


@pytest.mark.parametrize('name', WARP_GOLDEN)
def test_taps32_reproduces_the_golden_mask_bits_and_values(name):
    g = load_golden(name)
    x = g['x'].numpy()
    B, C, H, W = x.shape
    t = em.taps32(g['flow'].numpy(), H, W)
    assert np.array_equal(t['valid']['literal'], unpack_mask(g['mask'], (B, 1, H, W)).numpy()[:, 0])
    for mode, key in (('literal', 'y'), ('none', 'y_nomask')):
        ref, ra = em.warp_forward_ref(x, t, mode)
        assert bool(em.accept_y(g[key], ref, em.gamma(4) * ra, em.F32).all()), key


def test_rne_rounds_once():
    v = np.array([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 - 2.0 ** -30), 0.0, 3.0])
    assert em.rne(v, torch.bfloat16).double().tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6, -1.0, 0.0, 3.0]
    # through fp32 the first value would lose its sticky bits, land on the tie and go down
    assert float(torch.tensor(v[0]).float().to(torch.bfloat16)) == 1.0
    h = np.array([1.0 + 2.0 ** -11 + 2.0 ** -30, 1.0 + 2.0 ** -11])
    assert em.rne(h, torch.float16).double().tolist() == [1.0 + 2.0 ** -10, 1.0]


@pytest.mark.parametrize('mode', ['literal', 'robust', None])
def test_sampling_reference_agrees_with_the_fp64_autograd_of_the_oracle(mode):
    from oracle import ops as oops
    for shape, pattern in (((2, 3, 6, 20), 'rand4'), ((1, 5, 7, 13), 'const')):     # (smooth positions: the flow gradient jumps at integers)
        c = em.warp_case(shape, em.F32, pattern, False)
        B, C, H, W = shape
        t = em.taps32(c['flow'], H, W)
        m = mode or 'none'
        x64, f64, g64 = (torch.from_numpy(c[k]).double() for k in ('x', 'flow', 'gy'))
        y = oops.warp(x64, f64, mode)
        if mode == 'literal':                         # (the oracle's fp64 mask is not the fp32 contract: compare on the pixels where both agree)
            agree = torch.from_numpy(t['valid'][m])[:, None] == (oops.warp_mask(f64, H, W, mode))
        else:
            agree = torch.ones(B, 1, H, W, dtype=torch.bool)
        assert float(agree.float().mean()) > 0.9
        gxo, gfo = oops.warp_backward(x64, f64, g64 * agree, mode)
        ref, ra = em.warp_forward_ref(c['x'], t, m)
        # the model's weights are fp32 roundings of the fp64 ones: relative 2^-22 at most (three fp32 steps behind the position)
        tol = lambda a: 8 * em.U32 * a + 1e-12
        ag = agree.numpy()
        assert np.all((np.abs(y.numpy() - ref) <= tol(ra + 4 * np.abs(c['x']).max()))[np.broadcast_to(ag, ref.shape)])
        gx, gf, gfa = em.warp_backward_ref(c['x'], c['gy'] * ag, t, m)
        assert np.all(np.abs(gxo.numpy() - gx) <= tol(np.abs(gx) + 16 * np.abs(c['gy']).max()))
        assert np.all(np.abs(gfo.numpy() - gf) <= tol(gfa + 16 * C * np.abs(c['gy']).max() * np.abs(c['x']).max()))


@pytest.mark.parametrize('dtype', SDT)
def test_dyadic_sampling_cases_keep_their_guards_and_equal_the_plain_formula(dtype):
    """Every dyadic case: the guard (inside warp_case); the reference through taps32 equals the plain fp64 formula (taps64) exactly;
    the fixed-point model of gx equals the fp64 formula rounded once."""
    for shape in em.WARP_DYADIC + em.WARP_C8_DYADIC:
        B, C, H, W = shape
        for pattern in sorted(set(em.FWD_PATTERNS + em.BWD_PATTERNS)):
            c = em.warp_case(shape, dtype, pattern, True)
            t64 = em.taps64(c['flow'], H, W)
            for mode in em.MODES:
                for shift in shifts_of(B):
                    y, _ = em.warp_forward_ref(c['x'], c['t'], mode, shift)
                    y64, _ = em.warp_forward_ref(c['x'], t64, mode, shift)
                    assert np.array_equal(y, y64) and np.all(np.isfinite(y))
                    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)                 # exact in fp32
                    if pattern not in em.BWD_PATTERNS:
                        continue
                    gx, gf, gfa = em.warp_backward_ref(c['x'], c['gy'], c['t'], mode, shift)
                    gx64, gf64, _ = em.warp_backward_ref(c['x'], c['gy'], t64, mode, shift)
                    assert np.array_equal(gx, gx64) and np.array_equal(gf, gf64)
                    assert np.array_equal(gf.astype(np.float32).astype(np.float64), gf) and float(gfa.max()) * 8 * 64 < em.LIMIT
                    got, q = em.warp_gx_model(c['gy'], c['t'], mode, shift, dtype)
                    assert torch.equal(got, em.rne(gx, dtype)), (shape, pattern, mode, shift)
                    assert np.array_equal(q.astype(np.float64) / em.FIX, gx)
                    if pattern == 'nonfinite':
                        for n, _, i, j in em.nonfinite_places(B, H, W):
                            assert np.all(gf[n, :, i, j] == 0) and np.all(y[n, :, i, j] == 0)


@pytest.mark.parametrize('dtype', SDT)
def test_general_sampling_cases_rarely_have_two_candidates(dtype):
    shapes = em.WARP_GENERAL + em.WARP_C8_GENERAL + ([em.WARP_PXT4] if dtype == em.F32 else [])
    for shape in shapes:
        for pattern in em.FWD_PATTERNS:
            c = em.warp_case(shape, dtype, pattern, False)
            for mode in em.MODES:
                ref, ra = em.warp_forward_ref(c['x'], c['t'], mode)
                assert np.all(np.isfinite(ref))
                if dtype != em.F32:                   # (an fp32 output is held to the interval itself)
                    share = em.two_candidate_share(ref, em.gamma(4) * ra, dtype)
                    assert share <= 0.01, (shape, pattern, mode, share)
                if pattern == 'nonfinite':
                    for n, _, i, j in em.nonfinite_places(*c['flow'].shape[:1], *shape[2:]):
                        assert np.all(ref[n, :, i, j] == 0)


def test_backward_cases_hold_what_they_claim():
    """Counted on the model: the constant flow merges lane pairs (also across lanes 63 / 64 of a wave — never — and across row ends
    — never: counted inside), the converging flow collides, random flows put taps outside and make the masks reject pixels."""
    for shape in em.WARP_DYADIC + em.WARP_BWD_GENERAL:
        B, C, H, W = shape
        dy = shape in em.WARP_DYADIC
        for pattern in em.BWD_PATTERNS:
            t = em.warp_case(shape, em.F32, pattern, dy)['t']
            for mode in em.MODES:
                n = em.warp_counts(t, mode, 0, B, H, W)
                big = H >= 5 and W >= 9
                if pattern == 'const' and W >= 9 and n['invalid'] < B * H * W // 2:      # (H == 1: 'robust' rejects every fy != 0)
                    assert n['merged'] > 0, (shape, mode, n)
                if pattern == 'converge' and H * W > 4:
                    assert n['collisions'] > 0, (shape, mode, n)
                if pattern == 'rand4' and big:
                    assert n['outside'] > 0 or mode != 'none', (shape, mode, n)
                    assert (n['invalid'] > 0) == (mode != 'none'), (shape, mode, n)
                if pattern == 'nonfinite':
                    assert n['invalid'] >= (0 if mode == 'none' else min(3, H * W)), (shape, mode, n)
    # the 65-wide cases cross lane 63 / 64 inside a row, every case crosses row ends: the merge must stay off there
    t = em.warp_case((1, 32, 9, 65), em.F32, 'const', True)['t']
    assert 0 < em.warp_counts(t, 'none', 0, 1, 9, 65)['merged'] < 2 * 9 * 65 - 2 * (9 * 65 // 64)


def test_every_warp_route_has_a_case():
    fwd = set()
    for dtype in em.SAMP_DTYPES:
        shapes = em.WARP_DYADIC + em.WARP_GENERAL + ([em.WARP_PXT4] if dtype == em.F32 else [])
        for B, C, H, W in shapes:
            fwd.add((em.SAMP_NAMES[dtype], em.warp_pxt(dtype, B, C, H, W)))
            fwd.add((em.SAMP_NAMES[dtype] + ' odd offset', em.warp_pxt(dtype, B, C, H, W, y_align=2 if dtype != em.F32 else 4)))
    assert {('bf16', 'narrow'), ('bf16', 'pxt2'), ('bf16', 'pxt1'), ('fp16', 'pxt2'), ('fp16', 'pxt1'), ('fp32', 'pxt1'), ('fp32', 'pxt4'),
            ('fp32', 'narrow'), ('fp32 odd offset', 'pxt1'), ('bf16 odd offset', 'pxt1')} <= fwd
    assert em.warp_pxt(em.F32, *em.WARP_PXT4) == 'pxt4' and em.warp_pxt(em.F32, *em.WARP_PXT4, y_align=4) == 'pxt1'
    B, C, H, W = em.WARP_PXT4
    assert em.warp_pxt(em.F32, B, C, H // 2, W) == 'pxt1'                    # the smallest grid that takes it
    # the pitched forms at odd W: a full pitch behind every row keeps the pair store, the admitted minimum (and one more) does not
    assert em.warp_pxt(torch.bfloat16, 2, 5, 7, 13, 16, 16, 5 * 7 * 16) == 'pxt2' and em.warp_pxt(torch.bfloat16, 1, 5, 7, 13, 16) == 'pxt2'
    assert em.warp_pxt(torch.bfloat16, 2, 5, 7, 13, 16, 16, 5 * 7 * 16 - 3) == 'pxt1' and em.warp_pxt(torch.bfloat16, 2, 5, 7, 13, 16, 16, 5 * 7 * 16 - 2) == 'pxt1'
    slices = {s: em.pick_cpt(s[0], s[1], s[2] * s[3]) for s in em.WARP_DYADIC + em.WARP_BWD_GENERAL}
    assert slices[(1, 32, 9, 65)] == (8, 4) and slices[(1, 33, 9, 65)] == (9, 4) and 33 % 9 != 0          # a short last slice
    assert slices[(2, 16, 13, 26)][1] == 2 and slices[(1, 3, 5, 9)][1] == 1


def test_every_resize_route_has_a_case():
    want = {'group1', 'group4', 'group16', 'group16_notable', 'wg', 'wg_notable', 'band', 'band_2bands', 'band_norowtable'}
    got = set()
    for name, (lo, hi) in em.RESIZE_BWD_ROUTES:
        for bc in em.RESIZE_BC:
            assert em.upsample_bwd_route(*lo, *hi, bc) == name, (name, lo, hi)
        got.add(name)
    assert got == want
    assert any(hi[1] == 1 for _, (lo, hi) in em.RESIZE_BWD_ROUTES) and any(lo[1] == 1 for _, (lo, hi) in em.RESIZE_BWD_ROUTES)
    # what the older tolerance test reaches (its comment once claimed the fallback loops)
    old = [((6, 20), (12, 40)), ((4, 13), (256, 832)), ((64, 208), (256, 832)), ((1, 3), (7, 9)), ((5, 1), (11, 6)), ((24, 40), (9, 15)), ((3, 5), (3, 5)),
           ((32, 104), (256, 832)), ((16, 52), (256, 832)), ((6, 5), (6, 200)), ((2, 3), (400, 12))]
    assert {em.upsample_bwd_route(*lo, *hi, 6) for lo, hi in old} <= {'group1', 'group4', 'band', 'band_2bands'}


def test_the_backward_range_brackets_every_weight_with_room_to_spare():
    """upsample_bwd_range is generous on purpose: no non-zero weight lies beyond ceil((a + 1) * inv) or below floor((a - 1) * inv) - 1,
    so its outermost `+ 1` is slack and a range without it computes the same sums (why no test can tell that variant apart)."""
    for n_in in list(range(2, 34)) + [52, 104]:
        for n_out in list(range(2, 131)) + [513, 832, 1025]:
            i0, i1, l0, l1 = em.lerp32(n_out, n_in)
            inv = np.float32(n_out - 1) / np.float32(n_in - 1)
            a = np.arange(n_in)
            hi = np.minimum(n_out - 1, np.ceil((a + 1).astype(np.float32) * inv).astype(np.int64))
            lo = np.maximum(0, np.floor((a - 1).astype(np.float32) * inv).astype(np.int64) - 1)
            j = np.arange(n_out)
            for idx, l in ((i0, l0), (i1, l1)):
                assert not np.any(((j > hi[idx]) | (j < lo[idx])) & (l != 0)), (n_in, n_out)
            for b in (0, n_in - 1):
                assert em._bwd_range(b, n_in, n_out)[0] <= lo[b] and em._bwd_range(b, n_in, n_out)[1] >= hi[b]


def test_dyadic_resize_cases_keep_their_guard_and_general_ones_are_general():
    for lo, hi in em.RESIZE_FWD_DYADIC + [c for _, c in em.RESIZE_BWD_ROUTES]:
        for bc in em.RESIZE_BC:
            x, gy = em.resize_case(lo, hi, bc, True)                          # (guards inside)
            for rate in (False, True):
                y, _ = em.resize_forward_ref(x, hi[0], hi[1], rate)
                gx, _, nnz = em.resize_backward_ref(gy, lo[0], lo[1], rate)
                assert np.all(np.isfinite(y)) and np.all(np.isfinite(gx)) and int(nnz.max()) >= 1
                if not rate:
                    assert np.array_equal(y.astype(np.float32).astype(np.float64), y) and np.array_equal(gx.astype(np.float32).astype(np.float64), gx)
    for lo, hi in em.RESIZE_FWD_GENERAL + em.RESIZE_BWD_GENERAL:
        assert not (em.is_dyadic_ratio(lo[0], hi[0]) and em.is_dyadic_ratio(lo[1], hi[1]))
    # the adjoint really is the adjoint of the forward: <resize(x), gy> == <x, adjoint(gy)> in fp64
    x, gy = em.resize_case((4, 13), (64, 208), 6, False)
    y, _ = em.resize_forward_ref(x, 64, 208, True)
    gx, _, _ = em.resize_backward_ref(gy, 4, 13, True)
    a, b = float((y * gy).sum()), float((gx * x).sum())
    assert abs(a - b) <= 1e-10 * max(1.0, abs(a))


# ---- normalisation, SGU blend, occlusion check, census (tests/test_hip_norm_exact.py, tests/test_hip_blend_exact.py) ---------------------
def _norm_routes():
    for name in em.NORM_CASES:
        for dtype in em.norm_dtypes(name):
            c = em.norm_case(name, dtype)
            yield name, dtype, c, em.normalize_route(c['N'], c['HW'], dtype, aligned=not c['misalign'])


def test_normalize_route_names_every_case():
    """normalize_route on the issue's table: the route each case was chosen for, and every (form, segmented, vec, ragged) combination
    the host code can produce (wave rows are never segmented; a ragged last segment has an odd-length row behind it, never vectors for
    16-bit types) has a case."""
    r = {(n, em.SAMP_NAMES[d]): route for n, d, _, route in _norm_routes()}
    assert r['hw2', 'bf16'] == ('wave', 1, 2, False) and r['hw63_9rows', 'fp16'] == ('wave', 1, 63, False)
    assert r['hw64', 'bf16'] == ('wave', 1, 64, True) and r['hw64_misaligned', 'bf16'] == ('wave', 1, 64, False)
    assert r['hw64', 'fp32'] == ('block', 1, 64, True) and r['hw64_misaligned', 'fp32'] == ('block', 1, 64, False)
    assert r['wave_limit', 'fp16'] == ('wave', 1, 4096, True) and r['block_4104', 'fp16'] == ('block', 1, 4104, True)
    assert r['seg2_2048', 'bf16'] == ('block', 2, 2048, True) and r['seg2_2048', 'fp32'] == ('block', 2, 2048, True)
    assert r['seg2_2052', 'fp32'] == ('block', 2, 2052, True) and r['seg2_2052', 'fp16'] == ('block', 2, 2052, False)
    assert r['seg2_ragged', 'bf16'] == ('block', 2, 2105, False) and 2 * 2105 > 61 * 69
    assert r['seg4_ragged', 'fp32'] == ('block', 4, 2071, False) and 91 * 91 - 3 * 2071 == 2068
    assert r['spike_wave', 'bf16'][0] == 'wave' and r['spike_block', 'fp16'] == ('block', 8, 3584, True)
    assert em.NORM_CASES['hw63_9rows'][0][0] * em.NORM_CASES['hw63_9rows'][0][1] == 9            # a second workgroup with one live wave
    assert max(c['N'] * c['HW'] for _, _, c, _ in _norm_routes()) == 2 * 256 * 57 * 72                   # 2.1 M elements: the largest operand
    # every combination the host code can produce over a sweep of sizes ...
    reach = set()
    for dtype in em.SAMP_DTYPES:
        for N in (1, 2, 3, 9, 64, 512, 600):
            for HW in list(range(1, 70)) + list(range(4090, 4110)) + list(range(4200, 4216)) + list(range(8270, 8290)) + [28672, 172800]:
                for aligned in (True, False):
                    form, nseg, seglen, vec = em.normalize_route(N, HW, dtype, aligned)
                    reach.add((dtype == em.F32, form, nseg > 1, vec, nseg * seglen != HW))
    have = {(d == em.F32, route[0], route[1] > 1, route[3], route[1] * route[2] != c['HW']) for _, d, c, route in _norm_routes()}
    assert have == reach, sorted(reach - have)


def norm_share_cap(route, dtype):
    """The cap on the share of elements of y with two 16-bit candidates: 1 %.  The bound of y is at least gamma_k (kappa |y| +
    E|x - K| / std) and an fp16 value has 2^-11 |y| ... 2^-10 |y| to its neighbour, so for segments of 2048 elements and more (k >= 18) the interval of the bound itself spans more than 1 % of fp16's spacing whatever the data: there the cap is the ceiling
    2 * 2^11 gamma_k (kappa + 2) of that ratio for |y| >= 1/2, and the bit-for-bit check of y against the returned statistics
    (tests/test_hip_norm_exact.py) is what keeps those values sharp."""
    k = em.norm_roundings(route, dtype)
    if dtype == torch.float16 and route[2] >= 2048:
        return lambda kappa: 2 * 2.0 ** 11 * em.gamma(k) * (kappa + 2.0)
    return lambda kappa: 0.01


def test_normalize_caps_and_spikes():
    for name, dtype, c, route in _norm_routes():
        ref = em.norm_forward_ref(c['x'], route, dtype)
        assert np.all(np.isfinite(ref['y'])) and np.all(ref['b_y'] >= 0)
        if c['spike']:
            assert ref['kappa'].min() > 1000 and ref['b_rstd'].max() < 0.05                # wide, as the pivot note says, and still a check
            continue
        assert ref['kappa'].max() < 100 if dtype != em.F32 else True
        if dtype != em.F32:
            share, cap = em.two_candidate_share(ref['y'], ref['b_y'], dtype), norm_share_cap(route, dtype)(float(ref['kappa'].max()))
            assert share <= cap, (name, em.SAMP_NAMES[dtype], share, cap)
            assert cap <= 0.01 or (dtype == torch.float16 and cap < 0.1)
    for HW in em.NORM_BWD_HW:
        for dtype in em.SAMP_DTYPES:
            y, gy, r = em.norm_bwd_case(HW, dtype)
            ref, bound = em.norm_backward_ref(y, gy, r)
            assert np.all(bound > 0) and np.all(np.isfinite(ref))
    assert 513 - em.NORM_NT == 1                                                          # one element in the second stride


def test_normalize_reference_notices_the_mutations():
    """Dropping the last element of a ragged segment, or merging with HW for HW - 1, moves the statistics by more than their bounds."""
    for name in ('seg2_ragged', 'seg4_ragged'):
        for dtype in em.SAMP_DTYPES:
            c = em.norm_case(name, dtype)
            route = em.normalize_route(c['N'], c['HW'], dtype)
            ref = em.norm_forward_ref(c['x'], route, dtype)
            x = c['x'].astype(np.float64)
            short = np.delete(x, c['HW'] - 1, axis=1)
            assert np.all(np.abs(short.mean(1) - ref['mean']) > ref['b_mean'])
            biased = 1.0 / np.sqrt(((x - ref['mean'][:, None]) ** 2).sum(1) / c['HW'] + em.NORM_EPS)
            assert np.all(np.abs(biased - ref['rstd']) / ref['rstd'] > ref['b_rstd'])


BLEND_COUNT_KEYS = ('merged', 'refused_lane63', 'refused_address', 'refused_row_end', 'collisions', 'left', 'right', 'top', 'bottom', 'past_hw')


@pytest.mark.parametrize('dtype', [pytest.param(d, id=em.SAMP_NAMES[d]) for d in em.BLEND_DTYPES])
def test_blend_cases_hold_their_guards_and_counts(dtype):
    """Every blend case builds (the dyadic and final-level guards run inside blend_case); per regime every count the backward claims
    is > 0; the wide cases have all of them at once; the final level's resize-gradient routes are named."""
    for regime, cases in (('dyadic', [(s, None) for s in em.BLEND_DYADIC]), ('general', [(s, None) for s in em.BLEND_GENERAL]),
                          ('final', [((2,) + hi, lo) for lo, hi in em.BLEND_FINAL])):
        total = dict.fromkeys(BLEND_COUNT_KEYS, 0)
        for shape, lo in cases:
            c = em.blend_case(shape, dtype, regime, lo)
            n = em.blend_counts(c['t'], *shape)
            for k in BLEND_COUNT_KEYS:
                total[k] += n[k]
            if shape[1] >= 9 and shape[2] > 64:
                assert all(n[k] > 0 for k in BLEND_COUNT_KEYS), (shape, n)
        assert all(total[k] > 0 for k in BLEND_COUNT_KEYS), (regime, total)
    assert em.blend_counts(em.blend_case((2, 9, 29), dtype, 'general')['t'], 2, 9, 29)['past_hw'] == 2 * 256 - 261
    routes = {em.upsample_bwd_route(lo[0], lo[1], hi[0], hi[1], 3 * 2) for lo, hi in em.BLEND_FINAL}
    assert routes == {'group4', 'band'}, routes
    for shape in em.BLEND_GENERAL:
        c = em.blend_case(shape, dtype, 'nonfinite')
        assert int((~np.isfinite(c['inter'])).sum()) == 2
        fu, b = em.blend_forward_ref(c['flow_init'], c['t'], c['m'])
        assert np.all(np.isfinite(fu)) and np.all(np.isfinite(b))                         # no NaN from an outside tap's weight


def test_blend_fixed_point_model_equals_the_fp64_adjoint_in_the_dyadic_regime():
    for dtype in em.BLEND_DTYPES:
        for shape in em.BLEND_DYADIC:
            c = em.blend_case(shape, dtype, 'dyadic')
            t64 = em.taps64(c['inter'], shape[1], shape[2])
            gx, _, _ = em.warp_backward_ref(c['flow_init'], c['g'] * (1.0 - c['m'])[:, None], t64, 'none')
            want = gx + c['m'][:, None] * c['g']
            assert np.array_equal(em.blend_ginit_model(c['g'], c['t'], c['m32']).astype(np.float64), want)
            assert set(np.unique(c['m'])) <= {0.0, 0.5, 1.0} and len(np.unique(c['m'])) == 3 or shape == (2, 2, 2)
            # a merge without the address comparison would move contributions: pairs that the comparison separates exist
            assert em.blend_counts(c['t'], *shape)['refused_address'] > 0 or shape == (2, 2, 2)


def test_occ_cases_counts_caps_and_the_nan_pixel():
    from oracle import ops as oracle_ops
    total = dict(consistent_in=0, inconsistent_in=0, outgoing=0, edge=0, nonfinite=0)
    nan_in_frame = 0
    for shape in em.OCC_DYADIC + em.OCC_GENERAL:
        dyadic = shape in em.OCC_DYADIC
        c = em.occ_case(shape, dyadic)
        ref = em.occ_ref(c['ff'], c['fb'], *em.OCC_ALPHA)
        n = em.occ_counts(c, ref)
        for k in total:
            total[k] += n[k]
        if shape[1] > 1 and shape[2] > 1:
            assert n['consistent_in'] > 0 and n['inconsistent_in'] > 0 and n['outgoing'] > 0 and n['edge'] > 0, (shape, n)
        assert dyadic or n['nonfinite'] == 3
        if not dyadic:
            b, ch, i, j = em.nonfinite_places(*shape)[0]                                 # the NaN flow: never consistent, output 0 while in frame
            assert np.isnan(c['ff'][b, ch, i, j]) and not ref[0][2][b, i, j] and ref[0][0][b, i, j] == (0.0 if ref[0][3][b, i, j] else 1.0)
            nan_in_frame += int(ref[0][3][b, i, j])
        for _, undecided, _, _ in ref:
            assert undecided.mean() <= 0.01, (shape, undecided.mean())
        # the oracle (torch, fp32) agrees with the step-by-step model wherever the comparison is decided — NaN flows included
        o1, o2 = oracle_ops.occ_check(torch.from_numpy(c['ff']), torch.from_numpy(c['fb']), *em.OCC_ALPHA)
        for o, (want, undecided, _, _) in zip((o1, o2), ref):
            assert np.array_equal(o.numpy()[:, 0][~undecided], want[~undecided]), shape
    assert all(v > 0 for v in total.values()) and nan_in_frame > 0, (total, nan_in_frame)
    # '<=' for '<' in the threshold would show: dyadic pixels sit exactly on it
    c = em.occ_case((2, 17, 65), True)
    ref = em.occ_ref(c['ff'], c['fb'], *em.OCC_ALPHA)
    assert sum(int(u.sum()) for _, u, _, _ in ref) > 0


def test_oracle_occ_check_keeps_a_nan_flow_in_the_frame():
    """utils/tools.py:663-667 starts from ones and zeroes px > W-1, px < 0, py > H-1, py < 0: a NaN position fails all four and stays in
    the frame; its comparison with the threshold is false, so the pixel's output is 0."""
    from oracle import ops as oracle_ops
    ff, fb = torch.zeros(1, 2, 4, 5), torch.zeros(1, 2, 4, 5)
    ff[0, 0, 1, 2] = float('nan')
    o1, o2 = oracle_ops.occ_check(ff, fb)
    assert float(o1[0, 0, 1, 2]) == 0.0 and float(o1.sum()) == 19.0 and float(o2[0, 0, 1, 2]) == 0.0
    ff[0, 0, 1, 2] = 10.0                                                                 # leaves the frame: outgoing, 1
    assert float(oracle_ops.occ_check(ff, fb)[0][0, 0, 1, 2]) == 1.0


def test_census_model_is_the_adjoint_and_its_cases_are_what_they_claim():
    for size in em.CENSUS_SIZES:
        H, W = size
        for R in em.CENSUS_R:
            for kind in em.CENSUS_KINDS:
                g1, g2, G = em.census_case(size, kind)
                assert g1.min() >= 0 and g1.max() <= 1 and g2.min() >= 0 and g2.max() <= 1
                ref = em.census_ref(g1, g2, G, R)
                a, b = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (g1, g2))
                pa, pb = F.pad(a, (R,) * 4), F.pad(b, (R,) * 4)
                d = 0
                for dy in range(2 * R + 1):
                    for dx in range(2 * R + 1):
                        u1, u2 = pa[:, dy:dy + H, dx:dx + W] - a, pb[:, dy:dy + H, dx:dx + W] - b
                        t = u1 / torch.sqrt(em.CENSUS_A + u1 * u1) - u2 / torch.sqrt(em.CENSUS_A + u2 * u2)
                        d = d + t * t / (em.CENSUS_B + t * t)
                ga, gb = torch.autograd.grad(d, (a, b), torch.tensor(G, dtype=torch.float64))
                assert np.allclose(d.detach().numpy(), ref['dist'], rtol=1e-12, atol=1e-14)
                assert np.allclose(ga.numpy(), ref['gg1'], rtol=1e-9, atol=1e-12) and np.allclose(gb.numpy(), ref['gg2'], rtol=1e-9, atol=1e-12)
                assert np.all(ref['b_dist'] <= 1e-4 * np.maximum(ref['dist'], 1e-3))       # the bounds stay a check: 1e-4 relative at most
                if kind == 'equal':
                    assert not ref['dist'].any() and not ref['gg1'].any() and not ref['gg2'].any()
                if kind == 'constant' and H > 2 * R and W > 2 * R:
                    assert np.all(g1[:, R:H - R, R:W - R] == g1[0, 0, 0])
                if kind == 'random' and min(H, W) > 1:
                    # the bound is a small fraction of the gradient: a missing family of terms (the neighbour role) cannot hide in it
                    assert np.abs(ref['gg1']).max() > 100 * ref['b_gg1'].max()
    assert 2 < 2 * min(em.CENSUS_R) + 1 and 17 * 65 > 256                                 # an image smaller than the window; two workgroups


# ---- the default loss path (tests/test_hip_loss_exact.py) ---------------------------------------------------------------------------------
def _msd_eval(name, B, masked, dtype):
    levels, y, occ = em.msd_case(name, B, masked)
    xs = [x.to(dtype).clone().requires_grad_(True) for x in levels]
    v = em.msd_ref(xs, y.to(dtype), None if occ is None else occ.to(dtype), em.MSD_WEIGHT)
    return v.detach(), torch.autograd.grad(v, xs)


def test_boundary_warp_cases_hold_the_guard_and_the_shares():
    """Every case is on its grids and below 2^24 quanta, the fp32 oracle equals the fp64 restatement bit for bit (output and autograd
    flow gradient), and the matrix is not vacuous: samples outside the frame, on integer coordinates, non-zero outputs."""
    from oracle import ops as oracle_ops
    for name in em.BWARP_CASES:
        c = em.bwarp_case(name)
        fwd, bwd, g = em.bwarp_guard(c)
        assert fwd < em.LIMIT and bwd < em.LIMIT
        out, gf = em.bwarp_expected(c)
        flow = c['flow'].clone().requires_grad_(True)
        o32 = oracle_ops.boundary_warp(c['image'], flow, c['start'])
        (g32,) = torch.autograd.grad(o32, flow, c['grad_out'])
        assert torch.equal(o32.detach(), out) and torch.equal(g32, gf), name
        if name in em.BWARP_SHARE_CASES:
            outside, integer, nonzero = em.bwarp_shares(c)
            print(name, 'outside %.2f, on an integer coordinate %.2f, non-zero outputs %.2f' % (outside, integer, nonzero))
            assert 0.2 <= outside <= 0.8 and integer >= 0.1 and nonzero >= 0.25, (name, outside, integer, nonzero)
            assert gf.abs().max() > 0
    B, C, Hi, Wi, h, w, _ = em.BWARP_SHAPES['far']
    assert h * w == 323 and h * w > em.LOSS_NT and h * w % em.LOSS_NT != 0                # two workgroups, the second ragged
    _, _, g = em.bwarp_guard(em.bwarp_case('far'))
    assert g['x'].min() < -1 and g['x'].max() > Wi and g['y'].min() < -1 and g['y'].max() > Hi          # far outside on all four sides
    c = em.bwarp_case('frame1')                                                           # a one-pixel frame: every corner clamps to it
    out, gf = em.bwarp_expected(c)
    assert not out.any() and not gf.any()
    c = em.bwarp_case('full')
    assert c['image'].shape[2:] == c['flow'].shape[2:]


def test_boundary_warp_hand_built_case_is_what_it_claims():
    c = em.bwarp_case('edges')
    Hi, Wi = em.BWARP_EDGES
    assert tuple(c['image'].shape[2:]) == (Hi, Wi)
    out, _ = em.bwarp_expected(c)
    _, _, g = em.bwarp_guard(c)
    w = c['flow'].shape[3]
    n = 0
    for kind, targets in em.bwarp_edge_targets(Hi, Wi).items():
        for tx, ty in targets:
            i, j = divmod(n, w)
            n += 1
            x, y = float(g['x'][0, i, j]), float(g['y'][0, i, j])
            assert (x, y) == (tx, ty), (kind, (tx, ty), (x, y))
            if kind == 'integer':
                assert x == round(x) and y == round(y)
            if kind == 'last':                                                            # both corners of one axis clamp to one pixel: weights cancel
                assert x == Wi - 1 or y == Hi - 1
                assert not out[0, :, i, j].any(), (tx, ty)
            if kind == 'before':
                assert -1 < x < 0 or -1 < y < 0
            if kind == 'after':
                assert Wi - 1 < x < Wi or Hi - 1 < y < Hi
    inside = [(2.0, 3.0), (5.0, 1.0)]                                                      # integer positions inside: the pixel itself
    for k, (tx, ty) in enumerate(em.bwarp_edge_targets(Hi, Wi)['integer']):
        if (tx, ty) in inside:
            i, j = divmod(k, w)
            assert torch.equal(out[0, :, i, j], c['image'][0, :, int(ty), int(tx)])


@pytest.mark.parametrize('i', range(3))
def test_bwarp_ref_in_fp64_matches_the_golden_fixtures(i):
    """fp64 arithmetic on the fixtures' operands as recorded, within the fixtures' own tolerances (1e-6 on the output, 1e-5 on the flow
    gradient).  The flow is handed over in the fp32 it was recorded in, so bwarp_ref forms the sample positions as the reference formed
    them — (grid + offset) + flow, rounded to fp32 — and runs everything after them in fp64: measured 5.3e-8 / 1.0e-7 / 2.0e-8 on the
    output, 2.4e-7 / 4.8e-7 / 6.0e-8 on the gradient.  With the flow promoted to fp64 first the positions are other numbers than the
    recorded ones (up to 55.9 in fixture 0: half an fp32 ulp is 1.9e-6 of a pixel), and the same comparison gives 1.7e-6 / 8.4e-7 /
    1.1e-7 and 5.7e-6 / 2.8e-6 / 8.2e-8 (printed; the exact cases of the GPU file sit on grids where the two positions coincide)."""
    g = load_golden('bwarp_%d' % i)
    flow = g['flow'].clone().requires_grad_(True)
    out, geo = em.bwarp_ref(g['image'].double(), flow, g['start'])
    assert out.dtype == torch.float64 and geo['x'].dtype == torch.float64
    e_out = float((out.detach() - g['out'].double()).abs().max())
    (gf,) = torch.autograd.grad(out, flow, g['grad_out'].double())
    e_gf = float((gf.double() - g['gflow'].double()).abs().max())
    flow64 = g['flow'].double().clone().requires_grad_(True)
    out64, _ = em.bwarp_ref(g['image'].double(), flow64, g['start'].double())
    (gf64,) = torch.autograd.grad(out64, flow64, g['grad_out'].double())
    print('bwarp_%d: fp64 arithmetic on the recorded positions: output %.3g, gradient %.3g; positions in fp64 too: %.3g, %.3g'
          % (i, e_out, e_gf, float((out64.detach() - g['out'].double()).abs().max()), float((gf64 - g['gflow'].double()).abs().max())))
    assert e_out <= 1e-6 and e_gf <= 1e-5


@pytest.mark.parametrize('i', range(3))
def test_bwarp_ref_in_fp32_gives_the_golden_fixtures_bits(i):
    g = load_golden('bwarp_%d' % i)
    flow = g['flow'].clone().requires_grad_(True)
    out, _ = em.bwarp_ref(g['image'], flow, g['start'])
    (gf,) = torch.autograd.grad(out, flow, g['grad_out'])
    assert out.dtype == torch.float32 and torch.equal(out.detach(), g['out']) and torch.equal(gf, g['gflow'])


def test_smooth1_exact_cases_partials_and_totals():
    from oracle import ops as oracle_ops
    assert em.SMOOTH1_SHAPES[-1][2] * em.SMOOTH1_SHAPES[-1][3] == em.LOSS_MAX_BLOCKS * em.LOSS_NT + 1
    assert [em.red_blocks(n) for n in (1, 256, 257, 262144, 262145, 10 ** 7)] == [1, 1, 2, 1024, 1024, 1024]
    for shape in em.SMOOTH1_SHAPES:
        B, Ci, H, W = shape
        c = em.smooth1_exact_case(shape)
        assert c['nblocks'] == em.red_blocks(B * H * W) and tuple(c['partials'].shape) == (c['nblocks'], 2)
        assert (c['img'] == c['img'][:, :, :1, :1]).all() and len(set(c['img'][:, :, 0, 0].reshape(-1).tolist())) == B * Ci
        assert max(c['total']) / em.SMOOTH1_GRID[0] < em.LIMIT
        assert tuple(c['partials'].sum(0).tolist()) == c['total'] and c['total'][0] > 0 and c['total'][1] > 0
        assert torch.equal(c['partials'].float().double(), c['partials'])
        assert (c['partials'].sum(1) > 0).all()                                              # every workgroup has work
        v = oracle_ops.smooth_edge1(c['img'].double(), c['pred'].double())                 # exp(-0) = 1: the mean of the differences
        want = c['total'][0] / (B * 2 * (H - 1) * W) + c['total'][1] / (B * 2 * H * (W - 1))
        assert abs(float(v) - want) <= 1e-12 * want
    # the last pixel of the largest shape is the second element of workgroup 0's first thread; it has no lower or right neighbour
    c = em.smooth1_exact_case(em.SMOOTH1_SHAPES[-1])
    assert c['nblocks'] == em.LOSS_MAX_BLOCKS


def test_msd_routes_are_the_named_ones():
    r = {n: em.msd_route(sizes, H, W) for n, ((H, W), sizes) in list(em.MSD_ROUTE_CASES.items()) + list(em.MSD_DYADIC_CASES.items())}
    assert all(v is not None and all(l['span'] <= em.MSD_BAND_COLS and l['NB'] >= 1 for l in v) for v in r.values())
    assert all(not l['row_table'] for l in r['no_row_table']) and all(l['row_table'] for n, v in r.items() if n != 'no_row_table' for l in v)
    assert len(r['six_levels']) == em.MSD_MAXL == len(r['dyadic_6']) and em.MSD_ROUTE_CASES['six_levels'][1][0][0] == 1        # a one-row level
    (H, W), sizes = em.MSD_ROUTE_CASES['ratio_limit']
    assert all((W - 1) / (w - 1) == em.MSD_RATIO_LIMIT for _, w in sizes) and all(l['NB'] == 1 and l['strips'] == 2 for l in r['ratio_limit'])
    assert [(l['NB'], l['strips']) for l in r['ragged_strips']] == [(64, 2), (64, 3), (64, 3)]
    assert all(w > 64 and w % 64 for _, w in em.MSD_ROUTE_CASES['ragged_strips'][1])
    assert [l['second_half'] for l in r['both_halves']] == [True] and r['both_halves'][0]['strips'] == 2
    assert not any(l['second_half'] for n, v in r.items() if n != 'both_halves' for l in v)
    # the entry point's refusals: a strip width of 0, a level narrower than 2, seven levels, a level larger than the label
    assert em.msd_route([(2, 2)], 6, 253) is not None and em.msd_route([(2, 2)], 6, 254) is None
    assert em.msd_route([(2, 1)], 6, 9) is None and em.msd_route([(2, 2)] * 7, 6, 9) is None and em.msd_route([(7, 2)], 6, 9) is None
    assert {(B, m) for _, B, m in em.msd_cases()} == {(1, True), (3, False)} and len(em.msd_cases()) == 14


def test_msd_reference_fp32_error_is_nonzero_and_capped():
    """The rule's right-hand side exists for every case (the fp32 composition differs from fp64), no route case's own fp32 gradient
    error passes MSD_TORCH32_CAP, and the rule can be met: the fp32 position chain alone (msd_chain_grads, shared bit for bit by torch's
    fp32 resize and the kernels) stays within the bound.  The dyadic cases sit on their grid, where the chain is exact."""
    for name, B, masked in em.msd_cases():
        levels, y, occ = em.msd_case(name, B, masked)
        assert (occ is not None) == masked and y.shape[0] == B and (occ is None or 0 < float(occ.mean()) < 1)
        (v32, g32), (v64, g64) = _msd_eval(name, B, masked, torch.float32), _msd_eval(name, B, masked, torch.float64)
        errs = [lv.relerr(a, b) for a, b in zip(g32, g64)]
        print(name, B, masked, 'value %.3g' % lv.relerr(v32, v64), 'gradients', ' '.join('%.3g' % e for e in errs))
        assert lv.relerr(v32, v64) > 0 and all(e > 0 for e in errs)
        assert max(errs) <= em.MSD_TORCH32_CAP, (name, B, masked, errs)
        assert all(float(g.abs().max()) > 0 for g in g64)
        chain = [lv.relerr(torch.from_numpy(c), b) for c, b in zip(em.msd_chain_grads(levels, y, occ, em.MSD_WEIGHT), g64)]
        bounds = [lv.bound(a, b) for a, b in zip(g32, g64)]
        print('    position chain alone', ' '.join('%.3g' % e for e in chain), ' bounds', ' '.join('%.3g' % e for e in bounds))
        assert all(e <= b for e, b in zip(chain, bounds)), (name, B, masked, chain, bounds)
        if name in em.MSD_DYADIC_CASES:
            assert all(em.on_grid(t, em.RESIZE_GRID[0]) and float(t.abs().max()) <= em.RESIZE_GRID[1] for t in levels + [y])
            assert max(errs) <= 1e-5 and max(chain) <= 1e-12                               # exact positions: a small bound
    assert set(em.MSD_REDRAWN) <= {c for c in em.msd_cases() if c[0] in em.MSD_ROUTE_CASES}


# ---- the split-precision fp32 convolutions (tests/test_hip_conv_x3_exact.py) ----------------------------------------------------------
# Guards (a) lossless split, (b) < 2^24 quanta of absolute terms and (c) a reference exact in fp32 are asserted INSIDE the *_case
# functions of _exact_model (x3_products / guard / x3_exact32): building a case is running them.  Guard (d), the planted zeros and the
# model-equals-truth cases are asserted here; the GPU file repeats (d) on the operands it runs.
import math

import _x3_model as xm


def _log2(v):
    return math.log2(v) if v > 0 else float('-inf')


def test_x3_forward_cases_hold_their_guards():
    top, share = 0.0, 1.0
    for layer in em.X3_FWD + [em.X3_TWO]:
        for zeros in (True, False):
            _, o, ref = em.x3_forward_case(layer.name, zeros)
            assert ref['top'] < em.LIMIT and ref['share'] > 0.5, (layer.name, ref['top'], ref['share'])
            assert not ref['nolo'] and not ref['plain']                  # (the dropped lo * lo product is really there)
            assert bool((ref['pre'] == 0).any()) == zeros, (layer.name, zeros)
            # every non-zero operand half the kernel multiplies: x's low halves are non-zero on more than a third of the elements
            lo = xm.split(o['x'])[1]
            assert float((lo != 0).double().mean()) > 1.0 / 3 or layer.H * layer.W <= 6
            top, share = max(top, ref['top']), min(share, ref['share'])
    print('x3 forward: largest sum of |terms| = 2^%.2f quanta, smallest cross-product share %.2f' % (_log2(top), share))
    # the cases of the route list really reach their routes' conditions (upf_conv_x3_forward)
    assert {(l.k, min(l.d, 16) if l.s == 1 else 0) for l in em.X3_FWD if em.x3_splitk_eligible(l)} >= {(3, 1), (3, 2), (3, 4), (3, 8), (3, 16), (1, 1)}
    assert {(l.k, l.d, l.s) for l in em.X3_FWD} >= {(3, 1, 1), (3, 2, 1), (3, 4, 1), (3, 8, 1), (3, 16, 1), (3, 1, 2), (1, 1, 1)}
    for d in (8, 16):
        hs = [l.H for l in em.X3_FWD if l.d == d]
        assert min(hs) < d < max(hs)


def test_x3_model_is_the_plain_fp64_convolution_where_no_pair_has_two_low_halves():
    """x's low halves on even channels, w's on odd (ci, co): each cross product can be non-zero in at most half of the output
    channels' terms, so guard (d) here asks for a quarter, not a half."""
    for name in em.X3_PLAIN:
        layer, o, ref = em.x3_forward_case(name, True, 'disjoint')
        assert ref['nolo'] and ref['plain'] and ref['share'] > 0.25, (name, ref['share'])
        assert bool((xm.split(o['x'])[1] != 0).any()) and bool((xm.split(em.x3_scaled_w(o['w'])[0])[1] != 0).any())
    for name in em.X3_TRAIN_PLAIN:
        layer, o, ref = em.x3_train_case(name, em.SLOPE, 'disjoint')
        truth = em.layer_ref(o['x'], o['w'], o['b'], o['gy'], layer.k, layer.d, layer.s, em.SLOPE)
        assert ref['plain'] and torch.equal(ref['y'], truth['y']) and torch.equal(ref['gx'], truth['gx']) and torch.equal(ref['gb'], truth['gb'])
        assert torch.equal(ref['ag']['gpre'].double(), truth['gpre'])
    for conv, n in em.X3_WG_CASES:
        Cin, Cout, k, d, s = em.X3_WG_CONVS[conv]
        levels, ref = em.x3_wgrad_case(conv, n, True, 'levels')
        assert ref['nolo'] and ref['share'] > 0.5, (conv, n, ref['share'])
        assert torch.equal(ref['gw'], em.wgrad_ref([(x, ag['gpre']) for x, _, _, ag in levels], (Cout, Cin, k, k), d, s))
        assert torch.equal(ref['gb'], sum(ag['gpre'].double().sum((0, 2, 3)) for _, _, _, ag in levels))
    # the stride-2 data gradient (a plain fp32 kernel): the model there is the plain fp64 gradient by construction
    for layer in em.X3_DGRAD:
        if layer.s == 2:
            _, o, ag, ref = em.x3_dgrad_case(layer.name, em.SLOPE)
            assert torch.equal(ref['gx'], torch.nn.grad.conv2d_input(o['x'].shape, o['w'].double(), ag['gpre'].double(), **em.geom(3, 1, 2)))


def test_x3_torch_fp32_in_its_own_order_reproduces_the_reference():
    """Order independence without a GPU: torch's fp32 convolution of the halves, three products summed in fp32, the scaled bias
    added last (the kernels START at it), un-scaled — the reference's bits."""
    for name in ('x17', 'x243', 'x64d8', 'x16s2', 'x115p'):
        layer, o, ref = em.x3_forward_case(name, True)
        ws, scw = em.x3_scaled_w(o['w'])
        (xh, xl), (wh, wl) = xm.split(o['x']), xm.split(ws)
        g = em.geom(layer.k, layer.d, layer.s)
        acc = F.conv2d(xl.float(), wh.float(), None, **g) + F.conv2d(xh.float(), wl.float(), None, **g)
        acc = acc + F.conv2d(xh.float(), wh.float(), None, **g) + (o['b'] * scw).view(1, -1, 1, 1)
        assert torch.equal((acc / scw).double(), ref['pre']), name


def test_x3_scale_cases_are_the_same_case_times_a_power_of_two():
    for name in em.X3_SCALE:
        _, o, ref = em.x3_forward_case(name, True)
        for kx, kw in [(k, 0) for k in em.X3_X_POW2] + [(0, k) for k in em.X3_W_POW2]:
            _, ok, refk = em.x3_forward_case(name, True, 'all', kx, kw)
            assert torch.equal(ok['x'].double(), o['x'].double() * 2.0 ** kx) and torch.equal(ok['w'].double(), o['w'].double() * 2.0 ** kw)
            assert torch.equal(ok['b'].double(), o['b'].double() * 2.0 ** (kx + kw))
            assert torch.equal(refk['pre'], ref['pre'] * 2.0 ** (kx + kw)) and refk['top'] == ref['top']
            assert em.x3_scaled_w(ok['w'])[1] == em.x3_scaled_w(o['w'])[1] * 2.0 ** -kw
    lo = xm.split(em.x3_forward_case(em.X3_SCALE[0], True, 'all', -11, 0)[1]['x'])[1]
    assert float(lo.abs().max()) == 2.0 ** -24                           # the last fp16 subnormal
    assert float(em.x3_forward_case(em.X3_SCALE[0], True, 'all', 14, 0)[1]['x'].abs().max()) == 2.0 ** 15 + 2.0


def test_x3_split_breaks_where_the_issue_says_it_does():
    """A fine part of +-3 steps, or a fine part on a zero base, makes the fp16 high half fine-grained: guard (a)'s grid check refuses."""
    base = torch.tensor([1.0, 2.0, -1.0])
    em._x3_halves(base + em.X3_FINE, 1.0, 'one step')
    with pytest.raises(AssertionError):
        em._x3_halves(base + 5 * em.X3_FINE, 1.0, 'five steps')          # (past half an fp16 ulp of 1: hi is no longer the base)
    with pytest.raises(AssertionError):
        em._x3_halves(torch.tensor([em.X3_FINE]), 1.0, 'a step on a zero base')
    with pytest.raises(AssertionError):
        em._x3_halves(torch.randn(16), 2.0 ** -20, 'arbitrary fp32 values')


def test_x3_training_and_gradient_cases_hold_their_guards():
    tops, shares = {}, {}

    def note(op, top, share=None):
        tops[op] = max(tops.get(op, 0.0), top)
        if share is not None:
            shares[op] = min(shares.get(op, 1.0), share)

    for layer in em.X3_TRAIN:
        for slope in (em.SLOPE, 0.0):
            _, o, ref = em.x3_train_case(layer.name, slope)
            assert max(ref['tops'].values()) < em.LIMIT
            zeros = ref['pre'] == 0
            assert bool(zeros.any()) == bool(slope), layer.name
            if slope:                                 # the zeros take the slope in the forward AND in the mask of the gradient
                assert torch.equal(ref['ag']['gpre'].double()[zeros], o['gy'].double()[zeros] * slope) and bool((o['gy'][zeros] != 0).any())
            for n in ('y', 'gx', 'gw'):
                # stride 2: channel-disjoint low halves (each cross product in at most half of the terms) and a data gradient that
                # forms no cross products at all (the plain fp32 kernel)
                if layer.s == 1:
                    assert ref['shares'][n] > 0.5, (layer.name, n, ref['shares'][n])
                elif n != 'gx':
                    assert ref['shares'][n] > 0.25, (layer.name, n, ref['shares'][n])
                note('train ' + n, ref['tops'][n], ref['shares'][n] if layer.s == 1 else None)
            note('train gb', ref['tops']['gb'])
    for layer in em.X3_DGRAD:
        for slope in (0.0, em.SLOPE):
            if slope and layer.name in em.X3_DGRAD_PLAIN_ONLY:
                continue
            _, o, ag, ref = em.x3_dgrad_case(layer.name, slope)
            assert ref['top'] < em.LIMIT
            if layer.s == 1:
                assert ref['share'] > 0.5, (layer.name, ref['share'])
            note('dgrad s%d' % layer.s, ref['top'], ref['share'] if layer.s == 1 else None)
    assert {l.H % 2 for l in em.X3_DGRAD if l.s == 2} == {0, 1} and {l.W % 2 for l in em.X3_DGRAD if l.s == 2} == {0, 1}
    for conv, n in em.X3_WG_CASES + [em.X3_WG_ACT]:
        slope = em.SLOPE if (conv, n) == em.X3_WG_ACT else 0.0
        for scaled in (True, False):
            levels, ref = em.x3_wgrad_case(conv, n, scaled, 'all', slope)
            assert ref['top'] < em.LIMIT and ref['top_b'] < em.LIMIT and ref['share'] > 0.5, (conv, n, ref['share'])
            note('wgrad', ref['top'], ref['share'])
            note('wgrad bias', ref['top_b'])
            if slope:
                assert all(bool((y == 0).any()) and bool((y < 0).any()) for _, _, y, _ in levels)
            assert len(levels) == 1 or len({ag['sc'] for _, _, _, ag in levels}) > 1          # the levels' scales differ
    assert max(len(v) for v in em.X3_WG_LEVELS.values()) == 6            # MAXLV
    for shape in em.X3_ACT_SHAPES:
        gy, y = em.x3_act_case(shape)
        for pre in (None, y):
            ag = em.x3_act_grad_ref(gy, pre, em.SLOPE)
            note('act_grad bias runs', em.guard('bias runs', ag['gs'].double().abs().sum((0, 2, 3)), ag['ug'] * em.X3_FINE))
            assert ag['sc'] == xm.scale_of(ag['max']) and 2.0 ** 13 <= float(ag['gs'].abs().max()) < 2.0 ** 14
            assert torch.equal(em.x3_bias_runs(ag['gs']).sum(1), ag['gs'].double().sum((0, 2, 3)))
    for op in sorted(tops):
        print('x3 %s: largest sum of |terms| = 2^%.2f quanta%s' % (op, _log2(tops[op]), ', smallest cross-product share %.2f' % shares[op] if op in shares else ''))
