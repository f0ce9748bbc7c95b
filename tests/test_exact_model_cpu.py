"""The conditions tests/test_hip_conv_exact.py rests on, checked on tests/_exact_model.py alone (no GPU, nothing from the code under
test): the guard holds for every case list, torch's fp32 kernels in their own summation order reproduce the fp64 reference bit for
bit (the order independence the GPU file relies on), the operands make enough outputs round / tie / hit zero for bit equality to
mean something, and the fp16 range cases are what they claim to be."""
import pytest
import torch
import torch.nn.functional as F

import _exact_model as em

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
