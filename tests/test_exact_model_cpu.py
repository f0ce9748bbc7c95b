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
