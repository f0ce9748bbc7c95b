"""Host side of gradient-norm clipping inside the step (no GPU): the coefficient of the contract's host model
(tests/_clip_model.py), the argument checks of NativeAdam(max_grad_norm=...) and Trainer(max_grad_norm=...), and the number of
fp64 partials a tensor list needs, from ops.mt_plan."""
import math

import numpy as np
import pytest
import torch

import _clip_model


def test_model_coefficient():
    one = np.float32(1.0)
    for norm in (0.0, 1e-3, 0.5, 25.6, 1e30):
        assert _clip_model.coef32(norm, math.inf) == one
    for max_norm in (1e-3, 1.0, 25.0, 1000.0):
        m = float(np.float32(max_norm))
        edge = np.float32(m - 1e-6)                          # the largest fp32 norm that is <= max_norm - 1e-6
        if float(edge) > m - 1e-6:
            edge = np.nextafter(edge, np.float32(0.0))
        for norm in (0.0, 0.5 * max_norm, float(edge)):
            assert float(np.float32(norm)) <= m - 1e-6
            assert _clip_model.coef32(norm, max_norm) == one, (norm, max_norm)
        for norm in (1.001 * max_norm, 2.0 * max_norm, 1e6 * max_norm):
            c = _clip_model.coef32(norm, max_norm)
            assert 0.0 < c < one, (norm, max_norm, c)
    # torch's formula at an ordinary point
    assert _clip_model.coef32(25.6, 1.0) == np.float32(1.0 / (np.float64(np.float32(25.6)) + 1e-6))
    assert _clip_model.coef32(2.0, 1.0) == np.float32(1.0 / (2.0 + 1e-6))


def test_model_norm_is_the_fp64_norm_of_the_unscaled_gradients():
    g = [np.array([3.0, 0.0], np.float32), np.array([4.0], np.float32)]
    assert _clip_model.norm64(g) == 5.0
    assert _clip_model.norm64([a * np.float32(65536.0) for a in g], 65536.0) == 5.0
    rnd = np.random.RandomState(3)
    a = rnd.randn(10001).astype(np.float32)
    assert abs(_clip_model.norm64([a]) - float(np.linalg.norm(a.astype(np.float64)))) <= 1e-12 * 100.0
    assert _clip_model.ulps32(np.float32(1.0) + np.float32(2.0 ** -23), 1.0) == 1.0


def _tiny_net():
    return torch.nn.Conv2d(1, 1, 1)


BAD = [0.0, -1.0, float('nan'), -math.inf, 'big', True, [1.0]]


@pytest.mark.parametrize('bad', BAD)
def test_parse_and_native_adam_reject_a_bad_bound(bad):
    from upflow_pytorch_amd.optim import NativeAdam, parse_max_grad_norm
    with pytest.raises(ValueError):
        parse_max_grad_norm(bad)
    with pytest.raises(ValueError):                         # (before the device is looked at)
        NativeAdam(_tiny_net().parameters(), lr=1e-4, max_grad_norm=bad)


def test_parse_accepts_none_positive_numbers_and_inf():
    from upflow_pytorch_amd.optim import parse_max_grad_norm
    assert parse_max_grad_norm(None) is None
    assert parse_max_grad_norm(1) == 1.0 and parse_max_grad_norm(0.25) == 0.25 and parse_max_grad_norm(math.inf) == math.inf
    assert parse_max_grad_norm(np.float32(2.0)) == 2.0


def test_native_adam_with_a_bound_has_no_cpu_path():
    from upflow_pytorch_amd.ops import UpflowHipError
    from upflow_pytorch_amd.optim import NativeAdam
    with pytest.raises(UpflowHipError):
        NativeAdam(_tiny_net().parameters(), lr=1e-4, max_grad_norm=1.0)


@pytest.mark.parametrize('bad', BAD)
def test_trainer_rejects_a_bad_bound(bad):
    from upflow_pytorch_amd.train import Trainer
    with pytest.raises(ValueError):
        Trainer(_tiny_net(), device='cpu', distributed=False, max_grad_norm=bad)


@pytest.mark.parametrize('kw', [dict(max_grad_norm=1.0), dict(max_grad_norm=math.inf), dict(max_grad_norm=1.0, device=None)])
def test_trainer_max_grad_norm_needs_a_gpu(kw):
    from upflow_pytorch_amd.ops import UpflowHipError
    from upflow_pytorch_amd.train import Trainer
    kw = dict(dict(device='cpu'), **kw)
    with pytest.raises(UpflowHipError):
        Trainer(_tiny_net(), distributed=False, **kw)


def test_trainer_default_is_what_it_was():
    from upflow_pytorch_amd.train import Trainer
    tr = Trainer(_tiny_net(), device='cpu', distributed=False)
    assert type(tr.optimizer) is torch.optim.Adam and tr.max_grad_norm is None and tr.loss_scale is None


def test_partial_count_is_the_number_of_chunks_over_several_launches():
    from upflow_pytorch_amd import ops
    C = ops.MT_CHUNK
    sizes = [1 + (i % 7) for i in range(60)] + [C - 1, C, C + 1, 65537, 0, 300 * C + 3, 3 * C, 7]
    want = sum((n + C - 1) // C for n in sizes)
    plan = ops.mt_plan(sizes)
    assert len(sizes) > ops.MT_TENSORS and want > ops.MT_BLOCKS and len(plan) >= 3
    assert sum(len(blocks) for _, blocks in plan) == want == ops.mt_partials(sizes)
    t = ops.MtTables(sizes)
    assert t.n_blocks == want and [L.n_blocks for L, _ in t.launches] == [len(b) for _, b in plan]


def test_clipped_launch_argument_block_stays_under_4_kb():
    import ctypes
    from upflow_pytorch_amd import _lib, ops
    table = ctypes.sizeof(_lib.MtLaunch)
    assert ops.mt_kernarg_bytes(clipped=True) == table + 4 * 8 + 5 * 8 == ops.mt_kernarg_bytes() + 8
    assert ops.mt_kernarg_bytes(clipped=True) <= ops.MT_KERNARG_LIMIT
