"""Host side of the device-resident optimizer step (no GPU): the multi-tensor launch planner of ops.mt_plan, the loss-scale
state machine the kernel implements (tests/_amp_model.py), and the argument checks of Trainer(loss_scale=...)."""
import ctypes
import random

import pytest
import torch

import _amp_model
import _weights


def _real_sizes():
    return [int(v.numel()) for k, v in _weights.make_state_dict(0).items()]


def _size_lists():
    from upflow_pytorch_amd import ops
    C = ops.MT_CHUNK
    rnd = random.Random(7)
    return {
        'tiny': [1, 2, 3],
        'chunk_edges': [C - 1, C, C + 1, 1, 2 * C - 1, 2 * C, 2 * C + 1],
        'issue_sizes': [1, 2, 3, 65535, 65536, 65537],
        'one': [1],
        'with_empty': [0, 5, 0, C + 1, 0],
        'two_hundred': [rnd.choice([1, 2, 3, 7, 33, 4097, C - 1, C, C + 1, 65537]) for _ in range(200)],
        'two_hundred_small': [1 + i % 5 for i in range(200)],
        # more chunks than one launch has workgroups: the tensor continues in the next launch, twice
        'longer_than_a_launch': [3, ops.MT_BLOCKS * C * 2 + 17, 5],
        'exact_launch': [ops.MT_BLOCKS * C],
        'real_network': _real_sizes(),
    }


@pytest.mark.parametrize('name', ['tiny', 'chunk_edges', 'issue_sizes', 'one', 'with_empty', 'two_hundred', 'two_hundred_small',
                                  'longer_than_a_launch', 'exact_launch', 'real_network'])
def test_planner_covers_every_element_exactly_once(name):
    from upflow_pytorch_amd import ops
    sizes = _size_lists()[name]
    if name == 'real_network':
        assert len(sizes) == 80 and min(sizes) == 2 and max(sizes) > 600000
    C = ops.MT_CHUNK
    covered = [[] for _ in sizes]                      # per tensor: the [lo, hi) ranges its workgroups take
    for tensors, blocks in ops.mt_plan(sizes):
        assert 0 < len(tensors) <= ops.MT_TENSORS and 0 < len(blocks) <= ops.MT_BLOCKS
        assert len(set(tensors)) == len(tensors)
        used = set()
        for slot, chunk in blocks:
            assert 0 <= slot < len(tensors)
            ti = tensors[slot]
            lo, hi = chunk * C, min((chunk + 1) * C, sizes[ti])
            assert 0 <= lo < hi <= sizes[ti], 'a workgroup must start inside its tensor'
            covered[ti].append((lo, hi))
            used.add(slot)
        assert used == set(range(len(tensors))), 'a tensor in the table without a workgroup'
    for ti, n in enumerate(sizes):
        ranges = sorted(covered[ti])
        assert sum(hi - lo for lo, hi in ranges) == n, (ti, n)
        pos = 0
        for lo, hi in ranges:                          # contiguous, no overlap, no gap
            assert lo == pos, (ti, ranges)
            pos = hi
        assert pos == n


def test_launch_argument_block_stays_under_4_kb():
    from upflow_pytorch_amd import _lib, ops
    assert ops.MT_KERNARG_LIMIT == 4096
    table = ctypes.sizeof(_lib.MtLaunch)
    # the table as the header declares it: five pointer lists, the sizes, the workgroup maps, two counts
    assert table >= 5 * 8 * ops.MT_TENSORS + 4 * ops.MT_TENSORS + 5 * ops.MT_BLOCKS + 8
    assert ops.mt_kernarg_bytes() == table + 4 * 8 + 4 * 8 <= ops.MT_KERNARG_LIMIT
    assert ops.MT_TENSORS <= 256                       # (block_tensor is a byte)
    # and the real network needs only a few launches
    assert len(ops.mt_plan(_real_sizes())) <= 4


def test_header_and_binding_agree_on_the_table():
    import os
    import re
    from conftest import ROOT
    from upflow_pytorch_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'upflow_hip.h')).read()
    for name, val in (('UPF_MT_TENSORS', _lib.MT_TENSORS), ('UPF_MT_BLOCKS', _lib.MT_BLOCKS), ('UPF_MT_CHUNK', _lib.MT_CHUNK)):
        assert int(re.search(r'#define %s (\d+)' % name, txt).group(1)) == val


def test_planner_rejects_what_the_kernels_cannot_index():
    from upflow_pytorch_amd import ops
    with pytest.raises(ops.UpflowHipError):
        ops.mt_plan([2 ** 31])
    with pytest.raises(ops.UpflowHipError):
        ops.mt_plan([-1])


def test_scale_state_machine_model():
    G, B = False, True
    # good, good, inf, good, good, good with growth_interval = 2
    assert _amp_model.run([G, G, B, G, G, G], growth_interval=2) == [
        (2.0 ** 16, 1, 0), (2.0 ** 17, 0, 0), (2.0 ** 16, 0, 1), (2.0 ** 16, 1, 1), (2.0 ** 17, 0, 1), (2.0 ** 17, 1, 1)]
    # an overflow resets the tracker: growth needs growth_interval CONSECUTIVE clean steps
    assert _amp_model.run([G, B, G, B, G, G], growth_interval=2)[-1] == (2.0 ** 15, 0, 2)
    # the floor at 1: S never goes below it, the steps are still skipped and counted
    assert _amp_model.run([B, B, B, B], scale=4.0, growth_interval=2) == [(2.0, 0, 1), (1.0, 0, 2), (1.0, 0, 3), (1.0, 0, 4)]
    # fixed scale: no growth, no backoff, the tracker stays put; skipped steps are counted
    assert _amp_model.run([G, G, B, G], scale=1024.0, growth_interval=2, dynamic=False) == [
        (1024.0, 0, 0), (1024.0, 0, 0), (1024.0, 0, 1), (1024.0, 0, 1)]
    m = _amp_model.ScaleModel(growth_interval=2)
    for bad in (G, B, G):
        m.update(bad)
    assert m.steps == 2                               # a skipped step does not advance Adam's step counter


def _tiny_net():
    return torch.nn.Conv2d(1, 1, 1)


def test_trainer_loss_scale_needs_a_gpu():
    from upflow_pytorch_amd.ops import UpflowHipError
    from upflow_pytorch_amd.train import Trainer
    with pytest.raises(UpflowHipError):
        Trainer(_tiny_net(), device='cpu', distributed=False, loss_scale='dynamic')
    with pytest.raises(UpflowHipError):
        Trainer(_tiny_net(), device='cpu', distributed=False, loss_scale=1024.0)
    # the default stays what it was: torch's Adam, no scale
    tr = Trainer(_tiny_net(), device='cpu', distributed=False)
    assert type(tr.optimizer) is torch.optim.Adam and tr.loss_scale is None and tr.skipped_steps is None


@pytest.mark.parametrize('bad', [3.0, 0.0, -2.0, float('inf'), float('nan'), 'static', 2.0 ** 16 + 1])
def test_trainer_rejects_a_loss_scale_that_is_no_power_of_two(bad):
    from upflow_pytorch_amd.train import Trainer
    with pytest.raises(ValueError):
        Trainer(_tiny_net(), device='cpu', distributed=False, loss_scale=bad)


def test_parse_loss_scale():
    from upflow_pytorch_amd.optim import parse_loss_scale
    assert parse_loss_scale('dynamic') == (2.0 ** 16, True)
    assert parse_loss_scale(1024) == (1024.0, False) and parse_loss_scale(0.5) == (0.5, False) and parse_loss_scale(1.0) == (1.0, False)


def test_native_adam_has_no_cpu_path():
    from upflow_pytorch_amd.ops import UpflowHipError
    from upflow_pytorch_amd.optim import NativeAdam
    with pytest.raises(UpflowHipError):
        NativeAdam(_tiny_net().parameters(), lr=1e-4)
