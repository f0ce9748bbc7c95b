"""bench.py's command line: `--full` and `--dump-outputs DIR` exist; the dump writes float32 arrays, sampled the same way every time
when they exceed the budget; (GPU) a plain run times exactly --steps steps, carries only the headline, and two runs with the same
arguments dump the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')
FULL_ONLY = ('roofline', 'roofline_conv', 'roofline_step', 'literal_split', 'one_step_in_flight', 'epe_vs_reference', 'cpu_baseline',
             'train_step')


def test_help_lists_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert '--full' in out.stdout and '--dump-outputs' in out.stdout


def test_dump_outputs_float32_exact_under_budget(tmp_path):
    import bench
    g = torch.Generator().manual_seed(0)
    outs = {'flow_f_out': torch.randn(2, 2, 8, 12, generator=g).bfloat16(), 'occ_fw': torch.rand(2, 1, 8, 12, generator=g),
            'photo_loss': None}
    bench.dump_outputs(outs, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ['flow_f_out.npy', 'occ_fw.npy']
    for k in ('flow_f_out', 'occ_fw'):
        a = np.load(tmp_path / (k + '.npy'))
        assert a.dtype == np.float32 and a.shape == tuple(outs[k].shape)
        assert np.array_equal(a, outs[k].float().numpy())


def test_dump_outputs_sample_is_bounded_and_fixed(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 64 << 10)
    g = torch.Generator().manual_seed(1)
    outs = {'a': torch.randn(4, 2, 64, 96, generator=g), 'b': torch.randn(4, 1, 64, 96, generator=g)}
    bench.dump_outputs(outs, str(tmp_path / 'x'))
    bench.dump_outputs(outs, str(tmp_path / 'y'))
    total = 0
    for k in outs:
        a, b = np.load(tmp_path / 'x' / (k + '.npy')), np.load(tmp_path / 'y' / (k + '.npy'))
        assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size < outs[k].numel()
        assert np.array_equal(a, b)
        assert np.isin(a, outs[k].numpy().reshape(-1)).all()
        total += a.nbytes
    assert total <= 64 << 10


@pytest.mark.gpu
def test_plain_run_steps_headline_and_repeatable_dump(tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR`, twice: exit 0, one line with the headline keys, exactly 3 timed
    steps in one window, none of the --full measurements, and the same four output arrays (flows, occlusion masks) bit for bit."""
    dumps = []
    for i in range(2):
        d = tmp_path / ('run%d' % i)
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(d)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
        assert all(k in line for k in HEADLINE)
        assert line['steps'] == 3 and line['windows'] == 1 and line['ms_per_step'] > 0 and line['value'] > 0
        assert not any(k in line for k in FULL_ONLY)
        assert sorted(os.listdir(d)) == ['flow_b_out.npy', 'flow_f_out.npy', 'occ_bw.npy', 'occ_fw.npy']
        arrs = {k: np.load(d / (k + '.npy')) for k in ('flow_f_out', 'flow_b_out', 'occ_fw', 'occ_bw')}
        assert arrs['flow_f_out'].dtype == np.float32 and arrs['flow_f_out'].shape == (4, 2, 384, 1280)
        assert all(np.isfinite(a).all() for a in arrs.values())
        dumps.append(arrs)
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
