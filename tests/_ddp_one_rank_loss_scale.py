"""Body of tests/test_hip_train_loss_scale.py::test_scaled_trainer_under_rccl_ddp_bucket_views, run as a script in its own process
(as tests/_ddp_one_rank.py is: the RCCL process group and its background threads stay out of the pytest process).  Prints
DDP-ONE-RANK-LOSS-SCALE-OK and exits 0 on success."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _weights                      # noqa: E402
from test_hip_train import build     # noqa: E402

LR = 1e-4


def step_until_applied(tr, batch):
    """Steps until one is applied -> its stats.  The dynamic scale starts at 2^16, which overflows on this vector: a skipped step changes
    no parameter and halves S, so the applied step runs on the initial weights (at most 16 halvings to the floor of 1)."""
    for i in range(18):
        stats = tr.step(batch)
        if stats['skipped_steps'] == i:
            return stats
        assert stats['skipped_steps'] == i + 1
    raise AssertionError('no step was applied: %r' % (stats,))


def main():
    import socket
    import torch.distributed as dist
    from upflow_pytorch_amd.optim import NativeAdam
    from upflow_pytorch_amd.train import Trainer
    assert not dist.is_initialized()
    dev = torch.device('cuda', 0)
    batch = {k: v.cuda() for k, v in _weights.make_train_batch().items()}
    plain = Trainer(build(), lr=LR, device=dev, distributed=False, loss_scale='dynamic')
    want = step_until_applied(plain, batch)
    want_g = {n: p.grad.detach().clone() for n, p in plain.raw_net.named_parameters()}
    want_p = {n: p.detach().clone() for n, p in plain.raw_net.named_parameters()}
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    saved = {k: os.environ.get(k) for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    try:
        dist.init_process_group(backend='nccl', rank=0, world_size=1)
        tr = Trainer(build(), lr=LR, device=dev, loss_scale='dynamic')
        assert tr.distributed and type(tr.net).__name__ == 'DistributedDataParallel' and isinstance(tr.optimizer, NativeAdam)
        got = step_until_applied(tr, tr.shard(batch))
        print('first applied step: S = %g after %d skipped steps (plain: %g, %d)' % (got['loss_scale'], got['skipped_steps'], want['loss_scale'], want['skipped_steps']))
        assert set(got) == set(want) and got['loss_scale'] == want['loss_scale'] and got['skipped_steps'] == want['skipped_steps']
        for k in want:
            assert abs(got[k] - want[k]) <= 1e-4 * max(1.0, abs(want[k])), (k, got[k], want[k])
        # the gradients the native step read are views into the reducer's bucket: 4-byte aligned, most of them not 16-byte aligned
        grads = [p.grad for p in tr.raw_net.parameters()]
        odd = sum(g.data_ptr() % 16 != 0 for g in grads)
        print('DDP bucket views: %d of %d gradients are not 16-byte aligned' % (odd, len(grads)))
        assert odd > 0
        # the same (scaled) gradients as the plain run, to the tolerance of tests/_ddp_one_rank.py ...
        gnorm = float(torch.cat([g.flatten() for g in want_g.values()]).norm())
        worst = 0.0
        for n, p in tr.raw_net.named_parameters():
            worst = max(worst, float((p.grad - want_g[n]).norm()) / max(float(want_g[n].norm()), 1e-3 * gnorm))
        print('DDP (1 rank, RCCL) vs plain scaled gradient: worst relative difference %.3g' % worst)
        assert worst <= 2e-3          # (MIOpen's backward kernels use atomics: not bit-reproducible run to run)
        # ... and the same parameters after the step, by the same measure; element by element the first Adam step moves a parameter
        # by at most lr, so two runs differ by at most 2 lr (where a near-zero gradient flips its sign)
        pnorm = float(torch.cat([v.flatten() for v in want_p.values()]).norm())
        worst_p = upd = dpar = 0.0
        init = dict(build().named_parameters())
        for n, p in tr.raw_net.named_parameters():
            d = (p.detach() - want_p[n]).abs()
            assert float(d.max()) <= 2.0 * LR * (1 + 1e-3), n
            worst_p = max(worst_p, float(d.norm()) / max(float(want_p[n].norm()), 1e-3 * pnorm))
            dpar += float(d.double().sum())
            upd += float((want_p[n] - init[n].detach()).abs().double().sum())
        print('parameters after one step, DDP vs plain: worst relative difference %.3g; summed difference / summed update %.3g'
              % (worst_p, dpar / upd))
        assert worst_p <= 2e-3
        # DDP + hipGraph: 11 eager warm-up steps, then the captured step (bucket all-reduce + check + Adam + scale update) replays
        trg = Trainer(build(), lr=LR, device=dev, graph=True, loss_scale='dynamic')
        hist = [trg.step(batch) for _ in range(trg.graph_warmup + 2)]
        sg = hist[-1]
        assert trg._graph is not None and not trg.capture_fallback
        # the two replayed steps are finite and were APPLIED (the scale settled during the warm-up, as in the eager run above)
        assert all(np.isfinite(v) for st in hist[-2:] for v in st.values())
        assert sg['skipped_steps'] == hist[-3]['skipped_steps'] == want['skipped_steps'] and sg['loss_scale'] == want['loss_scale']
        assert all(torch.isfinite(p).all() for p in trg.raw_net.parameters())
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


if __name__ == '__main__':
    main()
    print('DDP-ONE-RANK-LOSS-SCALE-OK')
