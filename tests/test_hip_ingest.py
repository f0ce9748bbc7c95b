"""upf_frames_u8_assemble on the GPU (csrc/ingest.hip; ops.frames_from_u8, ops.assemble_train_batch): bit equality with the host
data path — img_func.get_process_img_only_img + slicing, pinned on the reference by tests/test_data_eval_edge.py — at the shapes
where the addressing can go wrong, then through Trainer.step (the launch is captured with the step and reads aug from device
memory on every replay) and Test_model.eval_forward.  Comparisons are torch.equal on the int32 view of the fp32 tensors.
(The in-kernel clamp of an out-of-range device aug is reviewed by reading; the numpy model of tests/test_ingest_cpu.py states it.)"""
import numpy as np
import pytest
import torch

import _weights
from test_ingest_cpu import model_batch, model_frames
from upflow_pytorch_amd.dataset.kitti_dataset import img_func

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
KEYS = ('im1', 'im2', 'im1_raw', 'im2_raw', 'start')


def same_bits(got, want):
    want = want if torch.is_tensor(want) else torch.from_numpy(np.ascontiguousarray(want))
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and want.dtype == torch.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    return torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


def host_batch(f1, f2, aug, crop_size, normalize=True):
    """The oracle: the host data path itself (img_func + slicing + np_2_tensor), item by item."""
    ph, pw = crop_size
    out = {k: [] for k in KEYS}
    for b in range(f1.shape[0]):
        x, y, flip = (int(v) for v in aug[b])
        for k, f in (('im1', f1), ('im2', f2)):
            raw = img_func.get_process_img_only_img(f[b].numpy(), normalize=normalize, if_horizontal_flip=bool(flip))
            t_raw, t_crop = img_func.np_2_tensor(raw, raw[:, y:y + ph, x:x + pw])
            out[k + '_raw'].append(t_raw)
            out[k].append(t_crop)
        out['start'].append(img_func.np_2_tensor(np.array([x, y]).reshape(2, 1, 1))[0])
    return {k: torch.stack(v) for k, v in out.items()}


def frames(seed, B, H, W):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)


def check_batch(B, H, W, crop_size, aug, normalize=True, seed=0):
    from upflow_pytorch_amd import ops
    f1, f2 = frames(seed, B, H, W), frames(seed + 100, B, H, W)
    aug = torch.tensor(aug, dtype=torch.int32)
    want = host_batch(f1, f2, aug, crop_size, normalize)
    model = model_batch(f1.numpy(), f2.numpy(), aug.numpy(), crop_size, normalize)
    got = ops.assemble_train_batch(f1.to(DEV), f2.to(DEV), aug.to(DEV), crop_size, normalize=normalize)
    assert set(got) == set(KEYS) and tuple(got['start'].shape) == (B, 2, 1, 1)
    for k in KEYS:
        assert same_bits(torch.from_numpy(model[k]), want[k]), k        # (the numpy model is the host path)
        assert same_bits(got[k], want[k]), k
    # a CPU aug is checked on the host and uploaded: the same tensors
    got2 = ops.assemble_train_batch(f1.to(DEV), f2.to(DEV), aug, crop_size, normalize=normalize)
    assert all(torch.equal(got[k], got2[k]) for k in KEYS)
    return f1, f2, aug, got


def test_every_dword_phase_and_mixed_flips():
    """13-pixel rows are 39 bytes: the source rows start at every dword phase; 5x8 crops at the corners and inside, flips mixed."""
    H, W, ph, pw = 11, 13, 5, 8
    check_batch(3, H, W, (ph, pw), [(0, 0, 0), (W - pw, H - ph, 1), (3, 2, 1)])


def test_crop_equal_to_the_frame():
    _, _, _, got = check_batch(2, 11, 13, (11, 13), [(0, 0, 1), (0, 0, 0)], seed=1)
    assert torch.equal(got['im1'], got['im1_raw']) and torch.equal(got['im2'], got['im2_raw'])


def test_aligned_case():
    check_batch(2, 8, 16, (4, 8), [(4, 2, 0), (8, 4, 1)], seed=2)


@pytest.mark.parametrize('x,flip', [(409, 0), (410, 0), (409, 1), (410, 1)])
def test_long_rows_both_tail_phases(x, flip):
    """KITTI's row length (3726 bytes: the dword phase alternates row by row) and crop width; x = 409 / 410 put the crop's 16-byte
    groups in two different phases relative to the frame's, and 410 = W - pw ends the crop on the row's last pixel."""
    check_batch(1, 6, 1242, (4, 832), [(x, 1, flip)], seed=3)


def test_more_than_one_tile_per_row():
    """Rows longer than a workgroup's tile (1344 pixels): a 16-byte group that starts in one tile and ends in the next."""
    check_batch(1, 5, 1400, (3, 850), [(500, 1, 1)], seed=4)
    check_batch(1, 5, 2700, (3, 100), [(1300, 2, 0)], seed=5)


def test_unnormalised():
    check_batch(2, 11, 13, (5, 8), [(1, 1, 1), (5, 6, 0)], normalize=False, seed=6)


def test_frames_from_u8_with_and_without_flip_and_without_a_second_frame_set():
    """The crop-less mode with src2 null: [B,H,W,3] uint8 -> [B,3,H,W], also from a view that starts at an odd byte."""
    from upflow_pytorch_amd import ops
    B, H, W = 3, 7, 21
    f = frames(7, B, H, W)
    d = f.to(DEV)
    for normalize in (True, False):
        want = torch.stack([img_func.np_2_tensor(img_func.get_process_img_only_img(f[b].numpy(), normalize=normalize))[0] for b in range(B)])
        assert same_bits(ops.frames_from_u8(d, normalize=normalize), want)
    flip = torch.tensor([1, 0, 2], dtype=torch.int32)
    want = torch.stack([img_func.np_2_tensor(img_func.get_process_img_only_img(f[b].numpy(), if_horizontal_flip=bool(flip[b])))[0]
                        for b in range(B)])
    assert same_bits(torch.from_numpy(model_frames(f.numpy(), flip.numpy())), want)
    assert same_bits(ops.frames_from_u8(d, flip=flip.to(DEV)), want)
    tail = d[1:]                                     # contiguous, data pointer H*W*3 = 441 bytes into the allocation
    assert tail.is_contiguous() and tail.data_ptr() % 4 == 1
    assert same_bits(ops.frames_from_u8(tail), model_frames(f[1:].numpy()))


def test_second_call_on_another_stream_gives_the_same_bits():
    from upflow_pytorch_amd import ops
    f1, f2, aug, got = check_batch(2, 20, 45, (9, 31), [(14, 11, 1), (2, 3, 0)], seed=8)
    side = torch.cuda.Stream(device=DEV)
    a, b, c = f1.to(DEV), f2.to(DEV), aug.to(DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(side):
        again = ops.assemble_train_batch(a, b, c, (9, 31))
    side.synchronize()
    assert all(torch.equal(got[k], again[k]) for k in KEYS)


def test_rejected_arguments():
    from upflow_pytorch_amd import ops
    from upflow_pytorch_amd._lib import UpflowHipError
    f = frames(9, 2, 10, 12).to(DEV)
    aug = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.assemble_train_batch(f, f, aug, (11, 8))                    # taller than the frame
    with pytest.raises(UpflowHipError):
        ops.assemble_train_batch(f, f[:, :, :8], aug, (4, 8))           # second set of another shape
    with pytest.raises(UpflowHipError):
        ops.assemble_train_batch(f.permute(0, 2, 1, 3), f.permute(0, 2, 1, 3), aug, (4, 8))      # not contiguous
    with pytest.raises(UpflowHipError):
        ops.frames_from_u8(f.float())


# ---- the trainer -------------------------------------------------------------------------------------------------------------
FLAGS = {'if_norm_before_cost_volume': True, 'norm_moments_across_channels': False,
         'norm_moments_across_images': False, 'if_sgu_upsample': True, 'warp_mask_mode': 'robust'}
CROP, FRAME = (128, 192), (144, 208)
# five steps: 3 eager ones (the 3rd ends with the capture) + 2 replays, each with another aug
AUGS = [[(3, 9, 0), (16, 0, 1)], [(0, 16, 1), (11, 5, 1)], [(8, 8, 0), (1, 13, 0)], [(16, 16, 1), (5, 2, 0)], [(7, 0, 0), (12, 15, 1)]]


def smooth_u8_frames(B, H, W):
    """A textured pair with a 2-pixel motion, quantised to uint8 [B,H,W,3]."""
    im1, im2 = _weights.make_smooth_images(11, B, H, W)
    q = lambda im: ((im + 0.45) * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # noqa: E731
    return q(im1), q(im2)


def run_trainer(sd, batches):
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    from upflow_pytorch_amd.train import Trainer
    conf = UPFlow_net.config()
    d = dict(FLAGS)
    d.update(_weights.TRAIN_FLAGS)
    d['train_conv_dtype'] = 'bf16'
    conf.update(d, verbose=False)
    net = conf()
    net.load_state_dict(sd)
    tr = Trainer(net, lr=1e-4, device=DEV, distributed=False, graph=True)
    stats = [tr.step(b, sync_stats=False).clone() for b in batches]
    assert tr._graph is not None and not tr.capture_fallback, tr.capture_error
    torch.cuda.synchronize(DEV)
    return torch.stack(stats).cpu(), {n: p.detach().clone() for n, p in tr.raw_net.named_parameters()}


@pytest.fixture
def deterministic_aten_convolutions():
    """At 128x192 the two coarsest pyramid levels are below the native convolution kernels' sizes and take ATen's (MIOpen's)
    gradients, whose default solvers are not reproducible run to run: measured on MI355X without this setting, two trainers fed
    the SAME fp32 batches differ by up to 5.4e-2 in the loss (of 27) and 5.9e-4 in a parameter after these five steps (DESIGN
    §10).  MIOpen's deterministic mode removes that, for every trainer of the test alike; restored afterwards."""
    before = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before


def test_trainer_fed_uint8_batches_equals_trainer_fed_the_host_batches(deterministic_aten_convolutions):
    """Two fp32-fed trainers agree bit for bit under this schedule (asserted first); the uint8-fed trainer — whose captured step
    begins with the assemble launch and is replayed twice with NEW aug values in its static inputs — returns the same stats at
    every step and ends with the same parameters, bit for bit."""
    f1, f2 = smooth_u8_frames(2, *FRAME)
    augs = [torch.tensor(a, dtype=torch.int32) for a in AUGS]
    host = [{k: v.to(DEV) for k, v in host_batch(f1, f2, a, CROP).items()} for a in augs]
    u8 = [{'frames1_u8': f1.to(DEV), 'frames2_u8': f2.to(DEV), 'aug': a if i % 2 else a.to(DEV), 'crop_size': CROP}
          for i, a in enumerate(augs)]                 # (aug from the host and from the device, alternately)
    sd = _weights.make_state_dict(0, head_scale=0.1)
    s_a, p_a = run_trainer(sd, host)
    s_b, p_b = run_trainer(sd, host)
    s_c, p_c = run_trainer(sd, u8)
    spread = lambda u, v: max(float((u[n].double() - v[n].double()).abs().max()) for n in u)   # noqa: E731
    print('stats fp32-fed A:\n%s\nfp32-fed B - A:\n%s\nuint8-fed - A:\n%s' % (s_a, s_b - s_a, s_c - s_a))
    print('parameters: fp32-fed A vs B max |d| %.3g; uint8-fed vs A max |d| %.3g' % (spread(p_a, p_b), spread(p_a, p_c)))
    assert len({tuple(r.tolist()) for r in s_a}) == len(AUGS)
    assert torch.equal(s_a.view(torch.int32), s_b.view(torch.int32)) and all(torch.equal(p_a[n], p_b[n]) for n in p_a), \
        'two fp32-fed trainers differ: a finding about the existing step'
    assert torch.equal(s_a.view(torch.int32), s_c.view(torch.int32))
    assert all(torch.equal(p_a[n].view(torch.int32), p_c[n].view(torch.int32)) for n in p_a)


# ---- evaluation --------------------------------------------------------------------------------------------------------------
def test_eval_forward_takes_uint8_frames():
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    from upflow_pytorch_amd.test import Test_model
    conf = UPFlow_net.config()
    conf.update(FLAGS, verbose=False)
    sd = _weights.make_state_dict(0, head_scale=0.1)
    pairs8 = [smooth_u8_frames(1, 64, 128), tuple(reversed(smooth_u8_frames(1, 64, 128))), (frames(12, 1, 64, 128), frames(13, 1, 64, 128))]
    host = lambda f: img_func.np_2_tensor(img_func.get_process_img_only_img(f[0].numpy()))[0][None].to(DEV)   # noqa: E731
    pairs32 = [(host(a), host(b)) for a, b in pairs8]
    pairs8 = [(a.to(DEV), b.to(DEV)) for a, b in pairs8]
    for kw in (dict(graph=True), dict(graph=True, streams=2), dict(graph=False)):
        net = conf()
        net.load_state_dict(sd)
        tm = Test_model(net=net, dtype=torch.float32, device=DEV, **kw)
        want = [tm.eval_forward(a, b, 0) for a, b in pairs32]
        got = [tm.eval_forward(a, b, 0) for a, b in pairs8]
        for w, g in zip(want, got):
            assert tuple(g.shape) == (1, 2, 64, 128) and same_bits(g, w.cpu()), kw
        if kw.get('streams'):
            assert tm.pipe is not None
            streamed = list(tm.eval_forward_stream(iter(pairs8)))
            ref = list(tm.eval_forward_stream(iter(pairs32)))
            assert len(streamed) == len(ref) == 3
            for r, g in zip(ref, streamed):
                assert same_bits(g, r.cpu()), kw
