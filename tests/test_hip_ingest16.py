"""upf_frames_u8_stack16 on the GPU (csrc/ingest.hip; ops.stack_frames_u8): the stacked 16-bit network input straight from uint8
frames is, bit for bit, ops.frames_from_u8(...).to(dtype) of the two frame sets concatenated — at the shapes where the addressing
can go wrong, into fresh tensors and into views carved from a sentinel-filled buffer (nothing but the items' rows may change) —
and a network / runner / Test_model fed uint8 frames returns the flows of the same network fed the host-normalised fp32 tensors.
Comparisons are torch.equal on integer views."""
import numpy as np
import pytest
import torch

import _weights
from test_ingest16_cpu import model_stack16
from upflow_pytorch_amd.dataset.kitti_dataset import img_func

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
F16, BF16 = torch.float16, torch.bfloat16
MODES = [(F16, None), (BF16, None), (F16, BF16)]
SENTINEL = 0x5a5a


def frames(seed, B, H, W):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)


def bits16(t):
    assert t.dtype in (F16, BF16), t.dtype
    return t.contiguous().view(torch.int16)


def reference(d1, d2, dtype, flip=None, normalize=True):
    """What the operator replaces: two frames_from_u8 launches, ATen's casts, the stacking."""
    from upflow_pytorch_amd import ops
    return torch.cat([ops.frames_from_u8(d1, flip=flip, normalize=normalize).to(dtype),
                      ops.frames_from_u8(d2, flip=flip, normalize=normalize).to(dtype)], 0)


def carve(shape, dtype, pitch, offset, gap):
    """A [2B,3,H,W] view with rows `pitch` apart and items 3*H*pitch + gap apart, `offset` elements into a sentinel-filled buffer
    -> (view, buffer, mask of the elements the operator may write: the items' rows, padding columns included)."""
    n, c, H, W = shape
    item = c * H * pitch
    bs = item + gap
    base = torch.full((offset + n * bs + 11,), SENTINEL, dtype=torch.int16, device=DEV).view(dtype)
    view = base.as_strided(shape, (bs, H * pitch, pitch, 1), offset)
    allowed = torch.zeros(base.numel(), dtype=torch.bool, device=DEV)
    for i in range(n):
        allowed[offset + i * bs: offset + i * bs + item] = True
    return view, base, allowed


def check(B, H, W, pitched=True, flips=None, normalize=True, seed=0, src=None, model=True):
    """Every output mode, into fresh tensors and into carved ones (an odd element offset: every destination phase; an aligned one)."""
    from upflow_pytorch_amd import ops
    f1, f2 = src if src is not None else (frames(seed, B, H, W), frames(seed + 100, B, H, W))
    d1, d2 = (f1, f2) if f1.is_cuda else (f1.to(DEV), f2.to(DEV))
    flip = None if flips is None else torch.tensor(flips, dtype=torch.int32, device=DEV)
    want = {dt: bits16(reference(d1, d2, dt, flip, normalize)) for dt in (F16, BF16)}
    if model:                                            # (the numpy model of tests/test_ingest16_cpu.py is the same statement)
        for dt in (F16, BF16):
            m = model_stack16(d1.cpu().numpy(), d2.cpu().numpy(), dt, flip=flips, normalize=normalize)
            assert np.array_equal(m.view(np.int16), want[dt].cpu().numpy()), dt
    pitch = (W + 7) // 8 * 8 if pitched and W >= 8 else W
    for dtype, dec in MODES:
        got = ops.stack_frames_u8(d1, d2, dtype, dec, pitched=pitched, normalize=normalize, flip=flip)
        got = got if dec is not None else (got,)
        assert len(got) == (2 if dec is not None else 1)
        for t, dt in zip(got, (dtype, dec)):
            assert t.dtype == dt and tuple(t.shape) == (2 * B, 3, H, W) and ops.nchw_pitch(t) == pitch
            assert torch.equal(bits16(t), want[dt]), (dtype, dec, dt)
        for offset, gap in ((3, 5), (8, 16)):
            outs = [carve((2 * B, 3, H, W), dt, pitch, offset + k, gap + k) for k, dt in enumerate((dtype, dec)) if dt is not None]
            r = ops.stack_frames_u8(d1, d2, dtype, dec, pitched=pitched, normalize=normalize, flip=flip, out=outs[0][0],
                                    out_dec=outs[1][0] if dec is not None else None)
            assert (r[0] if dec is not None else r) is outs[0][0]
            for (view, base, allowed), dt in zip(outs, (dtype, dec)):
                assert torch.equal(bits16(view), want[dt]), (dtype, dec, dt, offset)
                untouched = base.view(torch.int16)[~allowed]
                assert bool((untouched == SENTINEL).all()), 'bytes before / between / after the items changed: %s' % ((dtype, dec, dt, offset),)
    return d1, d2, flip


def test_every_source_dword_phase_pitch_16_mixed_flips():
    """13-pixel rows are 39 bytes: the source rows start at every dword phase; the outputs are pitched to 16."""
    check(3, 11, 13, flips=[1, 0, 2])


def test_rows_shorter_than_eight_are_contiguous_and_ragged():
    """W < 8: ops.empty_nchw does not pitch, rows are 7 elements apart, every destination phase occurs."""
    check(2, 5, 7, flips=[0, 1], seed=1)


def test_aligned_case_holds_every_operand():
    from test_ingest16_cpu import every_operand
    f = torch.from_numpy(np.concatenate([every_operand(), every_operand()[:, :, ::-1]]).copy())
    assert tuple(f.shape) == (2, 16, 16, 3)
    check(2, 16, 16, src=(f, f.flip(1).contiguous()))
    check(2, 16, 16, src=(f, f.flip(1).contiguous()), normalize=False)
    check(2, 8, 16, flips=[1, 0], seed=2)


def test_contiguous_ragged_rows_at_a_width_that_would_be_pitched():
    check(2, 7, 21, pitched=False, flips=[0, 1], seed=3)


@pytest.mark.parametrize('flip', [0, 1])
def test_kitti_row_length_tail_group_ends_in_the_padding(flip):
    """W = 1242: 3726-byte source rows (the dword phase alternates), pitch 1248; unpitched: 2484-byte rows, a ragged last group."""
    check(1, 6, 1242, flips=[flip], seed=4, model=False)
    check(1, 6, 1242, pitched=False, flips=[flip], seed=4, model=False)


def test_more_than_one_tile_per_row():
    """Rows longer than a workgroup's tile (1344 pixels): groups that start in one tile and end in the next, both directions."""
    check(1, 5, 1400, flips=[1], seed=5, model=False)
    check(1, 5, 2700, flips=[0], seed=6, model=False)
    check(1, 5, 2700, pitched=False, flips=[1], seed=6, model=False)


def test_source_view_at_an_odd_byte():
    d = frames(7, 3, 7, 21).to(DEV)
    e = frames(8, 4, 7, 21).to(DEV)
    t1, t2 = d[1:], e[2:]
    assert t1.is_contiguous() and t1.data_ptr() % 4 == 1 and t2.data_ptr() % 4 == 2
    check(2, 7, 21, src=(t1, t2), flips=[1, 0])


def test_unnormalised():
    check(2, 11, 13, normalize=False, flips=[1, 0], seed=9)


def test_second_call_on_another_stream_gives_the_same_bits():
    from upflow_pytorch_amd import ops
    d1, d2, flip = check(2, 20, 45, flips=[1, 0], seed=10)
    first = ops.stack_frames_u8(d1, d2, F16, BF16, flip=flip)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(side):
        again = ops.stack_frames_u8(d1, d2, F16, BF16, flip=flip)
    side.synchronize()
    assert all(torch.equal(bits16(a), bits16(b)) for a, b in zip(first, again))


def test_float32_is_the_two_frames_from_u8_results_stacked():
    from upflow_pytorch_amd import ops
    d1, d2 = frames(11, 3, 11, 13).to(DEV), frames(12, 3, 11, 13).to(DEV)
    flip = torch.tensor([0, 1, 1], dtype=torch.int32, device=DEV)
    for fl in (None, flip):
        for normalize in (True, False):
            got = ops.stack_frames_u8(d1, d2, torch.float32, flip=fl, normalize=normalize)
            want = torch.cat([ops.frames_from_u8(d1, flip=fl, normalize=normalize), ops.frames_from_u8(d2, flip=fl, normalize=normalize)], 0)
            assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(ops.stack_frames_u8(d1, d2, torch.float32, torch.float32), ops.stack_frames_u8(d1, d2, torch.float32))


def test_rejected_arguments():
    from upflow_pytorch_amd import _lib, ops
    from upflow_pytorch_amd._lib import UpflowHipError
    B, H, W = 2, 10, 13
    f = frames(13, B, H, W).to(DEV)
    bad = [
        lambda: ops.stack_frames_u8(f.float(), f.float(), BF16),                                   # not uint8
        lambda: ops.stack_frames_u8(f[0], f[0], BF16),                                             # wrong rank
        lambda: ops.stack_frames_u8(f, f[:, :, :8].contiguous(), BF16),                            # mismatched frame sets
        lambda: ops.stack_frames_u8(f.permute(0, 2, 1, 3), f.permute(0, 2, 1, 3), BF16),           # not contiguous
        lambda: ops.stack_frames_u8(f, f, F16, torch.float32),                                     # an fp32 decoder beside a 16-bit pyramid
        lambda: ops.stack_frames_u8(f, f, torch.float32, BF16),
        lambda: ops.stack_frames_u8(f, f, torch.float64),
        lambda: ops.stack_frames_u8(f, f, BF16, flip=torch.zeros(B, dtype=torch.int64, device=DEV)),
        lambda: ops.stack_frames_u8(f, f, BF16, out=torch.empty(2 * B, 3, H, W, dtype=F16, device=DEV)),          # another type
        lambda: ops.stack_frames_u8(f, f, BF16, out=torch.empty(2 * B, 3, H, W + 1, dtype=BF16, device=DEV)),     # another shape
        lambda: ops.stack_frames_u8(f, f, BF16, out_dec=torch.empty(2 * B, 3, H, W, dtype=BF16, device=DEV)),     # no second type
        # a column crop of a wider LIVE buffer has a pitched tensor's strides, and its "padding" is somebody's data
        lambda: ops.stack_frames_u8(f, f, BF16, out=torch.empty(2 * B, 3, H, W + 19, dtype=BF16, device=DEV)[..., :W]),
        lambda: ops.stack_frames_u8(f, f, F16, BF16, out_dec=torch.empty(2 * B, 3, H, 32, dtype=BF16, device=DEV)[..., :W]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(UpflowHipError):
            call()
            pytest.fail('case %d was accepted' % i)
    # the entry point itself refuses a pitch ops.empty_nchw does not make, an fp32 output and an item larger than the batch stride
    x = torch.empty(2 * B, 3, H, 32, dtype=BF16, device=DEV)
    consts = ops._ingest_constants(True)
    for dtype, pitch, bs in ((_lib.UPF_BF16, W + 1, 3 * H * 32), (_lib.UPF_BF16, 32, 3 * H * 32), (_lib.UPF_F32, 16, 3 * H * 32),
                             (_lib.UPF_BF16, 16, 3 * H * 16 - 1)):
        with pytest.raises(UpflowHipError):
            _lib.launch(DEV, 'upf_frames_u8_stack16', _lib.ptr(f), _lib.ptr(f), None, _lib.ptr(x), dtype, pitch, bs, None, 0, 0, 0, B, H, W, *consts)
    torch.cuda.synchronize(DEV)


# ---- network, runners, evaluation ------------------------------------------------------------------------------------------------
FLAGS = {'if_norm_before_cost_volume': True, 'norm_moments_across_channels': False,
         'norm_moments_across_images': False, 'if_sgu_upsample': True, 'warp_mask_mode': 'robust'}
NET_MODES = {'fp16_pyramid_bf16_decoder': dict(dtype=BF16), 'fp16': dict(dtype=F16), 'bf16': dict(dtype=BF16, pyramid_dtype=None)}
SIZES = [(64, 128), (64, 512), (70, 522)]            # generic stacked schedule; fast in-buffer schedule (coarsest level 1x8); fast, pitched rows


def make_net(mode):
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    conf = UPFlow_net.config()
    conf.update(FLAGS, verbose=False)
    net = conf()
    net.load_state_dict(_weights.make_state_dict(0, head_scale=0.1))
    return net.to_inference(device=DEV, **NET_MODES[mode])


def u8_pairs(H, W):
    """A smooth pair with a 2-pixel motion and a noise pair, uint8 [1,H,W,3] on the host."""
    im1, im2 = _weights.make_smooth_images(11, 1, H, W)
    q = lambda im: ((im + 0.45) * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # noqa: E731
    return [(q(im1), q(im2)), (frames(21, 1, H, W), frames(22, 1, H, W))]


def host_fp32(f):
    return torch.stack([img_func.np_2_tensor(img_func.get_process_img_only_img(f[b].numpy()))[0] for b in range(f.shape[0])]).to(DEV)


def same_flow(got, want):
    assert got.dtype == torch.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    return torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


def test_the_sizes_take_the_schedules_they_are_meant_to():
    fpe = make_net('bf16').feature_pyramid_extractor
    assert fpe.out_shapes(64, 128)[-1][2] < 8 and fpe.out_shapes(64, 512)[-1][1:] == (1, 8) and fpe.out_shapes(70, 522)[-1][2] >= 8
    assert 522 % 8 and all(s[2] % 8 for s in fpe.out_shapes(70, 522)[:3])


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('mode', list(NET_MODES))
def test_flows_from_uint8_pairs_equal_flows_from_the_host_tensors(mode, size):
    from upflow_pytorch_amd.test import Test_model
    H, W = size
    pairs8 = u8_pairs(H, W)
    pairs32 = [(host_fp32(a), host_fp32(b)) for a, b in pairs8]
    pairs8 = [(a.to(DEV), b.to(DEV)) for a, b in pairs8]
    for kw in (dict(graph=True), dict(graph=True, streams=2), dict(graph=False)):
        tm = Test_model(net=make_net(mode), dtype=None, device=DEV, **kw)
        want = [tm.eval_forward(a, b, 0) for a, b in pairs32]
        got = [tm.eval_forward(a, b, 0) for a, b in pairs8]
        assert not same_flow(want[0], want[1])
        for w, g in zip(want, got):
            assert tuple(g.shape) == (1, 2, H, W) and same_flow(g, w), (mode, size, kw)
        if kw.get('graph'):
            assert {k[1] for k in tm.runner._runners} == {torch.float32, torch.uint8}       # (one captured runner per input type)
        if kw.get('streams'):
            assert tm.pipe is not None
            streamed = [g.clone() for g in tm.eval_forward_stream(iter(pairs8 + pairs8[::-1]))]
            assert len(streamed) == 4
            for g, w in zip(streamed, want + want[::-1]):
                assert same_flow(g, w), (mode, size, kw)


@pytest.mark.parametrize('mode', list(NET_MODES))
def test_one_ingest_launch_and_no_assemble_launch(mode, monkeypatch):
    from upflow_pytorch_amd import _lib
    net = make_net(mode)
    (a, b), _ = u8_pairs(64, 512)
    a, b = a.to(DEV), b.to(DEV)
    names = []
    real = _lib.launch

    def counting(device, name, *args):
        names.append(name)
        return real(device, name, *args)
    monkeypatch.setattr(_lib, 'launch', counting)
    with torch.no_grad():
        out = net({'frames1_u8': a, 'frames2_u8': b, 'if_loss': False})
    assert names.count('upf_frames_u8_stack16') == 1 and names[0] == 'upf_frames_u8_stack16'
    assert 'upf_frames_u8_assemble' not in names
    # the same forward fed the host-normalised fp32 tensors: no ingest launch, the same flows in both directions
    del names[:]
    with torch.no_grad():
        want = net({'im1': host_fp32(a.cpu()), 'im2': host_fp32(b.cpu()), 'if_loss': False})
    assert 'upf_frames_u8_stack16' not in names and same_flow(out['flow_f_out'], want['flow_f_out']) and same_flow(out['flow_b_out'], want['flow_b_out'])


def test_a_captured_uint8_runner_reads_its_static_uint8_buffers():
    from upflow_pytorch_amd.runtime import GraphedInference, PipelinedInference
    net = make_net('fp16_pyramid_bf16_decoder')
    H, W = 64, 512
    (a, b), (c, d) = u8_pairs(H, W)
    r8 = GraphedInference(net, 1, H, W, in_dtype=torch.uint8, device=DEV, warmup=1)
    r32 = GraphedInference(net, 1, H, W, device=DEV, warmup=1)
    assert r8.im1.dtype == torch.uint8 and tuple(r8.im1.shape) == (1, H, W, 3) and r8.im1.numel() * 4 == r32.im1.numel() * r32.im1.element_size()
    first = r8(a.to(DEV), b.to(DEV))['flow_f_out'].clone()
    assert same_flow(first, r32(host_fp32(a), host_fp32(b))['flow_f_out'])
    second = r8(c.to(DEV), d.to(DEV))['flow_f_out'].clone()          # a replay with new contents of the static inputs
    assert same_flow(second, r32(host_fp32(c), host_fp32(d))['flow_f_out']) and not same_flow(first, second)
    assert same_flow(r8(a.to(DEV), b.to(DEV))['flow_f_out'], first)
    pipe = PipelinedInference(net, 1, H, W, streams=2, in_dtype=torch.uint8, device=DEV, warmup=1)
    t1, t2 = pipe.submit(a.to(DEV), b.to(DEV)), pipe.submit(c.to(DEV), d.to(DEV))
    assert same_flow(pipe.result(t1)['flow_f_out'], first) and same_flow(pipe.result(t2)['flow_f_out'], second)


def test_fp32_network_fed_uint8_frames_under_grad_and_no_grad(monkeypatch):
    """The parity mode: upf_frames_u8_assemble writes the halves of the fp32 X, same flow bits.  With gradients enabled the frames
    are normalised first (one frames_from_u8 launch per frame set, no stacking launch) and the forward is the one fed fp32 tensors;
    that forward runs MIOpen's convolutions, which choose solvers by the workspace at hand and do not repeat bit for bit from
    call to call, so the routing is asserted on the launches and not on the flows (tests/test_hip_ingest.py pins frames_from_u8
    to the host tensors)."""
    from upflow_pytorch_amd import _lib
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    conf = UPFlow_net.config()
    conf.update(FLAGS, verbose=False)
    net = conf()
    net.load_state_dict(_weights.make_state_dict(0, head_scale=0.1))
    net = net.to(DEV).eval()
    (a, b), _ = u8_pairs(64, 128)
    u8 = {'frames1_u8': a.to(DEV), 'frames2_u8': b.to(DEV), 'if_loss': False}
    f32 = {'im1': host_fp32(a), 'im2': host_fp32(b), 'if_loss': False}
    with torch.no_grad():
        assert same_flow(net(u8)['flow_f_out'], net(f32)['flow_f_out'])
    names = []
    real = _lib.launch
    monkeypatch.setattr(_lib, 'launch', lambda device, name, *args: (names.append(name), real(device, name, *args))[1])
    got = net(u8)['flow_f_out']
    assert got.requires_grad and tuple(got.shape) == (1, 2, 64, 128) and bool(torch.isfinite(got).all())
    assert names.count('upf_frames_u8_assemble') == 2 and 'upf_frames_u8_stack16' not in names
    with pytest.raises(ValueError):
        net(dict(u8, **f32))
