"""The 16-bit inference ingest without a GPU: a numpy model of ops.stack_frames_u8 / upf_frames_u8_stack16 — the fp32 table of
the host expression (tests/test_ingest_cpu.py: table), rounded to nearest-even to fp16 (numpy's astype) or bf16 (integer rounding
of the bit pattern), then look-ups, a reversed index for the flip, the two frame sets stacked along the batch, rows placed at a
pitch — against the host data path followed by torch's CPU cast, over all 3 x 256 operands.  That pins "table, then round" to
"ATen cast of the host tensor"; tests/test_hip_ingest16.py holds the kernel to the same bits."""
import numpy as np
import pytest
import torch

from test_ingest_cpu import table
from upflow_pytorch_amd.dataset.kitti_dataset import img_func

DTYPES = (torch.float16, torch.bfloat16)


def table16(dtype, normalize=True):
    """[3,256] uint16: the bits of the fp32 table rounded to nearest-even to `dtype`."""
    t = table(normalize)
    if dtype == torch.float16:
        return t.astype(np.float16).view(np.uint16)
    assert dtype == torch.bfloat16
    u = t.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def model_stack16(f1, f2, dtype, flip=None, normalize=True, pitch=None, fill=0):
    """numpy model of the operator: u8 [B,H,W,3] x 2 -> the uint16 bit patterns [2B,3,H,pitch] of X (pitch None: W); item n < B is
    frame n of f1, item n + B frame n of f2, both mirrored where flip[n] != 0; columns [W, pitch) keep `fill`."""
    f1, f2 = np.asarray(f1), np.asarray(f2)
    B, H, W, _ = f1.shape
    t = table16(dtype, normalize)
    out = np.full((2 * B, 3, H, W if pitch is None else pitch), fill, dtype=np.uint16)
    for s, f in enumerate((f1, f2)):
        for b in range(B):
            cols = np.arange(W - 1, -1, -1) if (flip is not None and int(flip[b]) != 0) else np.arange(W)
            for c in range(3):
                out[s * B + b, c, :, :W] = t[c][f[b][:, cols, c]]
    return out


def host_stack16(f1, f2, dtype, flip=None, normalize=True):
    """The oracle: the host data path (img_func + np_2_tensor), torch's CPU cast, torch.cat -> int16 view [2B,3,H,W]."""
    items = []
    for f in (f1, f2):
        for b in range(f.shape[0]):
            raw = img_func.get_process_img_only_img(np.asarray(f[b]), normalize=normalize,
                                                    if_horizontal_flip=flip is not None and bool(flip[b]))
            items.append(img_func.np_2_tensor(raw)[0])
    return torch.stack(items).to(dtype).view(torch.int16)


def every_operand():
    """[1,16,16,3] uint8: each channel holds every byte value once (channel c in another order)."""
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    return np.stack([v, v.T, v[::-1]], axis=-1)[None].copy()


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
def test_table_then_round_is_the_cast_of_the_host_tensor_for_every_operand(dtype, normalize):
    f1 = every_operand()
    f2 = f1[:, ::-1].copy()
    for c in range(3):
        assert sorted(f1[0, :, :, c].ravel().tolist()) == list(range(256))
    got = model_stack16(f1, f2, dtype, normalize=normalize)
    want = host_stack16(f1, f2, dtype, normalize=normalize)
    assert got.shape == (2, 3, 16, 16) and np.array_equal(got.view(np.int16), want.numpy())
    # the rounding is not a truncation: it moves some operand up
    if normalize:
        trunc = (table(True).view(np.uint32) >> 16).astype(np.uint16)
        assert dtype != torch.bfloat16 or (table16(dtype) != trunc).any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_stacking_flip_and_pitched_placement(dtype):
    g = np.random.default_rng(3)
    B, H, W, pitch = 3, 11, 13, 16
    f1 = g.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    f2 = g.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    flip = np.array([1, 0, 2])
    want = host_stack16(f1, f2, dtype, flip=flip).numpy()
    got = model_stack16(f1, f2, dtype, flip=flip, pitch=pitch, fill=0x5a5a)
    assert got.shape == (2 * B, 3, H, pitch)
    assert np.array_equal(got[..., :W].view(np.int16), want)
    assert (got[..., W:] == 0x5a5a).all()
    assert np.array_equal(model_stack16(f1, f2, dtype, flip=flip).view(np.int16), want)
    # item n + B is frame n of the SECOND set; a flipped item is the mirror image of the unflipped one
    plain = model_stack16(f1, f2, dtype)
    assert np.array_equal(plain[B:], model_stack16(f2, f1, dtype)[:B])
    assert np.array_equal(got[0, :, :, :W], plain[0, :, :, ::-1]) and np.array_equal(got[1, :, :, :W], plain[1])


def test_bf16_ties_round_to_even():
    """The integer rounding on the bit pattern against torch, on exact ties and their neighbours."""
    u = np.array([0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0xbf808000, 0xbf818000, 0x00000000, 0x42ff8000], dtype=np.uint32)
    r = ((u.astype(np.uint64) + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    want = torch.from_numpy(u.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(r, want) and r[0] == 0x3f80 and r[1] == 0x3f82


def test_cpu_frames_raise_and_the_network_refuses_both_key_sets():
    from upflow_pytorch_amd import ops
    from upflow_pytorch_amd._lib import UpflowHipError
    from upflow_pytorch_amd.model.upflow import UPFlow_net
    f = torch.zeros(1, 16, 24, 3, dtype=torch.uint8)
    with pytest.raises(UpflowHipError):
        ops.stack_frames_u8(f, f, torch.bfloat16)                       # no CPU path
    with pytest.raises(UpflowHipError):
        ops.stack_frames_u8(f.float(), f.float(), torch.bfloat16)
    net = UPFlow_net.config()()
    with pytest.raises(ValueError):
        net({'im1': torch.zeros(1, 3, 16, 24), 'im2': torch.zeros(1, 3, 16, 24), 'frames1_u8': f, 'frames2_u8': f, 'if_loss': False})
