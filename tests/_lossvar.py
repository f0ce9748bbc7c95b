"""Shared by tests/golden/make_golden_loss_variants.py and the loss-variant tests: seeded inputs, the fixture cases and the
error rule (tests/test_hip_conv_x3_train.py's: error against fp64 over max |fp64| <= max(3e-6, 2.5 x the fp32 torch error))."""
import torch
import torch.nn.functional as F


def gen(seed):
    return torch.Generator().manual_seed(seed)


def textured(shape, seed):
    """A bilinear-smoothed random base plus 0.25 * uniform noise, in [0,1]."""
    B, C, H, W = shape
    g = gen(seed)
    base = torch.rand(B, C, max(2, H // 4 + 1), max(2, W // 4 + 1), generator=g)
    up = F.interpolate(base, size=(H, W), mode='bilinear', align_corners=True)
    return (0.75 * up + 0.25 * torch.rand(B, C, H, W, generator=g)).clamp(0, 1)


def ssim_inputs(shape, seed):
    """x textured, y = x + 0.1 N clipped to [0,1], binary weight [B,1,H,W]."""
    B, C, H, W = shape
    x = textured(shape, seed)
    g = gen(seed + 1000)
    y = (x + 0.1 * torch.randn(B, C, H, W, generator=g)).clamp(0, 1)
    w = (torch.rand(B, 1, H, W, generator=g) > 0.3).float()
    return x, y, w


def flow_inputs(shape, seed, scale=3.0):
    return scale * torch.randn(*shape, generator=gen(seed))


def piecewise_constant(shape, seed, block=4):
    """Constant on block x block cells: exact zero differences inside a cell (checks sign(0) = 0)."""
    B, C, H, W = shape
    base = torch.randint(-3, 4, (B, C, (H + block - 1) // block, (W + block - 1) // block), generator=gen(seed)).float()
    return base.repeat_interleave(block, 2).repeat_interleave(block, 3)[:, :, :H, :W].contiguous()


def binary_mask(shape, seed, p=0.7):
    B, _, H, W = shape
    return (torch.rand(B, 1, H, W, generator=gen(seed)) < p).float()


FIXTURE_SHAPES = [(2, 3, 13, 17), (1, 1, 5, 5)]          # fixtures stay a few tens of KB


def relerr(got, want64):
    """max |got - fp64| / max |fp64| (an all-zero fp64 tensor: the absolute error)."""
    want64 = want64.detach().double().cpu().reshape(-1)
    got = got.detach().double().cpu().reshape(-1)
    assert got.numel() == want64.numel(), (got.numel(), want64.numel())
    d, m = float((got - want64).abs().max()), float(want64.abs().max())
    return d / m if m > 0 else d


def bound(torch32, want64):
    """The rule's right-hand side, from the fp32 torch composition's own error on the same inputs."""
    return max(3e-6, 2.5 * relerr(torch32, want64))


def check(name, got, torch32, want64):
    e, b = relerr(got, want64), bound(torch32, want64)
    print('%-40s error %.3g  bound %.3g  (torch fp32 %.3g)' % (name, e, b, relerr(torch32, want64)))
    assert torch.isfinite(got).all(), name
    assert e <= b, (name, e, b)
