"""The weight-gradient PLANNER (csrc/conv_wgrad.hip: make_levels / make_plan / pick_split / pc_split_co) is host code, and
upf_conv_wgrad_multi_workspace_bytes exposes its result: ns x J partial blocks of taps x pad64(Cout) x pad64(Cin) fp32.  No GPU
needed: the library loads without one and the level lists carry null data pointers (as upf_conv_wgrad_workspace_bytes builds them).

The byte counts below were recorded from the build of commit b1dc50b ("tests: exact checks of the warp and flow-resize kernels,
every route"), the last one whose host layer also planned for the first-form kernel; the planner was rewritten on top of it
(one level table, one plan) and must give the same split for every layer.  A changed count is a changed launch grid: the
training step's speed and summation order move with it, so change the table only together with a measured reason."""
import ctypes

import pytest

# the pyramid of a 256x832 training crop (batch 8): levels 64x208 ... 4x13
L208, L104, L52, L26, L13 = (8, 64, 208), (8, 32, 104), (8, 16, 52), (8, 8, 26), (8, 4, 13)
PYRAMID = [L208, L104, L52, L26, L13]

# (name, levels [(B, H, W)], Cin, Cout, k, d, bytes recorded from the parent build)
CASES = [
    # ---- the contractions of a config-3 training step (profiles/r05_wgrad_layers.txt)
    ('decoder 565->128, five levels (18 block pairs: one launch per co block)', PYRAMID, 565, 128, 3, 1, 63700992),
    ('decoder 243->128, five levels', PYRAMID, 243, 128, 3, 1, 37748736),
    ('feature pyramid 96->96 at 16x52', [L52], 96, 96, 3, 1, 9437184),
    ('feature pyramid 196->196 at 4x13', [L13], 196, 196, 3, 1, 9437184),
    ('1x1 64->32 at 32x104', [L104], 64, 32, 1, 1, 2097152),
    ('context 96->64, dilation 16', PYRAMID, 96, 64, 3, 16, 37748736),
    ('context 128->96, dilation 8', PYRAMID, 128, 96, 3, 8, 37748736),
    ('head 32->2', PYRAMID, 32, 2, 3, 1, 23592960),
    ('tail group 184->59 (Cout <= 64)', [L208, L208, L104, L52, L26], 184, 59, 3, 1, 35389440),
    ('space-to-depth 4x32->64 at 32x104', [L104], 4 * 32, 64, 3, 1, 18874368),
    ('space-to-depth 4x3->16 at 128x416', [(8, 128, 416)], 4 * 3, 16, 3, 1, 37748736),
    # ---- edges
    ('one 8x8 level: 2 tiles, fewer than the slices', [(1, 8, 8)], 64, 64, 3, 1, 294912),
    ('one 8x8 level, 1x1', [(1, 8, 8)], 64, 64, 1, 1, 32768),
    ('six levels, the maximum', PYRAMID + [(8, 128, 416)], 128, 128, 3, 2, 37748736),
    ('520->70: 2 x 9 block pairs, 256 + 4 tiles (split)', [(2, 64, 256), (2, 8, 26)], 520, 70, 3, 1, 42467328),
    ('520->70: 2 x 9 block pairs, exactly 256 tiles (split)', [(2, 64, 256)], 520, 70, 3, 1, 42467328),
    ('520->70: 2 x 9 block pairs, 224 tiles (one launch)', [(2, 64, 224)], 520, 70, 3, 1, 21233664),
    ('565->128 at 8x26: 18 block pairs, 16 tiles (one launch)', [L26], 565, 128, 3, 1, 10616832),
    ('Cin, Cout no multiples of 64: 115->70, dilation 4', [L104, L52], 115, 70, 3, 4, 23592960),
    ('Cin, Cout no multiples of 64: 40->130, 1x1', [L104, L52, L13], 40, 130, 1, 1, 3538944),
]


def _levels(levels):
    from upflow_pytorch_amd import _lib
    arr = (_lib.WgradLevel * len(levels))()
    for a, (B, H, W) in zip(arr, levels):
        a.x, a.x_batch_stride, a.grad_pre, a.g_batch_stride, a.B, a.H, a.W = None, 0, None, 0, B, H, W
    return arr


def _workspace_bytes(levels, Cin, Cout, k, d):
    import __graft_entry__ as g
    g.build()
    from upflow_pytorch_amd import _lib
    return _lib.lib().upf_conv_wgrad_multi_workspace_bytes(ctypes.cast(_levels(levels), ctypes.c_void_p), len(levels), Cin, Cout, k, d)


def _pad64(c):
    return (c + 63) // 64 * 64


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_the_plan_is_the_recorded_one(case):
    name, levels, Cin, Cout, k, d, recorded = case
    got = _workspace_bytes(levels, Cin, Cout, k, d)
    block = (1 if k == 1 else 9) * _pad64(Cout) * _pad64(Cin) * 4
    print('%s: %d bytes = %d partial blocks of %d' % (name, got, got // block, block))
    assert got > 0 and got % block == 0
    assert got == recorded, (name, got, recorded, 'partial blocks: %d, recorded %d' % (got // block, recorded // block))


def test_the_single_level_entry_point_plans_like_a_one_level_list():
    import __graft_entry__ as g
    g.build()
    from upflow_pytorch_amd import _lib
    for (B, H, W), Cin, Cout, k, d in ((L52, 96, 96, 3, 1), (L104, 64, 32, 1, 1), ((1, 8, 8), 64, 64, 3, 1)):
        assert _lib.lib().upf_conv_wgrad_workspace_bytes(B, Cin, Cout, H, W, k, d) == _workspace_bytes([(B, H, W)], Cin, Cout, k, d)


def test_a_bad_level_list_has_no_plan():
    import __graft_entry__ as g
    g.build()
    from upflow_pytorch_amd import _lib
    f = _lib.lib().upf_conv_wgrad_multi_workspace_bytes
    assert f(None, 1, 64, 64, 3, 1) == -1
    assert f(ctypes.cast(_levels(PYRAMID), ctypes.c_void_p), 0, 64, 64, 3, 1) == -1
    assert f(ctypes.cast(_levels(PYRAMID + [L13, L13]), ctypes.c_void_p), 7, 64, 64, 3, 1) == -1
