"""tests/_errmap_model.py, the numpy statement of upf_flow_error_image, and the host mirror tools.lib_to_show_flow, against what the
reference's flow_error_image_np returned for the fixture's inputs (tests/golden/errmap.npz, made by make_golden_errmap.py): every
pixel, no tolerance — numpy's fp32 square root (taken through float64) and divide are correctly rounded, and every bin bound is
an fp32 number.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _errmap_model as M
import _score_model as S
from conftest import ROOT

f32 = np.float32


@pytest.fixture(scope='module')
def fx():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'errmap.npz')))


def reference_bytes(ref):
    """rint(255 * image) of the reference's float B, G, R image, as R, G, B bytes; its NaN (a NaN error in the non-log map, whose
    cast is undefined) is the contract's 0"""
    with np.errstate(invalid='ignore'):
        x = np.rint(255.0 * ref[:, :, ::-1])
    assert np.nanmin(x) >= 0 and np.nanmax(x) <= 255
    return np.where(np.isnan(x), 0.0, x).astype(np.uint8)


def host_args(fx, dtype=np.float64):
    flow, m_occ = S.decode(fx['gt_occ'][0])
    _, m_noc = S.decode(fx['gt_noc'][0])
    return np.ascontiguousarray(fx['pred'][0].transpose(1, 2, 0)), flow, m_occ.astype(dtype)[..., None], m_noc.astype(dtype)[..., None]


def test_fixture_holds_the_cases(fx):
    """the bounds and one ulp below them, the relative branch, the values no bin holds, the last bin, every mask pair"""
    pred, gt_occ, gt_noc = fx['pred'], fx['gt_occ'], fx['gt_noc']
    assert pred.dtype == f32 and gt_occ.dtype == np.uint16 and gt_noc.dtype == np.uint16
    flow, m_occ = S.decode(gt_occ)
    _, m_noc = S.decode(gt_noc)
    diff, mag = M.error(pred[:, 0], pred[:, 1], flow[..., 0], flow[..., 1])
    third = M.div32(diff, f32(3.0))
    rgb = M.render(pred, gt_occ, gt_noc, True)[0]
    for k in range(1, 10):
        assert third[0, 0, k - 1] == M.LO[k] and tuple(rgb[0, 0, k - 1]) == tuple(M.FULL[k])
        assert third[0, 1, k - 1] == np.nextafter(M.LO[k], f32(0)) and tuple(rgb[0, 1, k - 1]) == tuple(M.FULL[k - 1])
    rel = M.div32(S.mul32(np.full_like(diff, 20.0), diff), S.add32(mag, np.full_like(mag, 1e-7)))
    assert mag[0, 2].min() > 60 and np.all(rel[0, 2] < third[0, 2]) and len({tuple(c) for c in rgb[0, 2]}) >= 10
    row = pred[0, 0, 3]
    assert row[0] == f32(4e9) and np.isposinf(row[2]) and np.isneginf(row[4]) and np.isnan(row[6]) and row[8] == f32(2.9999e9)
    assert not rgb[0, 3, :8].any() and not rgb[0, 3, 10:14].any()
    assert tuple(rgb[0, 3, 8]) == tuple(M.FULL[9]) and tuple(rgb[0, 3, 9]) == tuple(M.HALF[9])
    assert {(int(a), int(b)) for a, b in zip(m_occ.ravel(), m_noc.ravel())} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_tables_are_the_references(fx):
    assert np.array_equal(fx['table_full'], M.FULL) and np.array_equal(fx['table_half'], M.HALF)
    assert tuple(M.HALF[0]) == (25, 27, 75)
    assert np.array_equal(M.HALF, (M.FULL.astype(int) + 1) // 2)            # how the present table happens to evaluate
    from upflow_pytorch_amd.utils.tools import tools
    assert np.array_equal(np.array(tools.lib_to_show_flow.ERROR_COLORS)[:, 2:], M.FULL)
    assert np.array_equal(np.array(tools.lib_to_show_flow.ERROR_COLORS, dtype=f32)[:, 0], M.LO[:10])
    src = open(os.path.join(ROOT, 'upflow_pytorch_amd', 'csrc', 'errmap.hip')).read()
    for name, table in (('FULL', M.FULL), ('HALF', M.HALF)):
        body = re.search(r'%s\[BINS\]\[3\]\s*=\s*\{(.*?)\};' % name, src, flags=re.S).group(1)
        assert [int(v) for v in re.findall(r'\d+', body)] == [int(v) for v in table.ravel()], name


@pytest.mark.parametrize('log_colors', [True, False])
def test_model_gives_the_references_bytes_at_every_pixel(fx, log_colors):
    want = reference_bytes(fx['ref_log' if log_colors else 'ref_lin'])
    got = M.flow_error_image(fx['pred'], fx['gt_occ'], fx['gt_noc'], log_colors)[0]
    wrong = np.any(got != want, axis=-1)
    assert wrong.sum() == 0, 'the model differs from the reference at %d of %d pixels, first %s' % (wrong.sum(), wrong.size, np.argwhere(wrong)[:4].tolist())


@pytest.mark.parametrize('log_colors', [True, False])
def test_host_mirror_returns_the_references_array(fx, log_colors):
    from upflow_pytorch_amd.utils.tools import tools
    ref = fx['ref_log' if log_colors else 'ref_lin']
    got = tools.lib_to_show_flow.flow_error_image_np(*host_args(fx), log_colors=log_colors)
    assert got.shape == ref.shape and np.issubdtype(got.dtype, np.floating)
    assert np.array_equal(got.astype(np.float64), ref, equal_nan=True)


@pytest.mark.parametrize('log_colors', [True, False])
@pytest.mark.parametrize('mask_dtype', [np.float64, np.float32])
def test_flow_error_image_u8_is_the_model(fx, log_colors, mask_dtype):
    from upflow_pytorch_amd.utils.tools import tools
    got = tools.flow_error_image_u8(*host_args(fx, mask_dtype), log_colors=log_colors)
    assert got.dtype == np.uint8
    assert np.array_equal(got, M.flow_error_image(fx['pred'], fx['gt_occ'], fx['gt_noc'], log_colors)[0])


def test_mask_noc_defaults_to_not_occluded(fx):
    from upflow_pytorch_amd.utils.tools import tools
    pred, flow, m_occ, _ = host_args(fx)
    a = tools.lib_to_show_flow.flow_error_image_np(pred, flow, m_occ)
    b = tools.lib_to_show_flow.flow_error_image_np(pred, flow, m_occ, np.ones_like(m_occ), True)
    assert np.array_equal(a, b)


def test_dilate_model_on_a_hand_made_case():
    """5 x 7, r = 1: valid pixels a (0,0), b (1,2), c (1,3), d (4,6) and e (3,1), whose colour is BLACK (it still paints).  Each
    invalid pixel shows the valid pixel of its 3 x 3 window that comes last in raster order; '.' has none."""
    col = {'a': (10, 11, 12), 'b': (20, 21, 22), 'c': (30, 31, 32), 'd': (40, 41, 42), 'e': (0, 0, 0), '.': (0, 0, 0)}
    rgb = np.zeros((1, 5, 7, 3), dtype=np.uint8)
    valid = np.zeros((1, 5, 7), dtype=bool)
    for name, (y, x) in {'a': (0, 0), 'b': (1, 2), 'c': (1, 3), 'd': (4, 6), 'e': (3, 1)}.items():
        rgb[0, y, x], valid[0, y, x] = col[name], True
    want = ['abccc..',
            'abbcc..',
            'eeecc..',
            'eee..dd',
            'eee..dd']
    # (0,1): a (0,0) and b (1,2) compete, b is later; (1,1): a, b -> b; (2,1): b (1,2) and e (3,1) -> e; (2,2): b, c, e -> e;
    # (0,2), (0,3): b, c -> c; (1,2) and (1,3) keep their own; (2,3): b, c -> c; (2,4): c
    expected = np.array([[col[ch] for ch in row] for row in want], dtype=np.uint8)[None]
    assert np.array_equal(M.dilate(rgb, valid, 1), expected)
    assert np.array_equal(M.dilate(rgb, valid, 0), rgb)
    # r = 4 covers the frame from (4,6) back to (0,2) and (0,..): the last valid pixel in raster order wins everywhere it reaches
    big = M.dilate(rgb, valid, 4)
    assert tuple(big[0, 0, 2]) == col['d'] and tuple(big[0, 0, 1]) == col['e'] and tuple(big[0, 0, 0]) == col['a']


def test_symbols_in_the_header_and_the_library():
    import __graft_entry__ as g
    g.build()
    from upflow_pytorch_amd import _build, _lib
    header = open(os.path.join(ROOT, 'include', 'upflow_hip.h')).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ('upf_flow_error_image', 'upf_flow_error_image_workspace_bytes'):
        assert re.search(r'\bint %s\(' % sym, header) and hasattr(L, sym) and sym in _lib.SIGNATURES
    assert ('errmap.hip', ['-ffp-contract=off']) in _build.SOURCES
    nbytes = ctypes.c_longlong(-1)
    for r in range(5):                                                      # (host code only: no GPU is touched)
        assert L.upf_flow_error_image_workspace_bytes(1, 375, 1242, r, ctypes.byref(nbytes)) == 0 and nbytes.value >= 0
    assert L.upf_flow_error_image_workspace_bytes(1, 375, 1242, 0, ctypes.byref(nbytes)) == 0 and nbytes.value == 0
    assert L.upf_flow_error_image_workspace_bytes(1, 375, 1242, 5, ctypes.byref(nbytes)) != 0
    assert L.upf_flow_error_image_workspace_bytes(1, 375, 1242, -1, ctypes.byref(nbytes)) != 0
    assert L.upf_flow_error_image_workspace_bytes(0, 375, 1242, 0, ctypes.byref(nbytes)) != 0
    assert L.upf_flow_error_image_workspace_bytes(1, 375, 1242, 0, None) != 0
