"""The result export, the parts that need no GPU: the numpy model of upf_flow_export (tests/_export_model.py) and the host
renderer tools.flow_to_image against what the reference's flow_to_image and the host KITTI writer's encode recorded
(tests/golden/export_*.npz, make_golden_export.py); the new flow_io writers against the existing ones, byte for byte; the new
symbols in the header, the binding and the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import _export_model as em
from conftest import GOLDEN, ROOT

FRAMES = em.golden_frames()


@pytest.fixture(scope='module')
def recorded():
    return np.load(os.path.join(GOLDEN, 'export_rgb.npz')), np.load(os.path.join(GOLDEN, 'export_kitti.npz'))


def test_the_fixtures_hold_the_frames_the_model_generates(recorded):
    rgb, kitti = recorded
    assert sorted(rgb.files) == sorted(FRAMES) == sorted(kitti.files)
    for H, W in ((9, 70), (33, 130), (64, 257)):
        for s in ('0.3', '3', '40'):
            assert FRAMES['motion_%dx%d_%s' % (H, W, s)].shape == (H, W, 2)
    total = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in ('export_rgb.npz', 'export_kitti.npz'))
    assert total < 100 * 1024
    above = [n for n, f in FRAMES.items() if em.top_pixel_rad(f) > 1.0]
    below = [n for n, f in FRAMES.items() if em.top_pixel_rad(f) <= 1.0]
    print('largest pixel with float64 rad > 1:', above)
    assert len(above) >= 3 and len(below) >= 3                       # the fp32 maximum lands on both sides of rad <= 1


@pytest.mark.parametrize('name', sorted(FRAMES))
def test_model_and_host_renderer_equal_the_reference(recorded, name):
    from upflow_pytorch_amd.utils.tools import tools
    rgb, kitti = recorded
    frame = FRAMES[name]
    before = frame.copy()
    assert np.array_equal(em.rgb(frame), rgb[name])
    got = tools.flow_to_image(frame)
    assert got.dtype == np.uint8 and np.array_equal(got, rgb[name])
    assert np.array_equal(em.kitti(frame), kitti[name]) and kitti[name].dtype == np.uint16
    assert np.array_equal(frame.view(np.uint32), before.view(np.uint32))          # (the reference zeroes unknown pixels in place)


def test_planted_pixels_of_the_fixtures(recorded):
    rgb, _ = recorded
    assert (rgb['zero'] == 255).all()                                             # no motion renders white
    unk = rgb['unknown']
    for y, x in ((0, 0), (1, 5), (2, 9), (3, 13), (8, 69)):
        assert (unk[y, x] == 0).all()                                             # unknown renders black
    assert (unk.reshape(-1, 3).max(axis=1) > 0).sum() == 9 * 70 - 5
    # an axis direction at full radius is a wheel entry (fk = 1 + 54 * (angle / 2 pi + 1/2) is an integer): +u is entry 1, red
    ax = rgb['axes4'][0]
    assert tuple(ax[0]) == (255, 0, 0)
    assert ax[2, 0] == 0 and ax[2, 2] == 255                                      # -u: entry 28, between cyan and blue


def test_a_nan_pixel_is_black_and_leaves_the_scale_alone():
    from upflow_pytorch_amd.utils.tools import tools
    frame = FRAMES['motion_9x70_3'].copy()
    want = em.rgb(frame)
    frame[4, 7, 1] = np.nan
    for got in (em.rgb(frame), tools.flow_to_image(frame)):
        assert (got[4, 7] == 0).all()
        keep = np.ones((9, 70), dtype=bool)
        keep[4, 7] = False
        assert np.array_equal(got[keep], want[keep])
    assert (em.kitti(frame)[4, 7] == 0).all()


def test_a_given_scale():
    from upflow_pytorch_amd.utils.tools import tools
    frame = FRAMES['motion_33x130_3']
    a, b = em.rgb(frame, max_rad=2.5), tools.flow_to_image(frame, max_rad=2.5)
    assert np.array_equal(a, b) and not np.array_equal(a, em.rgb(frame))
    assert np.array_equal(em.rgb(frame, max_rad=0), em.rgb(frame))
    assert np.array_equal(tools.flow_to_image(frame, max_rad=float(em.maxrad(frame))), em.rgb(frame))


def test_the_angle_decides_almost_nothing():
    """atan2 is the one operation of the rendering that is not IEEE-exact: moving it by one ulp either way changes no value of the
    random frames (on the axes it moves the angle across a wheel entry, and the two neighbours blend to the same colour +- 1)."""
    changed = total = 0
    for name, frame in FRAMES.items():
        if name.startswith(('motion', 'radgt1')):
            base = em.rgb(frame)
            for ulps in (-1, 1):
                changed += int((em.rgb(frame, angle_ulps=ulps) != base).sum())
                total += base.size
    print('values changed by one ulp of the angle: %d of %d' % (changed, total))
    assert changed == 0


def test_new_writers_are_byte_identical_and_read_back(tmp_path):
    from upflow_pytorch_amd.utils import flow_io
    for i, name in enumerate(('motion_9x70_40', 'motion_33x130_3', 'unknown', 'axes8')):
        frame = FRAMES[name]
        valid = (np.random.default_rng(i).random(frame.shape[:2]) > 0.3).astype(np.float32) if i % 2 else None
        old_png, new_png = str(tmp_path / ('old%d.png' % i)), str(tmp_path / ('new%d.png' % i))
        with np.errstate(invalid='ignore'):
            flow_io.write_kitti_png_file(old_png, frame, valid)
        flow_io.write_kitti_png_u16(new_png, em.kitti(frame, valid))
        assert open(old_png, 'rb').read() == open(new_png, 'rb').read()
        flow, mask = flow_io.read_kitti_png_flow(new_png)
        assert np.array_equal(mask[0], np.ones(frame.shape[:2]) if valid is None else valid)
        finite = np.isfinite(frame).all(axis=-1) & (np.abs(frame) < 511).all(axis=-1)
        assert np.all(np.abs(np.transpose(flow, [1, 2, 0])[finite] - frame[finite]) < 1.0 / 64)
        old_flo, new_flo = str(tmp_path / ('old%d.flo' % i)), str(tmp_path / ('new%d.flo' % i))
        flow_io.write_flo(frame, old_flo)
        flow_io.write_flo_payload(em.flo(frame), new_flo)
        assert open(old_flo, 'rb').read() == open(new_flo, 'rb').read()
        assert np.array_equal(flow_io.read_flo(new_flo).view(np.uint32), frame.view(np.uint32))
    for bad in (np.zeros((4, 5, 3), np.int16), np.zeros((4, 5, 2), np.uint16), np.zeros((4, 5), np.uint16)):
        with pytest.raises(ValueError):
            flow_io.write_kitti_png_u16(str(tmp_path / 'bad.png'), bad)
    for bad in (np.zeros((4, 5, 2), np.float64), np.zeros((4, 5, 3), np.float32)):
        with pytest.raises(ValueError):
            flow_io.write_flo_payload(bad, str(tmp_path / 'bad.flo'))


def test_new_symbols_in_header_binding_and_library():
    import __graft_entry__ as g
    g.build()
    from upflow_pytorch_amd import _lib, _build
    header = open(os.path.join(ROOT, 'include', 'upflow_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('upf_flow_export', 'upf_flow_export_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, header) and name in _lib.SIGNATURES and hasattr(L, name)
    assert ('export.hip', ['-ffp-contract=off']) in _build.SOURCES


def test_rejected_arguments_of_the_entry_point_need_no_gpu():
    """The argument checks come before any launch: they can be exercised with host pointers."""
    import __graft_entry__ as g
    g.build()
    from upflow_pytorch_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    nbytes = ctypes.c_longlong(-1)
    assert L.upf_flow_export_workspace_bytes(1, 375, 1242, ctypes.byref(nbytes)) == 0 and nbytes.value == 4 * 455
    assert L.upf_flow_export_workspace_bytes(2, 3, 5, ctypes.byref(nbytes)) == 0 and nbytes.value == 8
    assert L.upf_flow_export_workspace_bytes(1, 0, 5, ctypes.byref(nbytes)) == -1
    assert L.upf_flow_export_workspace_bytes(1, 3, 5, None) == -1
    assert L.upf_flow_export_workspace_bytes(2, 32768, 32768, ctypes.byref(nbytes)) == -4
    call = lambda *a: L.upf_flow_export(*a, None)                                 # noqa: E731
    assert call(None, None, p, None, None, 0.0, p, 1, 2, 2) == -1                 # no prediction
    assert call(p, None, None, None, None, 0.0, p, 1, 2, 2) == -1                 # no output
    assert call(p, None, None, p, None, 0.0, None, 1, 2, 2) == -1                 # a per-item scale without a workspace
    assert call(p, None, p, None, None, 0.0, p, 1, 0, 2) == -1                    # a non-positive size
    assert call(p, None, p, None, None, 0.0, p, 2, 32768, 32768) == -4            # 2^31 pixels
    assert call(p + 2, None, p, None, None, 0.0, p, 1, 2, 2) == -3                # misaligned prediction
    assert call(p, None, p + 1, None, None, 0.0, p, 1, 2, 2) == -3                # misaligned kitti
    assert call(p, None, None, None, p + 2, 0.0, p, 1, 2, 2) == -3                # misaligned flo
    assert 'aligned' in L.upf_last_error().decode()
