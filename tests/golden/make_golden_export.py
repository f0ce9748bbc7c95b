#!/usr/bin/env python3
"""Generate tests/golden/export_*.npz by IMPORTING the reference (as make_golden.py does; build container only).

For every frame of tests/_export_model.py's golden_frames() — float32 [H,W,2], regenerated from integers wherever the tests run —
the fixtures record results only:
    export_rgb.npz    <name>: uint8  [H,W,3]   the reference's tools.flow_to_image(frame)   (utils/tools.py:1342-1480)
    export_kitti.npz  <name>: uint16 [H,W,3]   the array flow_io.write_kitti_png_file encodes and hands to the PNG writer
flow_to_image modifies its argument (unknown pixels are zeroed in place), so it is given a copy.  A frame with a NaN is not
among them: the reference turns such a frame's scale into -1, which the package deliberately does not reproduce.

Usage:  python tests/golden/make_golden_export.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _export_model as em  # noqa: E402
from make_golden import import_reference  # noqa: E402


def encoded_by_the_host_writer(frame):
    """what write_kitti_png_file passes to write_png, caught there"""
    from upflow_pytorch_amd.utils import flow_io
    caught = []
    real = flow_io.write_png
    flow_io.write_png = lambda fn, img, *a, **k: caught.append(np.array(img))
    try:
        flow_io.write_kitti_png_file('unused.png', frame)
    finally:
        flow_io.write_png = real
    return caught[0]


def main():
    _, _, ref_tools, _ = import_reference()
    rgb, kitti = {}, {}
    for name, frame in em.golden_frames().items():
        with np.errstate(all='ignore'):
            rgb[name] = ref_tools.flow_to_image(frame.copy())
            kitti[name] = encoded_by_the_host_writer(frame)
        assert rgb[name].dtype == np.uint8 and kitti[name].dtype == np.uint16
        print('%-22s %-12s top-pixel rad - 1 = %+.3e' % (name, frame.shape[:2], em.top_pixel_rad(frame) - 1.0))
    np.savez_compressed(os.path.join(HERE, 'export_rgb.npz'), **rgb)
    np.savez_compressed(os.path.join(HERE, 'export_kitti.npz'), **kitti)
    for f in ('export_rgb.npz', 'export_kitti.npz'):
        print(f, os.path.getsize(os.path.join(HERE, f)), 'bytes')


if __name__ == '__main__':
    main()
