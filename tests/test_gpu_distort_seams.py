"""GPU: the two stand-alone distort kernels (raster_resolve.h) beyond one trip of their grid-stride loops, against
``oracle.ref_numpy`` (pinned to the reference's own float32 maps, g13, by test_oracle_golden_render.py), and the reference's
``_distort`` vectors (g2) through ``alp_distort_map``.

seam                                                              size that crosses it             test
distort_map_kernel / distort_image_kernel: grid capped at 4096    1024 x 1024 (exactly one trip),   test_distort_beyond_one_trip
blocks of 256 = 1 048 576 pixels per trip                         1024 x 1025 (one row more),
                                                                  1201 x 1807 (two trips and a
                                                                  ragged third)
one pixel, one row, one column, the width and height limits       1 x 1, 1 x 1000, 1000 x 1,        test_distort_beyond_one_trip
                                                                  3 x 32768, 32768 x 3
distort_image_kernel: channel count c > 1 and the 2-D form        c = 1, 3, 4 and (h, w)            test_distort_beyond_one_trip
the reference's _distort (g2) on the device                      31 grid points of 5616 x 3744     test_g2_distort_vectors_through_the_device_map
                                                                  and 641 x 479

The maps are bit-equal to the numpy oracle's at g13's sizes, and the arithmetic per pixel does not depend on the size: they
must be bit-equal here too.  At 1201 x 1807 the sets radial, full and strong put 244 to 278 values of the two maps exactly on a
rounding tie and radial and full send 6.4 and 4.7 % of the pixels outside the image (asserted below): round-half-even and the
zero border are both exercised."""
import os

import numpy as np
import pytest

from oracle import ref_numpy as orc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
SIZES = [(1, 1), (1, 1000), (1000, 1), (1024, 1024), (1024, 1025), (1201, 1807), (3, 32768), (32768, 3)]
COEFFS = ["identity", "aonly", "radial", "full", "strong"]
TRIP = 4096 * 256                      # alp_raster.hip, distort_setup: at most 4096 blocks of 256 threads


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(G, "g13_distort_map.npz"), allow_pickle=False)


def test_the_sizes_sit_on_the_grid_cap():
    src = open(os.path.join(os.path.dirname(G), os.pardir, "alproj_amd", "csrc", "alp_raster.hip")).read()
    assert "*grid = (int)(want < 4096 ? want : 4096);" in src
    trips = [-(-h * w // TRIP) for h, w in SIZES]
    assert trips == [1, 1, 1, 1, 2, 3, 1, 1] and 1024 * 1024 == TRIP and 2 * TRIP < 1201 * 1807 < 3 * TRIP


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", COEFFS)
def test_distort_beyond_one_trip(L, g13, name, size):
    h, w = size
    coeffs = g13[f"coeffs_{name}"]
    want_x, want_y = orc.distort_maps(w, h, coeffs)
    mx, my = L.distort_map(h, w, coeffs)
    assert mx.dtype == np.float32 and mx.shape == (h, w)
    np.testing.assert_array_equal(mx, want_x)
    np.testing.assert_array_equal(my, want_y)
    del mx, my
    if size == (1201, 1807) and name in ("radial", "full", "strong"):
        ties = sum(int((np.abs(m.astype(np.float64) - np.floor(m.astype(np.float64)) - 0.5) == 0).sum()) for m in (want_x, want_y))
        assert ties >= 100
        if name != "strong":
            sx, sy = np.rint(want_x.astype(np.float64)), np.rint(want_y.astype(np.float64))
            assert 0.04 < 1 - ((sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)).mean() < 0.07
    index = np.arange(1, h * w + 1, dtype=np.float32).reshape(h, w)            # < 2^24: every pixel its own exact value
    for c in (None, 1, 3, 4):
        img = index if c is None else np.stack([index + np.float32(k) for k in range(c)], axis=2)
        got = L.distort_image(img, coeffs)
        assert got.shape == img.shape and got.dtype == np.float32
        np.testing.assert_array_equal(got, orc.remap_nearest(img, want_x, want_y), err_msg=f"c = {c}")
    if name == "identity" and h > 1 and w > 1:      # (one row or column: the centre (w - 1) / 2 is 0, the reference's map is NaN)
        np.testing.assert_array_equal(got[..., 0], index)


def test_g2_distort_vectors_through_the_device_map(L):
    """g2 = the reference's ``_distort`` on grids of points.  ``distort`` evaluates ``_distort`` with 1/a1, 1/a2 and every
    other coefficient negated (project.py:128-140), so alp_distort_map with (1/a1, 1/a2, -k1 .. -s4) evaluates ``_distort``
    with g2's own coefficients at every pixel: float32(g2's output) at every g2 point that is a pixel of the image"""
    g = np.load(os.path.join(G, "g2_distort.npz"), allow_pickle=False)
    compared = 0
    for size in ("5616x3744", "641x479"):
        w, h = (int(s) for s in size.split("x"))
        pts = g[f"pts_{size}"]
        sel = (pts == np.rint(pts)).all(axis=1) & (pts[:, 0] >= 0) & (pts[:, 0] < w) & (pts[:, 1] >= 0) & (pts[:, 1] < h)
        x, y = pts[sel, 0].astype(np.int64), pts[sel, 1].astype(np.int64)
        for name in ("zero", "aonly", "radial", "full"):
            c = g[f"coeffs_{name}"]
            mx, my = L.distort_map(h, w, np.concatenate([1.0 / c[:2], -c[2:]]))
            want = g[f"out_{name}_{size}"][sel].astype(np.float32)
            np.testing.assert_array_equal(mx[y, x], want[:, 0], err_msg=f"{name} {size}")
            np.testing.assert_array_equal(my[y, x], want[:, 1], err_msg=f"{name} {size}")
            del mx, my
        compared += int(sel.sum())
    assert compared == 31
