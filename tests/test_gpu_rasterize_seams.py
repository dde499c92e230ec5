"""GPU: the rasterisation kernels (alproj_amd/csrc/rasterize_runs.h, rasterize_median.h, rasterize_tail.h) at every internal
seam, on the tables of tests/rasterize_seam_cases.py that hit each seam on purpose (tests/test_rasterize_seam_cases.py asserts
on the CPU that they do): 16-position segments and their join, groups of 64 in turns of 512 with five files by run length,
the in-register networks, the wave-wide histogram select, the composite keys of 8, 16 and 32 value bits and the two-sort
median, the eight-at-a-time Kahan walk, and the tiled tail with its halo, its 3 x 3 "holds a point" mask and its second
trips.  The reference is ``oracle.ref_numpy.rasterize_points`` throughout (pandas groupby + scipy's generic_filter):
aggregates on the float32 raster, every bit and the NaN pattern; the tail on bytes.

Not covered: the second trip of rz_median_packed_kernel's turn loop (``turn += gridDim.x``).  Its launch has
min(turns, 256 * cu_count) workgroups, so a second trip needs more than 512 * 256 * cu_count points -- 33.5 M on 256 CUs,
which no test that runs in seconds reaches -- and the product gets no test hook for it."""
import ctypes
import time
import warnings

import numpy as np
import pandas as pd
import pytest

from oracle import ref_numpy as orc
from tests import rasterize_seam_cases as sc

pytestmark = pytest.mark.gpu

PATHS = (None, "ALP_RZ_NO_PACKED", "ALP_RZ_SEQUENTIAL")
ENVS = ("ALP_RZ_NO_PACKED", "ALP_RZ_SEQUENTIAL", "ALP_RZ_SEPARATE_PASSES")
AGG_CODE = {"mean": 0, "max": 1, "min": 2, "median": 3}


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def _only(monkeypatch, env):
    for e in ENVS:
        monkeypatch.delenv(e, raising=False)
    if env:
        monkeypatch.setenv(env, "1")


def _oracle(x, y, vals, interpolate, max_dist, agg, nodata=255, return_float=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return orc.rasterize_points(x, y, vals, 1.0, interpolate, max_dist, agg, nodata, return_float=return_float)


def _differing(got, ref):
    same = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    return np.argwhere(~same)


@pytest.mark.parametrize("agg", sc.AGGS)
@pytest.mark.parametrize("layout", list(sc.LAYOUTS))
def test_aggregates_at_every_seam(L, layout, agg, monkeypatch):
    """the float32 raster of every table of the layout, for every value kind and band count of its plan, on the default
    path, with ALP_RZ_NO_PACKED=1 and with ALP_RZ_SEQUENTIAL=1: pandas' bits, pandas' NaN pattern"""
    t0, calls = time.perf_counter(), 0
    for table in sc.LAYOUTS[layout]():
        for kind, nb in sc.value_plan(layout):
            vals = sc.values(table, kind, nb)
            ref, rb = _oracle(table.x, table.y, vals, False, 1.0, agg, return_float=True)
            assert ref.shape == (nb, table.size[1], table.size[0])
            for env in PATHS:
                _only(monkeypatch, env)
                got, gb = L.rasterize_points_f32(table.x, table.y, vals, 1.0, False, 1.0, agg)
                calls += 1
                assert gb == rb and got.dtype == np.float32 and got.shape == ref.shape
                bad = _differing(got, ref)
                assert not len(bad), (f"{layout}/{table.name} {kind} x{nb} {agg} {env or 'default'}: {len(bad)} cells differ, first "
                                      f"(band, row, col) {bad[0].tolist()}: {got[tuple(bad[0])]!r} for {ref[tuple(bad[0])]!r}")
    print(f"{layout} {agg}: {calls} device calls, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("agg", sc.AGGS)
@pytest.mark.parametrize("case", list(sc.TAIL_CASES))
def test_tail_at_every_tile_seam(L, case, agg, monkeypatch):
    """S = 0, 1, 2, 7, 8 sweeps: the fused tail's bytes are the oracle's and those of the separate passes
    (ALP_RZ_SEPARATE_PASSES=1); S = 9: the separate passes' bytes are the oracle's.  nodata 255, 0 and 7 in turn."""
    from alproj_amd import project as prj
    table, vals = sc.tail_case(case)
    bands = [f"b{k}" for k in range(vals.shape[1])]
    df = pd.DataFrame({"x": table.x, "y": table.y, **{b: vals[:, k] for k, b in enumerate(bands)}})
    for k, S in enumerate(sc.TAIL_SWEEPS + (sc.RZ_SMAX + 1,)):
        nodata = sc.NODATA[k % 3]
        kw = dict(resolution=1.0, bands=bands, interpolate=S > 0, max_dist=float(S), agg_func=agg, nodata=nodata)
        ref, rb = _oracle(table.x, table.y, vals, S > 0, float(max(S, 1)), agg, nodata)
        assert ref.shape == (len(bands), table.size[1], table.size[0])
        _only(monkeypatch, "ALP_RZ_SEPARATE_PASSES")
        sep, sb = prj.rasterize(df, **kw)
        assert sb == rb
        if S <= sc.RZ_SMAX:
            _only(monkeypatch, None)
            got, gb = prj.rasterize(df, **kw)
            assert gb == rb
            np.testing.assert_array_equal(got, ref, err_msg=f"{case} {agg} S={S} nodata={nodata}: fused tail against the oracle")
            np.testing.assert_array_equal(got, sep, err_msg=f"{case} {agg} S={S} nodata={nodata}: fused tail against the separate passes")
        np.testing.assert_array_equal(sep, ref, err_msg=f"{case} {agg} S={S} nodata={nodata}: separate passes against the oracle")


@pytest.mark.parametrize("agg", sc.AGGS)
def test_points_outside_the_extent_go_to_the_rim_cells(L, agg, monkeypatch):
    """alp_rasterize_points with an extent tighter than the table: points left, right, above and below it are clipped into
    the rim cells (project.py:435-436) -- the oracle's raster of the same table with its coordinates clipped into the extent"""
    _only(monkeypatch, None)
    rng = np.random.default_rng(17)
    lengths = rng.integers(0, 5, 20 * 16)
    lengths[[0, 19, 300, 319]] = 2
    x, y, (w, h) = sc.table_from_runs(lengths, 20, seed=5)
    x_min, x_max, y_min, y_max = 3.0, w - 2.0, 1.0, h - 4.0
    assert (x < x_min).any() and (x > x_max).any() and (y < y_min).any() and (y > y_max).any()
    w2, h2 = int(x_max - x_min), int(y_max - y_min)
    xc, yc = np.clip(x, x_min, x_max), np.clip(y, y_min, y_max)
    makers = {"floats": lambda nb: rng.uniform(-40.0, 300.0, (len(x), nb)),                      # the Kahan walk: row order in the rim cells
              "bytes": lambda nb: rng.integers(0, 256, (len(x), nb)).astype(np.float64),
              "float32": lambda nb: rng.uniform(-40.0, 300.0, (len(x), nb)).astype(np.float32).astype(np.float64)}
    for kind, nb, nodata in (("floats", 3, 255), ("bytes", 4, 7), ("float32", 1, 0)):
        vals = makers[kind](nb)
        ref, rb = _oracle(xc, yc, vals, True, 1.0, agg, nodata)
        assert rb == (x_min, y_min, x_max, y_max, w2, h2)
        out = np.empty((nb, h2, w2), dtype=np.uint8)
        L.check(L.lib().alp_rasterize_points(L.as_dp(x), L.as_dp(y), L.as_dp(vals), len(x), nb, x_min, y_max, 1.0, w2, h2,
                                             AGG_CODE[agg], 1, nodata, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        np.testing.assert_array_equal(out, ref, err_msg=f"{agg} {kind}")


def test_second_trips_of_the_tail_and_the_fill(L, monkeypatch):
    """a sparse raster of 64 x 36 tiles (more on a device of more than 256 CUs) with four byte bands and one point per tile, at a
    different in-tile position each: more tiles than rz_fill_tiles_kernel has workgroups (8 * cu_count) and more
    (tile, band) items than rz_tail_kernel has (32 * cu_count) -- both loops take a second trip"""
    from alproj_amd import project as prj
    cu = L.device_info()["cu_count"]
    tiles_x, tiles_y = 64, max(36, (8 * cu) // 64 + 4)
    table = sc.sparse_tiles_table(tiles_x, tiles_y)
    nb = 4
    assert tiles_x * tiles_y > 8 * cu and tiles_x * tiles_y * nb > 32 * cu and table.n == tiles_x * tiles_y
    vals = sc.values(table, "bytes", nb)
    bands = [f"b{k}" for k in range(nb)]
    df = pd.DataFrame({"x": table.x, "y": table.y, **{b: vals[:, k] for k, b in enumerate(bands)}})
    _only(monkeypatch, None)
    for agg in ("mean", "median"):
        got, gb = prj.rasterize(df, resolution=1.0, bands=bands, interpolate=False, agg_func=agg, nodata=7)
        ref, rb = _oracle(table.x, table.y, vals, False, 1.0, agg, 7)             # no filter runs: cheap
        assert gb == rb and got.shape == (nb, tiles_y * sc.RZ_TH, tiles_x * sc.RZ_TW)
        np.testing.assert_array_equal(got, ref, err_msg=agg)
        assert (got != 7).sum() >= 0.98 * nb * table.n
    # one sweep: the fused tail against the separate passes (which the small cases hold to the oracle)
    fused, _ = prj.rasterize(df, resolution=1.0, bands=bands, interpolate=True, max_dist=1.0, agg_func="mean", nodata=7)
    _only(monkeypatch, "ALP_RZ_SEPARATE_PASSES")
    sep, _ = prj.rasterize(df, resolution=1.0, bands=bands, interpolate=True, max_dist=1.0, agg_func="mean", nodata=7)
    np.testing.assert_array_equal(fused, sep)
    assert (fused != 7).sum() > 8 * table.n
