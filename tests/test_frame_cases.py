"""CPU: pin the numpy statements of tests/frame_cases.py to what the REFERENCE produced -- g12: the tables its
reverse_proj returned for seeded raw renders (tags a, b, c, with and without offsets) and the bytes its sim_image
returned -- and their case tables to the constants of raster_post.h.  The GPU seam tests (test_gpu_frame_seams.py) hold
the kernels to these statements at sizes the fixtures do not reach.  (``oracle.ref_numpy.distort_maps``, the reference of
test_gpu_distort_seams.py, is pinned to g13 by test_oracle_golden_render.py.)"""
import os
import re

import numpy as np
import pytest

from alproj_amd import synthetic as syn
from tests import frame_cases as fc

G = os.path.join(os.path.dirname(__file__), "golden")
CSRC = os.path.join(os.path.dirname(os.path.dirname(__file__)), "alproj_amd", "csrc")


@pytest.fixture(scope="module")
def g12():
    return np.load(os.path.join(G, "g12_wrappers.npz"), allow_pickle=False)


@pytest.mark.parametrize("otag", ["off", "nooff"])
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_valid_table_and_gather_reproduce_the_references_tables(g12, tag, otag):
    raw, array = g12[f"{tag}_raw"], g12[f"{tag}_array"]
    off = g12["offsets"] if otag == "off" else None
    cols = [str(c) for c in g12[f"{tag}_{otag}_columns"]]
    want = dict(zip(cols, g12[f"{tag}_{otag}_values"].T))
    idx, xyz, u, v, chan = fc.valid_table(raw, off, array)
    assert idx.dtype == np.uint32 and u.dtype == np.int16 and v.dtype == np.int16 and xyz.dtype == np.float64
    np.testing.assert_array_equal(idx, g12[f"{tag}_{otag}_index"])
    np.testing.assert_array_equal(u, want["u"])
    np.testing.assert_array_equal(v, want["v"])
    np.testing.assert_array_equal(xyz, np.stack([want["x"], want["y"], want["z"]], axis=1))
    assert chan.shape == (array.shape[2], len(idx)) and chan.dtype == np.float64
    for k, name in enumerate(str(c) for c in g12[f"{tag}_chnames"]):
        np.testing.assert_array_equal(chan[k], want[name])
    assert len(idx) > 1000 and (raw[..., 0] <= 0).any()
    # the lookup of the table's own pixels gives its rows back, every other pixel of the frame NaN
    np.testing.assert_array_equal(fc.gather(raw, u, v, off), xyz)
    h, w = raw.shape[:2]
    vv, uu = np.divmod(np.arange(h * w), w)
    everywhere = fc.gather(raw, uu, vv, off)
    np.testing.assert_array_equal(everywhere[idx], xyz)
    assert np.isnan(np.delete(everywhere, idx, axis=0)).all()
    assert np.isnan(fc.gather(raw, [-1, w, 0, 0], [0, 0, -1, h], off)).all()
    # bounds: the extent of the finite part of the reference's columns
    with np.errstate(invalid="ignore"):
        b = fc.valid_bounds(xyz)
    assert b[0] == np.nanmin(want["x"]) and b[3] == np.nanmax(want["y"])


def test_valid_bounds_skips_nan_and_is_nan_when_empty():
    xyz = np.array([[3.0, np.nan, 1.0], [2.0, -np.inf, np.nan], [np.inf, 7.0, 0.0]])
    assert fc.valid_bounds(xyz) == (2.0, -np.inf, np.inf, 7.0)
    assert np.isnan(fc.valid_bounds(np.empty((0, 3)))).all()


def test_image_u8_reproduces_the_references_bytes(g12):
    np.testing.assert_array_equal(fc.image_u8(g12["sim_raw"], 255.0, True), g12["sim_bgr"])
    np.testing.assert_array_equal(fc.image_u8(g12["sim_raw"], 255.0, False), g12["sim_bgr"][:, :, ::-1])
    wild = np.array([[[-0.01, 1.004, 2.5], [300.7, -1.2, 0.5], [np.nan, 1e12, -1e12]]], dtype=np.float32)
    # -2.55 -> -2 -> 254, 256.02 -> 0, 637.5 -> 637 - 512; 76678.5 -> 76678 - 299 * 256, -306 + 512, 127.5 -> 127; none in range
    np.testing.assert_array_equal(fc.image_u8(wild, 255.0, False), [[[254, 0, 125], [134, 206, 127], [0, 0, 0]]])


def test_distance_keep_is_the_references_filter():
    """g10: the rows the reference's filter_gcp_distance kept, for every (lo, hi) it was run with"""
    g = np.load(os.path.join(G, "g10_gcp.npz"), allow_pickle=False)
    rows = g["filt_input"]
    masks = 0
    for k, (lo, hi) in enumerate(g["filt_cases"]):
        if np.isnan(lo) and np.isnan(hi):             # no bound at all: the reference hands its input back, no mask is formed
            continue
        keep = fc.distance_keep(rows[:, 2:5], g["cam"], None if np.isnan(lo) else lo, None if np.isnan(hi) else hi)
        np.testing.assert_array_equal(rows[keep], g[f"filt{k}_values"])
        masks += 1
        assert 0 < keep.sum() < len(rows)
    assert masks >= 3


def test_grid_triangles_is_the_grid_of_the_surface_module():
    for n in (2, 3, 17):
        for dtype in (np.int32, np.int64):
            t = fc.grid_triangles(n, n, dtype)
            assert t.dtype == dtype
            np.testing.assert_array_equal(t, syn.grid_indices(n, dtype))
    t = fc.grid_triangles(3, 4)                 # 3 rows of 4: cells 0 1 2 / 4 5 6
    np.testing.assert_array_equal(t[:2], [[0, 4, 5], [0, 5, 1]])
    np.testing.assert_array_equal(t[-2:], [[6, 10, 11], [6, 11, 7]])
    assert len(t) == 2 * 2 * 3


def test_case_tables_sit_on_the_kernels_constants():
    """the shapes are chosen against COMPACT_CHUNK and the scan's 1024 threads: both are read from the source"""
    post = open(os.path.join(CSRC, "raster_post.h")).read()
    assert int(re.search(r"constexpr int COMPACT_CHUNK = (\d+);", post).group(1)) == fc.COMPACT_CHUNK
    assert re.search(r"__launch_bounds__\((\d+)\) void scan_counts_kernel", post).group(1) == str(fc.SCAN_THREADS)
    assert "const int per = (n + 1023) / 1024;" in post
    for name, (h, w) in fc.LARGE_SHAPES.items():
        chunks, tail = fc.LARGE_CHUNKS[name]
        assert h <= fc.MAX_SIDE and w <= fc.MAX_SIDE
        assert fc.chunks_of(h * w) == chunks and h * w - (chunks - 1) * fc.COMPACT_CHUNK == tail, name
    per = sorted({-(-c // fc.SCAN_THREADS) for c, _ in fc.LARGE_CHUNKS.values()})
    assert per == [1, 2, 3]
    assert fc.shape_of(2048 * 4096 + 1) is None and fc.shape_of((1 << 20) + 1) is None      # why two cases are off by one
    assert sorted(h * w for h, w in fc.SMALL_SHAPES) == [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
    assert fc.shape_at_least((1 << 20) + 1) == (919, 1141) and fc.shape_at_most(1 << 20) == (1024, 1024)


@pytest.mark.parametrize("pattern", fc.PATTERNS)
def test_frame_patterns_do_what_their_names_say(pattern):
    h, w = 3, 4097
    raw = fc.frame(h, w, pattern, seed=1).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        alive = np.flatnonzero(raw[:, 0] > 0)
    n = h * w
    want = {"none": 0, "all": n, "first": 1, "last": 1, "first_of_last_chunk": 1}.get(pattern)
    if want is not None:
        assert len(alive) == want
    if pattern == "first_of_last_chunk":
        assert alive[0] == 3 * 4096 == (fc.chunks_of(n) - 1) * fc.COMPACT_CHUNK
    if pattern == "last":
        assert alive[0] == n - 1
    if pattern.startswith("d"):
        assert abs(len(alive) / n - float(pattern[1:])) < 0.02
    if pattern == "runs":
        np.testing.assert_array_equal(alive[:101], list(range(100)) + [137])
    if pattern == "specials":
        pos = fc.special_positions(n)
        assert {63, 64, 255, 256, 4095, 4096, 3 * 4096 - 1, 3 * 4096} <= set(pos.tolist())
        got = raw[pos, 0]
        for k, s in enumerate(fc.SPECIALS):
            np.testing.assert_array_equal(got[k::8].view(np.uint32), np.full(len(got[k::8]), s.view(np.uint32)))
        # numpy keeps the subnormal, FLT_MIN and +inf and drops the rest
        np.testing.assert_array_equal(fc.SPECIALS > 0, [False, False, True, True, False, False, True, False])
    if len(alive) >= 3:
        assert np.isnan(raw[alive[0], 2]) and raw[alive[-1], 2] == -np.inf and np.isnan(raw[alive[len(alive) // 2], 1])
