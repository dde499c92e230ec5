"""GPU: the kernels that run on a finished frame (raster_post.h) at every seam of their launch shapes, against the numpy
statements of tests/frame_cases.py (pinned to the reference's g12 tables by tests/test_frame_cases.py).  The frames are
installed with Mesh.load_image: no render is needed.  Every comparison is bit for bit -- both sides convert float32 to
float64 and add one float64 offset.

seam                                                          size that crosses it                        test
valid_count / valid_write: partial last chunk (4096 px)       1 .. 4097 px; last chunks of 1, 2 px         test_small_frames_*, test_large_frames
scan_counts_kernel: per = ceil(chunks / 1024) = 1 -> 2        1023, 1024 | 1025 chunks                     test_large_frames[c1023_* c1024_* c1025_*]
scan_counts_kernel: per = 2 -> 3                              2048 | 2049 chunks                           test_large_frames[c2048_* c2049_*]
scan_counts_kernel: extents joined over all 16 waves          the extent in the last sixteenth of 1023,    test_extent_in_the_last_sixteenth_of_the_chunks,
                                                              1024, 2048 chunks (wave 15 owns it there)    test_large_frames (last, first_of_last_chunk)
valid_write_kernel: idx beyond 2^22                           > 4 194 304 px                               test_large_frames[c1025_* c2048_* c2049_*]
width / height limit                                          1 x 32768, 32768 x 1, 128 x 32768            test_large_frames[row_* column_* c1024_width_limit]
compact_cap reuse (span moves with chunks)                    2049 -> 3 -> 2049 chunks on one mesh         test_one_mesh_serves_frames_of_changing_size
image_u8_kernel: second trip of the stride loop               cu_count * 4096 - 1, + 0, + 1.., * 2.5       test_fetch_u8_across_the_grid_stride
gather_pixels_kernel: last block partial                      n = 0, 1, 255, 256, 257, 100 001             test_gather
distance_mask_kernel: last block partial                      n = 1, 255, 256, 257, 1 000 001              test_distance_mask
table_columns_kernel: every array type and channel count      uint8, uint16, float32, float64 x 0, 1, 4, 64 test_table_columns_every_type_and_channel_count
"""
import ctypes

import numpy as np
import pytest

from tests import frame_cases as fc

pytestmark = pytest.mark.gpu

VERT = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1]], dtype=np.float32)       # any mesh: the frames are loaded


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def new_mesh(L):
    return L.Mesh(VERT, None, None, grid=(2, 2))


def same_bounds(got, want, what):
    """bit-equal, NaN == NaN, and no -0.0 for 0.0"""
    got, want = np.array(got, dtype=np.float64), np.array(want, dtype=np.float64)
    assert (got.view(np.uint64) == want.view(np.uint64))[~np.isnan(want)].all() and (np.isnan(got) == np.isnan(want)).all(), \
        f"{what}: bounds {got} != {want}"


def check_frame(m, raw, offsets, what, array=None, block_rows=2):
    """fetch_valid, fetch_valid_block, fetch_valid_table and rasterize_plan of the loaded frame against frame_cases"""
    with np.errstate(invalid="ignore"):
        idx, xyz, u, v, chan = fc.valid_table(raw, offsets, array)
        bounds = fc.valid_bounds(xyz)
    got_idx, got_xyz = m.fetch_valid(offsets)
    assert got_idx.dtype == np.uint32 and got_xyz.dtype == np.float64 and got_xyz.shape == (len(idx), 3), what
    np.testing.assert_array_equal(got_idx, idx, err_msg=what)
    np.testing.assert_array_equal(got_xyz, xyz, err_msg=what)
    del got_idx, got_xyz
    bidx, block = m.fetch_valid_block(offsets, extra_rows=block_rows)
    assert block.shape == (3 + block_rows, len(idx)), what
    np.testing.assert_array_equal(bidx, idx, err_msg=what)
    np.testing.assert_array_equal(block[:3], xyz.T, err_msg=what)
    del bidx, block
    if array is not None:
        labels, gu, gv, tab = m.fetch_valid_table(array, offsets)
        assert labels.dtype == np.int64 and gu.dtype == np.int16 and gv.dtype == np.int16, what
        assert tab.shape == (3 + array.shape[2], len(idx)) and tab.dtype == np.float64, what
        np.testing.assert_array_equal(labels, idx.astype(np.int64), err_msg=what)
        np.testing.assert_array_equal(gu, u, err_msg=what)
        np.testing.assert_array_equal(gv, v, err_msg=what)
        np.testing.assert_array_equal(tab[:3], xyz.T, err_msg=what)
        np.testing.assert_array_equal(tab[3:], chan, err_msg=what)
        del labels, gu, gv, tab
    n, got_bounds = m.rasterize_plan(offsets)
    assert n == len(idx), what
    same_bounds(got_bounds, bounds, what)
    if len(idx) == 0:
        assert np.isnan(got_bounds).all(), what
    return idx, xyz


@pytest.mark.parametrize("shape", fc.SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_frames_every_pattern(L, shape):
    h, w = shape
    rng = np.random.default_rng([5, h, w])
    body = fc.fill_channels(h, w, rng)
    array = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    seen = 0
    with new_mesh(L) as m:
        for pattern in fc.PATTERNS:
            raw = fc.set_pattern(body, pattern, rng).reshape(h, w, 3)
            m.load_image(raw)
            for off in (None, fc.UTM_OFFSETS):
                idx, _ = check_frame(m, raw, off, f"{h}x{w} {pattern} offsets={off is not None}", array)
                seen += len(idx)
    assert seen > 0


def test_specials_the_device_keeps_what_numpy_keeps(L):
    """every special value at every position of a wave, so that each meets each lane; the smallest subnormal and FLT_MIN are
    > 0 and stay in the table (a device that flushes subnormals would drop them), -0.0, NaN and -inf do not"""
    h, w = 8, 64
    raw = np.zeros((h, w, 3), dtype=np.float32)
    for r in range(h):
        raw[r, :, 0] = np.roll(np.tile(fc.SPECIALS, w // len(fc.SPECIALS)), r)
    raw[..., 1] = 7.0
    raw[..., 2] = 9.0
    with new_mesh(L) as m:
        m.load_image(raw)
        idx, xyz = check_frame(m, raw, None, "specials 8x64")
        assert len(idx) == h * w * 3 // 8
        assert (xyz[:, 0] == float(np.float32(1e-45))).sum() == h * w // 8
        _, xyz = check_frame(m, raw, fc.UTM_OFFSETS, "specials 8x64 with offsets")
        assert (xyz[:, 0] == fc.UTM_OFFSETS[0]).sum() == h * w // 4                     # both tiny values vanish in the sum


TABLE_DTYPES = [np.uint8, np.uint16, np.float32, np.float64]


@pytest.mark.parametrize("C", [0, 1, 4, 64])
@pytest.mark.parametrize("dtype", TABLE_DTYPES, ids=lambda d: np.dtype(d).name)
def test_table_columns_every_type_and_channel_count(L, dtype, C):
    with new_mesh(L) as m:
        for (h, w), pattern in [((1, 1), "all"), ((13, 5), "d0.5"), ((257, 1), "runs"), ((63, 65), "d0.5"), ((17, 241), "runs"),
                                ((17, 241), "none")]:
            rng = np.random.default_rng([6, h, w, C])
            raw = fc.frame(h, w, pattern, seed=C)
            if np.issubdtype(dtype, np.integer):
                array = rng.integers(0, np.iinfo(dtype).max, (h, w, C), dtype=dtype, endpoint=True)
            else:
                array = (rng.normal(0, 1e4, (h, w, C))).astype(dtype)
                if array.size > 2:
                    array.reshape(-1)[[0, -1]] = [np.nan, -np.inf]
            m.load_image(raw)
            for off in (None, fc.UTM_OFFSETS):
                check_frame(m, raw, off, f"{h}x{w} {pattern} {np.dtype(dtype).name} C={C}", array, block_rows=C)


# pattern subsets at the large shapes: the cheap single-survivor patterns everywhere (they are the ones that put the frame's
# extent and the scan's last entries into the last chunk), half density everywhere, the full tables where they say most
LARGE_PATTERNS = {
    "c1023_full": ["last", "d0.5"], "c1023_one": ["first_of_last_chunk", "runs"],
    "c1024_full": ["none", "last", "d0.5"], "c1024_one": ["first_of_last_chunk", "d0.999"],
    "c1025_full": ["last", "runs"], "c1025_one": ["first_of_last_chunk", "first", "d0.5"],
    "c2048_full": ["last", "specials"], "c2048_one": ["first_of_last_chunk", "d0.5"],
    "c2049_full": ["last", "all"], "c2049_two": ["first_of_last_chunk", "d0.001", "specials"],
    "row_1x32768": fc.PATTERNS, "column_32768x1": fc.PATTERNS,
    "c1024_width_limit": ["last", "first_of_last_chunk", "d0.5"],
}


@pytest.mark.parametrize("name", list(fc.LARGE_SHAPES))
def test_large_frames(L, name):
    h, w = fc.LARGE_SHAPES[name]
    rng = np.random.default_rng([7, h, w])
    body = fc.fill_channels(h, w, rng)
    array = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    with new_mesh(L) as m:
        for k, pattern in enumerate(LARGE_PATTERNS[name]):
            raw = fc.set_pattern(body, pattern, rng).reshape(h, w, 3)
            m.load_image(raw)
            off = fc.UTM_OFFSETS if k % 2 == 0 else None
            # the full table at the densities that leave it small; fetch_valid, the block and the plan always
            dense = pattern in ("all", "d0.999", "d0.5", "runs", "specials") and h * w > (1 << 20)
            idx, xyz = check_frame(m, raw, off, f"{name} {h}x{w} {pattern}", None if dense else array, block_rows=1)
            if pattern in ("last", "first_of_last_chunk"):
                assert len(idx) == 1 and fc.chunks_of(int(idx[0]) + 1) == fc.LARGE_CHUNKS[name][0]
            # a lookup on the same frame: corners, the last chunk, random pixels
            u = np.concatenate([[0, w - 1, 0, w - 1, w, -1], rng.integers(-2, w + 2, 500)])
            v = np.concatenate([[0, 0, h - 1, h - 1, h - 1, 0], rng.integers(-2, h + 2, 500)])
            np.testing.assert_array_equal(m.gather(u, v, off), fc.gather(raw, u, v, off), err_msg=f"{name} {pattern}")


def test_extent_in_the_last_sixteenth_of_the_chunks(L):
    """scan_counts_kernel joins the chunks' extents over its 16 waves: with 2048 chunks every thread owns two and wave 15 the
    last 128 (with 2049 a thread owns three and the waves from 11 on own none).  The frame's x maximum and y minimum sit in
    wave 15's chunks, the x minimum and y maximum in wave 0's"""
    h, w = fc.LARGE_SHAPES["c2048_full"]
    raw = fc.frame(h, w, "d0.5", seed=3).reshape(-1, 3)
    raw[:, 0] = np.where(raw[:, 0] > 0, np.float32(500.0), raw[:, 0])
    raw[:, 2] = np.float32(100.0)
    a, b = 5, h * w - 5
    raw[a] = [0.5, 0.0, 900.0]
    raw[b] = [900.0, 0.0, -3.0]
    assert fc.chunks_of(h * w) == 2048 and fc.chunks_of(b + 1) - 1 >= 960 * 2
    raw = raw.reshape(h, w, 3)
    with new_mesh(L) as m:
        m.load_image(raw)
        for off in (None, fc.UTM_OFFSETS):
            n, bounds = m.rasterize_plan(off)
            ox, oy = (0.0, 0.0) if off is None else (off[0], off[2])
            assert n == int((raw[..., 0] > 0).sum())
            assert bounds == (0.5 + ox, -3.0 + oy, 900.0 + ox, 900.0 + oy)


GATHER_N = [0, 1, 255, 256, 257, 100_001]


@pytest.mark.parametrize("n", GATHER_N)
def test_gather(L, n):
    h, w = 301, 517
    raw = fc.frame(h, w, "d0.5", seed=11)
    rng = np.random.default_rng([12, n])
    u = rng.integers(-3, w + 3, n).astype(np.int64)
    v = rng.integers(-3, h + 3, n).astype(np.int64)
    i32 = np.iinfo(np.int32)
    edge_u = [-1, w, 0, 0, i32.min, i32.max, 0, 0, w - 1, i32.min, i32.max, 65536 + 1, 1]
    edge_v = [0, 0, -1, h, 0, 0, i32.min, i32.max, h - 1, i32.min, i32.max, 1, 65536 + 1]
    k = min(n, len(edge_u))
    u[:k], v[:k] = edge_u[:k], edge_v[:k]
    flat = raw.reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        alive = np.flatnonzero(flat[:, 0] > 0)
    if n > 20:                                        # the survivors that carry NaN / -inf, and a pixel that is not valid
        dead = np.flatnonzero(~(flat[:, 0] > 0))[7]
        for j, p in enumerate([alive[0], alive[-1], alive[len(alive) // 2], dead]):
            u[14 + j], v[14 + j] = p % w, p // w
    with new_mesh(L) as m:
        m.load_image(raw)
        for off in (None, fc.UTM_OFFSETS):
            got = m.gather(u, v, off)
            want = fc.gather(raw, u, v, off)
            assert got.shape == (n, 3) and got.dtype == np.float64
            np.testing.assert_array_equal(got, want)
    if n > 20:
        assert np.isnan(want[14, 1]) and not np.isnan(want[14, 0]) and want[15, 1] == -np.inf and np.isnan(want[16, 2])
        assert np.isnan(want[17]).all() and np.isnan(want[:8]).all()
        assert 0.3 < (~np.isnan(want[:, 0])).mean() < 0.6


def test_one_mesh_serves_frames_of_changing_size(L):
    """compact_cap: the count and offset buffers made for 2049 chunks serve a frame of 3 chunks (the extents then sit behind
    3 counts, not 2049) and the large one again -- each time what a fresh mesh gives"""
    big_shape, small_shape = fc.LARGE_SHAPES["c2049_two"], (3, 4000)
    big = fc.frame(*big_shape, "d0.001", seed=21)
    small = fc.frame(*small_shape, "runs", seed=22)
    assert fc.chunks_of(big.shape[0] * big.shape[1]) == 2049 and fc.chunks_of(3 * 4000) == 3
    fresh = {}
    for name, raw in (("big", big), ("small", small)):
        with new_mesh(L) as f:
            f.load_image(raw)
            idx, xyz = f.fetch_valid(fc.UTM_OFFSETS)
            fresh[name] = (idx.copy(), xyz.copy(), f.rasterize_plan(fc.UTM_OFFSETS))
            del idx, xyz
    with new_mesh(L) as m:
        for name, raw in (("big", big), ("small", small), ("big", big)):
            m.load_image(raw)
            idx, xyz = check_frame(m, raw, fc.UTM_OFFSETS, f"reused mesh, {name}")
            np.testing.assert_array_equal(idx, fresh[name][0])
            np.testing.assert_array_equal(xyz, fresh[name][1])
            n, bounds = m.rasterize_plan(fc.UTM_OFFSETS)
            assert n == fresh[name][2][0]
            same_bounds(bounds, fresh[name][2][1], name)


def test_a_second_load_invalidates_the_count_and_the_plan(L):
    raw = fc.frame(40, 50, "d0.5", seed=31)
    other = fc.frame(30, 20, "d0.5", seed=32)
    array = np.zeros((30, 20, 1), dtype=np.uint8)
    with new_mesh(L) as m:
        m.load_image(raw)
        n = ctypes.c_int64()
        L.check(m._lib.alp_render_valid_count(m._h, ctypes.byref(n)))
        assert n.value == int((raw[..., 0] > 0).sum())
        m.load_image(other)                                        # the count belonged to the frame before
        idx = np.empty(n.value, dtype=np.uint32)
        xyz = np.empty((n.value, 3), dtype=np.float64)
        with pytest.raises(L.AlprojHipError, match="call alp_render_valid_count first"):
            L.check(m._lib.alp_render_fetch_valid(m._h, None, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), L.as_dp(xyz)))
        m.load_image(raw)
        assert m.rasterize_plan(None)[0] == n.value
        m.load_image(other)                                        # ... and so did the plan
        with pytest.raises(L.AlprojHipError, match="call alp_render_rasterize_plan for this frame first"):
            m.rasterize(array, [0], 0.0, 100.0, 1.0, 8, 8, 0, 0, 255)
        # and the frame now loaded is served as if nothing had happened
        check_frame(m, other, fc.UTM_OFFSETS, "after the refusals")


def wild_colours(h, w, rng):
    """values in [-2, 300] / 255 plus NaN, +-inf, +-3e9 sprinkled over every residue of 256 pixels"""
    raw = (rng.random((h, w, 3), dtype=np.float32) * np.float32(302.0) - np.float32(2.0)) / np.float32(255.0)
    flat = raw.reshape(-1)
    pos = rng.integers(0, flat.size, 4000)
    flat[pos] = np.array([np.nan, np.inf, -np.inf, 3e9, -3e9], dtype=np.float32)[np.arange(4000) % 5]
    flat[[0, -1]] = [np.nan, -3e9]
    return raw


@pytest.mark.parametrize("where", ["one_short", "exact", "one_over", "two_and_a_half_trips"])
def test_fetch_u8_across_the_grid_stride(L, where):
    """image_u8_kernel runs cu_count * 16 blocks of 256: one trip of its stride loop covers cu_count * 4096 pixels"""
    trip = L.device_info()["cu_count"] * 4096
    h, w = {"one_short": fc.shape_at_most(trip - 1), "exact": fc.shape_at_most(trip), "one_over": fc.shape_at_least(trip + 1),
            "two_and_a_half_trips": fc.shape_at_least(trip * 5 // 2)}[where]
    n = h * w
    assert {"one_short": n < trip, "exact": n <= trip, "one_over": n > trip, "two_and_a_half_trips": 2 * trip < n < 3 * trip}[where]
    if where != "two_and_a_half_trips":
        assert abs(n - trip) <= 64, (n, trip)          # as close to the seam as a frame shape comes
    raw = wild_colours(h, w, np.random.default_rng([41, h, w]))
    with new_mesh(L) as m:
        m.load_image(raw)
        for scale in (255.0, 1.0):
            for reverse in (True, False):
                got = m.fetch_u8(scale, reverse)
                assert got.dtype == np.uint8 and got.shape == (h, w, 3)
                np.testing.assert_array_equal(got, fc.image_u8(raw, scale, reverse), err_msg=f"scale {scale} reverse {reverse}")
                del got


CAM = np.array([732731.25, 4051171.5, 2458.125])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1_000_001])
def test_distance_mask(L, n):
    """test_gpu_gcp.py's cases at every block seam, plus rows at exactly lo and exactly hi: 64 * (3, 4, 0) and
    128 * (0, 3, 4) from the camera, whose squares, sum and root (320 and 640) are exact"""
    rng = np.random.default_rng([3, n])
    xyz = CAM + rng.normal(0, 1500, (n, 3))
    xyz[::97, 1] = np.nan
    exact = np.array([CAM + [192.0, 256.0, 0.0], CAM + [0.0, -384.0, 512.0], CAM + [-192.0, 0.0, -256.0]])
    k = min(n, 3)
    xyz[n - k:] = exact[:k]                                   # the last rows: the last, partial block
    assert (xyz[n - k:] - CAM == exact[:k] - CAM).all()
    with np.errstate(invalid="ignore"):
        d = np.sqrt((xyz[:, 0] - CAM[0]) ** 2 + (xyz[:, 1] - CAM[1]) ** 2 + (xyz[:, 2] - CAM[2]) ** 2)
    assert d[n - k] == 320.0
    ok = ~np.isnan(xyz).any(1)
    lo, hi = float(np.nanquantile(d, 0.3)), float(np.nanquantile(d, 0.8))
    lo, hi = float(d[ok][np.argmin(np.abs(d[ok] - lo))]), float(d[ok][np.argmin(np.abs(d[ok] - hi))])    # exact distances of two rows
    up, down = np.nextafter(320.0, np.inf), np.nextafter(640.0, 0.0)
    cases = [(lo, None), (None, hi), (lo, hi), (None, None), (0.0, 0.0),
             (320.0, 640.0), (up, 640.0), (320.0, down), (320.0, 320.0), (640.0, 640.0)]
    for a, b in cases:
        want = fc.distance_keep(xyz, CAM, a, b)
        np.testing.assert_array_equal(L.distance_mask(xyz, CAM, a, b), want, err_msg=f"n {n} lo {a} hi {b}")
    tail = n - k
    assert fc.distance_keep(xyz, CAM, 320.0, 640.0)[tail] and not fc.distance_keep(xyz, CAM, up, 640.0)[tail]
    if n >= 3:
        assert fc.distance_keep(xyz, CAM, 320.0, 640.0)[tail + 1] and not fc.distance_keep(xyz, CAM, 320.0, down)[tail + 1]
        assert fc.distance_keep(xyz, CAM, 320.0, 320.0)[[tail, tail + 2]].all()
