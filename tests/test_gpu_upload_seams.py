"""GPU: mesh creation across its staging chunks and round seams (alp_raster.hip: upload_f32, upload_indices,
streamed_grid_check, try_subgrid; the kernels of raster_post.h).

seam                                                               size that crosses it                      test
cast_f64_f32_kernel via upload_f32: chunks of 24 << 20 doubles     2897 x 2897 = 8 392 609 vertices          test_float64_vertices_and_values_across_the_staging_chunk
= 8 388 608 vertices, dst_off > 0 from the second on
narrow_indices_kernel via upload_indices: 24 << 20 int64 values    8 393 608 triangles, real ones at the     test_int64_indices_across_the_staging_chunk
= 8 388 608 triangles                                              start, across the seam and at the end     test_out_of_range_index_in_the_second_chunk_is_named
check_grid_chunk_kernel via streamed_grid_check: 192 MB of whole   int64: 2050 x 2049 grid = 8 392 704,      test_streamed_grid_check_across_its_chunk
triangles = 8 388 608 int64 or 16 777 216 int32, t0 > 0            int32: 2898 x 2898 = 16 785 218 triangles
subgrid_mark_kernel: cu_count * 8 blocks of 256, rounds k >= 1     1.5 .. 2.5 x cu_count * 2048 triangles    test_filtered_grid_beyond_one_round,
(predecessor by shuffle, lane 0 re-reads ind[t - 1])               defects at t = cu_count * 2048            test_defect_at_the_first_triangle_of_round_one
"""
import numpy as np
import pytest

from alproj_amd import synthetic as syn
from oracle import raster as orast
from tests import frame_cases as fc

pytestmark = pytest.mark.gpu

STAGE_VALUES = 24 << 20               # upload_f32, upload_indices: 8-byte values per staging chunk
STAGE_TRI = STAGE_VALUES // 3         # = 8 388 608 vertices or int64 triangles; the grid check's int32 chunk holds twice that


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def first_difference(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} rows differ, the first at index {bad[0]} (chunk {bad[0] // STAGE_TRI}, " \
                          f"{bad[0] % STAGE_TRI} in it): {got[bad[0]]} != {want[bad[0]]}"


def test_float64_vertices_and_values_across_the_staging_chunk(L):
    side = 2897
    n = side * side
    assert STAGE_TRI < n < STAGE_TRI + 5000
    rng = np.random.default_rng(51)
    vert = rng.random((n, 3)) * 4000.0 + 1.0 / 3.0
    value = rng.random((n, 3))
    assert (vert.astype(np.float32) != vert).mean() > 0.99                  # not float32-representable: the cast rounds
    with L.Mesh(vert, value, None, grid=(side, side)) as m:
        got_vert, got_value, valid = m.fetch_arrays()
        first_difference(got_vert, vert.astype(np.float32), "vert")
        first_difference(got_value, value.astype(np.float32), "value")
        assert valid.all()


def scattered_scene():
    """a 64 x 64 surface whose 7938 triangles sit in three runs of an index array of STAGE_TRI + 5000 triangles -- at the
    start, across position STAGE_TRI and at the end -- between degenerate triangles [v, v, v].  The triangle AT position
    STAGE_TRI, the first of the second staging chunk, is one the camera sees."""
    n = 64
    s = syn.surface(n)
    real = syn.grid_indices(n)
    p = syn.base_params(n)
    p.update(w=320, h=200, cx=160.0, cy=100.0, tilt=-20.0, z=p["z"] + 30)
    alone = orast.visibility(s["vert"], real, p, s["offsets"])
    seen = np.unique(0xFFFFFFFF - (alone[alone != 0] & np.uint64(0xFFFFFFFF)).astype(np.int64))
    T = STAGE_TRI + 5000
    ind = np.empty((T, 3), dtype=np.int64)
    ind[:] = (np.arange(T, dtype=np.int64) % (n * n))[:, None]
    third = len(real) // 3
    mid = seen[(seen >= third + 500) & (seen < 2 * third - 500)]
    at_seam = int(mid[len(mid) // 2])                          # a visible triangle of the middle run
    starts = [0, STAGE_TRI - (at_seam - third), T - (len(real) - 2 * third)]
    parts = [real[:third], real[third:2 * third], real[2 * third:]]
    for at, part in zip(starts, parts):
        ind[at:at + len(part)] = part
    assert starts[1] < STAGE_TRI < starts[1] + third and starts[2] > STAGE_TRI and len(real) == 7938
    assert (ind[STAGE_TRI] == real[at_seam]).all()
    return s, ind, p, starts


def test_int64_indices_across_the_staging_chunk(L, monkeypatch):
    monkeypatch.setenv("ALP_NO_GRID_DETECT", "1")
    s, ind, p, starts = scattered_scene()
    ref = orast.visibility(s["vert"], ind, p, s["offsets"])
    tri = 0xFFFFFFFF - (ref[ref != 0] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    for k, at in enumerate(starts):                                           # every run is seen, on both sides of the seam
        assert ((tri >= at) & (tri < at + 2646)).sum() > 500, k
    assert (tri == STAGE_TRI).any()                 # the first triangle of the second chunk owns pixels
    pv = L.params_vector(p)
    with L.Mesh(s["vert"], None, ind) as m:
        info = m.info()
        assert not info["implicit"] and info["n_tri"] == len(ind)
        m.render_enqueue(pv, s["offsets"])
        np.testing.assert_array_equal(m.fetch_visibility(), ref)
    ind32 = ind.astype(np.int32)
    with L.Mesh(s["vert"], None, ind32) as m:
        m.render_enqueue(pv, s["offsets"])
        np.testing.assert_array_equal(m.fetch_visibility(), ref)


def test_out_of_range_index_in_the_second_chunk_is_named(L, monkeypatch):
    monkeypatch.setenv("ALP_NO_GRID_DETECT", "1")
    s, ind, p, starts = scattered_scene()
    n_vert = len(s["vert"])
    for value in (n_vert, -1):
        bad = ind.copy()
        at = 3 * (STAGE_TRI + 100) + 1
        bad.reshape(-1)[at] = value
        with pytest.raises(L.AlprojHipError, match=f"index {value} out of range at {at}$"):
            L.Mesh(s["vert"], None, bad)
        del bad


@pytest.mark.parametrize("dtype,gh,gw", [(np.int64, 2050, 2049), (np.int32, 2898, 2898)], ids=["int64", "int32"])
def test_streamed_grid_check_across_its_chunk(L, monkeypatch, dtype, gh, gw):
    monkeypatch.setenv("ALP_HOST_THREADS", "0")               # the check runs on the device while the array streams
    chunk_tri = (192 << 20) // np.dtype(dtype).itemsize // 3
    ind = fc.grid_triangles(gh, gw, dtype)
    assert chunk_tri < len(ind) < chunk_tri + 10000 and ind.dtype == dtype
    vert = np.zeros((gh * gw, 3), dtype=np.float32)
    with L.Mesh(vert, None, ind) as m:
        assert m.info() == dict(implicit=True, grid_h=gh, grid_w=gw, n_tri=len(ind))
    # one index of the second chunk names another valid vertex: the array is not the grid and is kept as it is
    for t, k in ((chunk_tri, 0), (len(ind) - 1, 2)):
        other = ind.copy()
        other[t, k] -= 1
        with L.Mesh(vert, None, other) as m:
            assert m.info() == dict(implicit=False, grid_h=0, grid_w=0, n_tri=len(ind)), (t, k)
        del other


_ROUND_CASE = {}


def round_case(L):
    """_filtered_case of test_gpu_surface.py at a side where the kept array has about 1.65 times the cu_count * 2048
    triangles one round of subgrid_mark_kernel takes"""
    from tests.test_gpu_surface import _filtered_case
    one_round = L.device_info()["cu_count"] * 8 * 256
    if one_round in _ROUND_CASE:
        return _ROUND_CASE[one_round]
    side = int(round(np.sqrt(one_round * 0.93)))              # 2 (side - 1)^2 triangles, 0.96^3 of them kept
    s, vvalid, full, kept, p = _filtered_case(n=side)
    assert 1.5 <= len(kept) / one_round <= 2.5, (side, len(kept), one_round)
    _ROUND_CASE[one_round] = (s, vvalid, full, kept, p, one_round)
    return _ROUND_CASE[one_round]


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["int32", "int64"])
def test_filtered_grid_beyond_one_round(L, dtype):
    s, vvalid, full, kept, p, one_round = round_case(L)
    ref = orast.visibility(s["vert"], kept, p, s["offsets"])                 # ids = positions in the caller's array
    derived = np.zeros(len(vvalid), dtype=bool)
    derived[kept.ravel()] = True
    with L.Mesh(s["vert"], None, kept.astype(dtype)) as m:
        info = m.info()
        assert info["implicit"] and info["grid_h"] == info["grid_w"] == s["n_side"]
        np.testing.assert_array_equal(m.fetch_arrays()[2], derived)
        assert not derived.all()
        m.render_enqueue(L.params_vector(p), s["offsets"])
        np.testing.assert_array_equal(m.fetch_visibility(), ref)
    tri = 0xFFFFFFFF - (ref[ref != 0] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (ref != 0).mean() > 0.3 and (tri >= one_round).any() and (tri < one_round).any()


@pytest.mark.parametrize("defect", ["swapped", "duplicate", "foreign"])
def test_defect_at_the_first_triangle_of_round_one(L, defect):
    """t = cu_count * 2048 is lane 0 of block 0 in round 1: its predecessor is the last lane of the last block of round 0, no
    shuffle reaches it"""
    s, vvalid, full, kept, p, one_round = round_case(L)
    t = one_round
    ind = kept.copy()
    if defect == "swapped":
        ind[[t - 1, t]] = ind[[t, t - 1]]
    elif defect == "duplicate":
        ind[t] = ind[t - 1]
    else:
        ind[t] = [0, 5, 4000]
    ref = orast.visibility(s["vert"], ind, p, s["offsets"])
    with L.Mesh(s["vert"], None, ind) as m:
        info = m.info()
        assert not info["implicit"] and info["n_tri"] == len(ind)
        assert m.fetch_arrays()[2].all()                                          # no mask: not converted
        m.render_enqueue(L.params_vector(p), s["offsets"])
        np.testing.assert_array_equal(m.fetch_visibility(), ref)
