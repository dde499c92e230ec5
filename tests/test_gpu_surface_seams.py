"""alp_mesh_from_rasters (surface_zmin_kernel + surface_build_kernel, alp_mesh.hip) at the seams of its launches and at
the edges of its elevation and colour arithmetic, against tests/surface_cases.py -- the numpy statement of the reference's
get_colored_surface that tests/test_surface_cases.py pins to the reference's own arrays (g11).

Shapes are derived from the device's CU count: three (two) turns of the minimum kernel's grid-stride loop with the last
one partial, odd rows wider than 1000 vertices, every tail length.  Every comparison is exact."""
import warnings

import numpy as np
import pytest

from alproj_amd import synthetic as syn
from oracle import raster as orast
from tests import frame_cases as fc
from tests import surface_cases as sc

pytestmark = pytest.mark.gpu

DSM_TYPES = [np.float32, np.float64]
Z_MAX = 1540.0                               # a value of both DSM types, as surface.py:169 always passes one
DIVISOR = {np.uint8: 255.0, np.uint16: 65535.0, np.float32: 0.0}


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def cu(L):
    return L.device_info()["cu_count"]


def built(L, dsm, t, z_max, aerial, div, nodata=None):
    mesh, off = L.Mesh.from_rasters(dsm, t, z_max, aerial, div, nodata)
    with mesh:
        return mesh.fetch_arrays() + (off,)


def same(got, want):
    """(vert, col, valid, offsets) of the device against the statement's"""
    for g, w, what in zip(got, want, ("vert", "col", "valid", "offsets")):
        np.testing.assert_array_equal(g, w, err_msg=what)


def rough(rows, cols, dtype, seed):
    """elevations around 1500 m of which ~9 % lie above Z_MAX and 0.5 % below zero: both clamps act"""
    rng = np.random.default_rng(seed)
    dsm = 1500.0 + rng.normal(0, 30, (rows, cols))
    dsm[rng.random((rows, cols)) < 0.005] = -5.0
    return dsm.astype(dtype)


# ------------------------------------------------------------------ a. every instantiation at the three-turn shape
FULL = [(np.float32, np.uint8, 1, "north_up"), (np.float32, np.uint16, 2, "south_up"), (np.float32, np.float32, 3, "west_up"),
        (np.float64, np.uint8, 1, "half"), (np.float64, np.uint16, 1, "fine"), (np.float64, np.float32, 1, "north_up")]


@pytest.mark.parametrize("dsm_dtype,aerial_dtype,rem,tname", FULL,
                         ids=[f"{np.dtype(d).name}-{np.dtype(a).name}-tail{r}-{t}" for d, a, r, t in FULL])
def test_three_turn_raster_equals_the_reference_statement(L, cu, dsm_dtype, aerial_dtype, rem, tname):
    itemsize = np.dtype(dsm_dtype).itemsize
    rows, cols = sc.seam_shapes(itemsize, cu)[rem]
    n = rows * cols
    assert sc.zmin_slot(n - rem - 1, n, itemsize, cu)[0] == 2 and n % sc.pack_len(itemsize) == rem
    dsm = rough(rows, cols, dsm_dtype, seed=rem)
    aerial = sc.aerial_bands(rows, cols, aerial_dtype, seed=rem)
    nodata = np.random.default_rng(50 + rem).random((rows, cols)) < 0.05
    t = sc.transform(tname, rows, cols)
    want = sc.expected(dsm, t, Z_MAX, aerial, DIVISOR[aerial_dtype], nodata)
    assert want[3][1] == 0.0 and want[0][:, 1].max() == np.float32(Z_MAX)              # both clamps decide the extremes
    same(built(L, dsm, t, Z_MAX, aerial, DIVISOR[aerial_dtype], nodata), want)


@pytest.mark.parametrize("tname", ["north_up", "west_up", "fine"])
@pytest.mark.parametrize("shape", sc.SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dsm_dtype", DSM_TYPES, ids=lambda d: np.dtype(d).name)
def test_smallest_rasters(L, dsm_dtype, shape, tname):
    """n = 4, 6, 9: one pack and no tail, a tail of 2 (float32), a tail of 1; no nodata mask at all"""
    rows, cols = shape
    dsm = rough(rows, cols, dsm_dtype, seed=rows * cols)
    dsm[-1, -1] = 1400.0                                                   # the minimum in the tail, where there is one
    aerial = sc.aerial_bands(rows, cols, np.uint8, seed=3)
    t = sc.transform(tname, rows, cols)
    want = sc.expected(dsm, t, Z_MAX, aerial, 255.0)
    assert want[3][1] == 1400.0 and want[2].all()
    same(built(L, dsm, t, Z_MAX, aerial, 255.0), want)


# ------------------------------------------------------------------ b. one lowest elevation in every slot of the launch
@pytest.fixture(scope="module", params=DSM_TYPES, ids=lambda d: np.dtype(d).name)
def sweep(request, cu):
    dtype = request.param
    itemsize = np.dtype(dtype).itemsize
    rows, cols = sc.seam_shapes(itemsize, cu)[1]
    dsm = sc.terrain(rows, cols, dtype, seed=7)                            # everything above 1500, nothing clamped
    aerial = sc.aerial_bands(rows, cols, np.uint8, seed=7)
    nodata = np.random.default_rng(8).random((rows, cols)) < 0.05
    t = sc.transform("north_up", rows, cols)
    want = sc.expected(dsm, t, Z_MAX, aerial, 255.0, nodata)
    for a in (dsm, aerial, nodata) + want:
        a.flags.writeable = False
    return dict(dsm=dsm, aerial=aerial, nodata=nodata, t=t, want=want, itemsize=itemsize,
                pos=sc.min_positions(rows * cols, itemsize, cu))


@pytest.mark.parametrize("where", sc.POSITIONS)
def test_the_minimum_is_found_in_every_slot(L, cu, sweep, where):
    """base + noise with ONE strictly lowest elevation: offsets[1] and the whole height column depend on the lane that reads
    it.  The other columns, the colours and the mask do not: they are held to the statement of the unchanged raster."""
    i = sweep["pos"][where]
    dsm = sweep["dsm"].copy()
    assert dsm.min() > 1500.0
    dsm.flat[i] = 1400.0
    zz = sc.clamped_z(dsm, Z_MAX).ravel()                                  # surface.py:175-176, then :211-212 on this column
    assert zz.min() == 1400.0 and np.flatnonzero(zz == zz.min()).tolist() == [i]
    vert, col, valid, off = built(L, dsm, sweep["t"], Z_MAX, sweep["aerial"], 255.0, sweep["nodata"])
    slot = sc.zmin_slot(i, dsm.size, sweep["itemsize"], cu)
    assert off[1] == 1400.0, f"{where}: element {i} = (turn, workgroup, wave, tail) {slot}"
    np.testing.assert_array_equal(vert[:, 1], (zz - zz.min()).astype(np.float32))
    want_vert, want_col, want_valid, want_off = sweep["want"]
    np.testing.assert_array_equal(off[[0, 2]], want_off[[0, 2]])
    np.testing.assert_array_equal(vert[:, [0, 2]], want_vert[:, [0, 2]])
    np.testing.assert_array_equal(col, want_col)
    np.testing.assert_array_equal(valid, want_valid)


# ------------------------------------------------------------------ c. elevation edges
EDGES = ["all_negative", "all_above", "min_equals_zmax", "zmax_zero", "plus_inf", "negzero_alone", "negzero_then_zero",
         "zero_then_negzero", "negzero_everywhere", "nan"]


def edge_raster(case, rows, cols, dtype, at):
    """-> (dsm, z_max); ``at``: the element the case turns on (in the second turn of a two-turn raster, alone in its
    workgroup there)"""
    V = sc.pack_len(np.dtype(dtype).itemsize)
    dsm = sc.terrain(rows, cols, dtype, seed=21)                           # (1500, 1530)
    flat = dsm.reshape(-1)
    z_max = Z_MAX
    if case == "all_negative":
        dsm *= -1
    elif case == "all_above":
        dsm += 100
    elif case == "min_equals_zmax":
        flat[at] = 1500.0
        z_max = 1500.0
    elif case == "zmax_zero":
        z_max = 0.0
    elif case == "plus_inf":
        flat[np.random.default_rng(22).random(flat.size) < 0.01] = np.inf
        flat[:V] = np.inf                                                  # a whole pack, the tail, the chosen element
        flat[-1] = flat[at] = np.inf
        z_max = 1520.0
    elif case == "negzero_alone":
        flat[at] = -0.0
    elif case in ("negzero_then_zero", "zero_then_negzero"):               # both in one pack of one lane, in either order
        a = at // V * V
        flat[a:a + 2] = [-0.0, 0.0] if case == "negzero_then_zero" else [0.0, -0.0]
    elif case == "negzero_everywhere":
        flat[:] = -0.0
    elif case == "nan":
        flat[np.random.default_rng(23).random(flat.size) < 0.01] = np.nan
        a = at // V * V
        flat[0] = flat[-1] = np.nan
        flat[a:a + V] = np.nan                                             # a whole pack of NaN ...
        flat[at] = 1400.0                                                  # ... but for the minimum itself
    return dsm, z_max


@pytest.mark.parametrize("case", EDGES)
@pytest.mark.parametrize("size", ["two_turns", "3x3"])
@pytest.mark.parametrize("dsm_dtype", DSM_TYPES, ids=lambda d: np.dtype(d).name)
def test_elevation_edges(L, cu, dsm_dtype, size, case):
    itemsize = np.dtype(dsm_dtype).itemsize
    if size == "3x3":
        rows, cols, at = 3, 3, 4
    else:
        rows, cols = sc.seam_shapes(itemsize, cu, turns=2)[1]
        at = sc.min_positions(rows * cols, itemsize, cu)["turn1"]
        assert sc.zmin_slot(at, rows * cols, itemsize, cu) == (1, 7, 1, False)
    dsm, z_max = edge_raster(case, rows, cols, dsm_dtype, at)
    aerial = sc.aerial_bands(rows, cols, np.uint8, seed=24)
    t = sc.transform("north_up" if dsm_dtype == np.float32 else "fine", rows, cols)
    got = built(L, dsm, t, z_max, aerial, 255.0)
    if case == "nan":
        # the kernel's minimum skips a NaN where numpy's returns it: offsets are the nanmin, a
        # NaN elevation is a NaN vertex height and every other value is what the statement gives with that offset
        zz = sc.clamped_z(dsm, z_max).ravel()
        assert np.isnan(zz).sum() >= 3 and np.nanmin(zz) == 1400.0
        want = sc.expected(np.where(np.isnan(dsm), dsm_dtype(1510.0), dsm), t, z_max, aerial, 255.0)
        assert got[3][1] == 1400.0
        np.testing.assert_array_equal(np.isnan(got[0][:, 1]), np.isnan(zz))
        np.testing.assert_array_equal(got[0][:, 1], (zz - 1400.0).astype(np.float32))          # NaN == NaN here
        np.testing.assert_array_equal(got[0][:, [0, 2]], want[0][:, [0, 2]])
        same((want[0],) + got[1:], want)
        return
    want = sc.expected(dsm, t, z_max, aerial, 255.0)
    assert np.isfinite(want[0]).all() and np.isfinite(want[3]).all()
    flat = {"all_negative": 0.0, "all_above": Z_MAX, "min_equals_zmax": 1500.0, "zmax_zero": 0.0, "negzero_everywhere": 0.0}
    if case in flat:
        assert want[3][1] == flat[case] and not want[0][:, 1].any()
    if case.startswith(("negzero", "zero")):
        assert want[3][1] == 0.0
        assert got[3][1] == 0.0 and np.isfinite(got[0][:, 1]).all(), (got[3], got[0][:3, 1])
    same(got, want)


# ------------------------------------------------------------------ d. colour edges
def edge_aerial(dtype, rows, cols, scale):
    rng = np.random.default_rng(31)
    if dtype == np.float32:
        a = ((rng.random((3, rows, cols)) * 1.4 - 0.2) * scale).astype(np.float32)     # below 0 and above the divisor
        specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 255.0, 256.0, 1e30, -1e30, 1e-45, np.nextafter(1, 2)],
                            dtype=np.float32)
        flat = a.reshape(-1)
        where = np.concatenate([np.arange(12), flat.size - 1 - np.arange(12), rng.choice(flat.size, 1200, replace=False)])
        flat[where] = np.resize(specials, len(where))
        return a
    a = rng.integers(0, int(np.iinfo(dtype).max) + 1, (3, rows, cols), dtype=dtype)
    a[:, 0, 0], a[:, -1, -1], a[:, 0, 1], a[:, -1, -2] = 0, np.iinfo(dtype).max, np.iinfo(dtype).max, 0
    return a


COLOURS = [(np.float32, np.float32, 0.0), (np.float64, np.float32, 255.0), (np.float32, np.uint16, 65535.0),
           (np.float64, np.uint16, 4095.0), (np.float64, np.uint8, 255.0), (np.float32, np.uint8, 0.0)]


@pytest.mark.parametrize("dsm_dtype,aerial_dtype,div", COLOURS,
                         ids=[f"{np.dtype(d).name}-{np.dtype(a).name}-div{int(v)}" for d, a, v in COLOURS])
def test_colour_edges(L, dsm_dtype, aerial_dtype, div):
    """numpy's float64 divide, np.clip (which keeps a NaN), the float32 cast: a divisor of 0 divides nothing, 4095 leaves
    most of a 16-bit raster above 1"""
    rows, cols = 67, 1031
    aerial = edge_aerial(aerial_dtype, rows, cols, div if div > 0 else 1.0)
    dsm = sc.terrain(rows, cols, dsm_dtype, seed=32)
    t = sc.transform("south_up", rows, cols)
    want = sc.expected(dsm, t, Z_MAX, aerial, div)
    col = want[1]
    assert np.nanmin(col) == 0.0 and np.nanmax(col) == 1.0 and (aerial_dtype != np.float32 or np.isnan(col).sum() >= 50)
    same(built(L, dsm, t, Z_MAX, aerial, div), want)


# ------------------------------------------------------------------ e. the Python layer at a seam shape
@pytest.fixture(scope="module")
def layer(cu):
    rows, cols = sc.seam_shapes(8, cu, turns=2)[1]
    rng = np.random.default_rng(41)
    dsm16 = rng.integers(1400, 1600, (rows, cols)).astype(np.int16)
    mask = rng.random((rows, cols)) < 0.03
    mask[100:140, 500:700] = True
    dsm16[120, 600] = 3000                                                 # the largest elevation sits under the mask
    aerial4 = sc.aerial_bands(rows, cols, np.uint8, seed=41, bands=4)
    t = sc.transform("half", rows, cols)
    z_max = float(dsm16[~mask].max())
    assert mask[120, 600] and z_max == 1599.0 and 0 < mask.mean() < 0.1
    want = sc.expected(dsm16.astype(np.float64), t, z_max, aerial4[:3], 255.0, mask)
    assert want[0][:, 1].max() == np.float32(z_max - want[3][1])           # the masked peak is clamped like any vertex
    return dict(dsm16=dsm16, dsm64=dsm16.astype(np.float64), mask=mask, aerial4=aerial4, t=t, z_max=z_max, want=want)


@pytest.mark.parametrize("how", ["contiguous", "strided", "four_bands", "int16", "default_height", "default_height_int16"])
def test_python_layer_hands_the_kernels_the_same_rasters(L, layer, how):
    """every way in gives the arrays of contiguous float64 rasters with explicit arguments"""
    from alproj_amd.surface import colored_surface_mesh
    d = layer
    rows, cols = d["mask"].shape
    if how == "contiguous":
        got = built(L, d["dsm64"], d["t"], d["z_max"], np.ascontiguousarray(d["aerial4"][:3]), 255.0, d["mask"])
    elif how == "strided":                   # views with a step in both directions into larger rasters
        big_d = np.full((2 * rows, 2 * cols), -7.0)
        big_a = np.full((3, 2 * rows, 2 * cols), 99, dtype=np.uint8)
        big_m = np.ones((2 * rows, 2 * cols), dtype=bool)
        dv, av, mv = big_d[1::2, ::2], big_a[:, ::2, 1::2], big_m[1::2, 1::2]
        dv[...], av[...], mv[...] = d["dsm64"], d["aerial4"][:3], d["mask"]
        assert not (dv.flags.c_contiguous or av.flags.c_contiguous or mv.flags.c_contiguous)
        got = built(L, dv, d["t"], d["z_max"], av, 255.0, mv)
    elif how == "int16":
        got = built(L, d["dsm16"], d["t"], d["z_max"], np.ascontiguousarray(d["aerial4"][:3]), 255.0, d["mask"])
    else:
        dsm = d["dsm16"] if how == "default_height_int16" else d["dsm64"]
        height = d["z_max"] if how == "four_bands" else None
        with warnings.catch_warnings():
            warnings.simplefilter("error")                                 # no negative elevation, not all nodata: silent
            mesh, off = colored_surface_mesh(d["aerial4"], dsm, d["t"], d["mask"], np.uint8, dsm_max_height=height)
        with mesh:
            got = mesh.fetch_arrays() + (off,)
    same(got, d["want"])


# ------------------------------------------------------------------ f. a rasters-built mesh rendered over several tiles
def test_render_of_a_rasters_built_mesh_over_several_tiles(L):
    """300 x 200 cells = 5 x 13 tiles of 64 x 16, the last of each direction partial, nodata blocks across the tile lines:
    the mesh from_rasters leaves behind and the same arrays uploaded as an implicit grid + set_valid render what the oracle
    renders from the filtered index array -- every visibility word, every image value"""
    from alproj_amd import project as prj
    rows, cols = 201, 301
    yy, xx = np.mgrid[0:rows, 0:cols]
    dsm = (1500.0 + 12.0 * np.sin(xx / 23.0) * np.cos(yy / 31.0) + np.random.default_rng(51).normal(0, 0.3, (rows, cols))).astype(np.float32)
    aerial = sc.aerial_bands(rows, cols, np.uint8, seed=51)
    nodata = sc.tile_straddling_nodata(rows, cols)
    t = sc.transform("north_up", rows, cols)
    want = sc.expected(dsm, t, Z_MAX, aerial, 255.0, nodata)
    mesh, off = L.Mesh.from_rasters(dsm, t, Z_MAX, aerial, 255.0, nodata)
    with mesh:
        vert, col, valid = mesh.fetch_arrays()
        same((vert, col, valid, off), want)
        assert mesh.info() == dict(implicit=True, grid_h=rows, grid_w=cols, n_tri=2 * (rows - 1) * (cols - 1))
        p = dict(syn.BASE_CAMERA)
        ext = vert.max(axis=0)
        p.update(x=off[0] - 20.0, y=off[2] + ext[2] / 2, z=off[1] + ext[1] + 60.0, pan=90.0, tilt=-25.0, fov=70.0,
                 w=320, h=200, cx=160.0, cy=100.0, k1=-0.03, p1=1e-3)
        full = fc.grid_triangles(rows, cols)
        keep = np.flatnonzero(valid[full].all(axis=1))                     # surface.py:203-205
        exp_img = orast.render(vert, col, full[keep], p, off)
        exp_vis = orast.visibility(vert, full[keep], p, off)
        hit = exp_vis != 0
        assert hit.mean() > 0.2 and 0 < len(keep) < len(full)
        tri_ref = keep[0xFFFFFFFF - (exp_vis[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
        # the frame looks at cells of many tiles, some next to the holes
        tiles = np.unique((tri_ref // 2 // (cols - 1)) // sc.TILE_H * 100 + (tri_ref // 2 % (cols - 1)) // sc.TILE_W)
        assert len(tiles) > 30

        def frame_equals_the_oracle(m):
            np.testing.assert_array_equal(prj.persp_proj(m, None, None, p, off), exp_img)
            vis = m.fetch_visibility()
            np.testing.assert_array_equal(vis != 0, hit)
            np.testing.assert_array_equal(vis[hit] >> np.uint64(32), exp_vis[hit] >> np.uint64(32))
            np.testing.assert_array_equal(0xFFFFFFFF - (vis[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64), tri_ref)

        frame_equals_the_oracle(mesh)
        with L.Mesh(vert, col, None, grid=(rows, cols)) as again:
            again.set_valid(valid)
            frame_equals_the_oracle(again)
