"""CPU: pin tests/surface_cases.py -- its numpy statement of the mesh construction to the arrays the REFERENCE's own
get_colored_surface returned (g11, tests/golden/gen_golden_surface.py), its map of surface_zmin_kernel's launch to an
enumeration of the kernel's loops and to the constants read from alp_mesh.hip, and its shapes and positions to the
conditions the GPU seam tests (test_gpu_surface_seams.py) rely on."""
import os
import re

import numpy as np
import pytest

from tests import surface_cases as sc

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "g11_surface.npz"))
NAMES = [str(n) for n in G["names"]]
CSRC = os.path.join(os.path.dirname(os.path.dirname(__file__)), "alproj_amd", "csrc")
CU_COUNTS = [256, 64, 304]


def _divisor(name):
    """what _normalize_aerial divides by for the fixture's aerial type (surface.py:45-56); 0 = nothing"""
    cm = float(G[f"{name}_color_max"])
    aerial = G[f"{name}_aerial"]
    if not np.isnan(cm):
        return cm
    if np.issubdtype(aerial.dtype, np.integer):
        return float(np.iinfo(aerial.dtype).max)
    return 0.0 if aerial.astype(np.float64).max() <= 1.0 else 255.0


@pytest.mark.parametrize("name", NAMES)
def test_expected_reproduces_the_references_arrays(name):
    nodata = G[f"{name}_nodata"]
    vert, col, valid, off = sc.expected(G[f"{name}_filled"], G[f"{name}_transform"], np.float32(G[f"{name}_zmax"]),
                                        G[f"{name}_aerial"], _divisor(name), nodata)
    assert vert.dtype == np.float32 and col.dtype == np.float32 and valid.dtype == bool and off.dtype == np.float64
    np.testing.assert_array_equal(off, G[f"{name}_offsets"])
    # bit for bit: the views also tell -0.0 from 0.0
    np.testing.assert_array_equal(vert.view(np.uint32), G[f"{name}_vert"].astype(np.float32).view(np.uint32))
    np.testing.assert_array_equal(col.view(np.uint32), G[f"{name}_col"].astype(np.float32).view(np.uint32))
    np.testing.assert_array_equal(valid, ~nodata.ravel())


def test_expected_on_the_values_the_fixtures_do_not_hold():
    """a non-square raster, both clamps, -0.0, NaN and +inf elevations, colours outside [0, 1]: by hand"""
    dsm = np.array([[-3.0, -0.0, 7.0], [np.inf, 2.0, np.nan]], dtype=np.float32)
    aerial = np.array([[[-1.0, 0.25, 2.0], [np.nan, np.inf, -np.inf]]] * 3, dtype=np.float32)
    t = (-2.0, 0.0, 10.0, 0.0, 0.5, 100.0)
    with np.errstate(invalid="ignore"):
        vert, col, valid, off = sc.expected(dsm, t, 5.0, aerial, 0.0, np.array([[0, 1, 0], [0, 0, 1]]))
    np.testing.assert_array_equal(sc.clamped_z(dsm, 5.0), [[0.0, 0.0, 5.0], [5.0, 2.0, np.nan]])
    assert np.signbit(sc.clamped_z(dsm, 5.0)[0, 1])                        # the reference leaves -0.0 as it is
    assert off[0] == 6.0 and np.isnan(off[1]) and off[2] == 100.0          # numpy's min returns the NaN
    np.testing.assert_array_equal(vert[:, 0], [4.0, 2.0, 0.0, 4.0, 2.0, 0.0])
    np.testing.assert_array_equal(vert[:, 2], [0.0, 0.0, 0.0, 0.5, 0.5, 0.5])
    assert np.isnan(vert[:, 1]).all()
    np.testing.assert_array_equal(col[:, 0], [0.0, 0.25, 1.0, np.nan, 1.0, 0.0])
    np.testing.assert_array_equal(col[:, 0], col[:, 2])
    np.testing.assert_array_equal(valid, [True, False, True, True, True, False])
    _, col255, _, off0 = sc.expected(np.where(np.isnan(dsm), 1.0, dsm), t, 5.0, np.full((3, 2, 3), 51, np.uint8), 255.0)
    np.testing.assert_array_equal(col255, np.float32(51 / 255))
    assert off0[1] == 0.0


def test_launch_constants_are_the_kernels():
    src = open(os.path.join(CSRC, "alp_mesh.hip")).read()
    assert re.search(r"__launch_bounds__\((\d+)\) void surface_zmin_kernel", src).group(1) == str(sc.WG_LANES)
    assert f"constexpr int V = {sc.PACK_BYTES} / (int)sizeof(Z);" in src
    assert f"const dim3 grid((unsigned)(ctx().cu_count * {sc.WG_PER_CU}));" in src
    assert "surface_zmin_kernel<float>, grid, dim3(256)" in src and "surface_zmin_kernel<double>, grid, dim3(256)" in src
    plan = open(os.path.join(CSRC, "raster_plan.h")).read()
    assert 1 << int(re.search(r"#define GT_W_LOG2 (\d+)", plan).group(1)) == sc.TILE_W
    assert 1 << int(re.search(r"#define GT_H_LOG2 (\d+)", plan).group(1)) == sc.TILE_H


@pytest.mark.parametrize("itemsize", [4, 8])
@pytest.mark.parametrize("cu_count", CU_COUNTS + [1, 3])
def test_zmin_slot_is_the_enumerated_launch(cu_count, itemsize):
    """every element of rasters of one, two and three turns (the real CU counts: two turns and a tail, to stay quick)"""
    V, T = sc.pack_len(itemsize), sc.turn_packs(cu_count)
    sizes = [1, V - 1, V, V + 1, 9, T * V, T * V + 1, T * V + 300 * V + V - 1]
    if cu_count <= 3:
        sizes += [2 * T * V + V - 1, 2 * T * V + V, 3 * T * V, 3 * T * V + 1]
    for n in sizes:
        slots = sc.launch_enumeration(n, itemsize, cu_count)
        assert (slots >= 0).all(), n                                       # every element is read by some lane
        idx = np.arange(n)
        if n >= 5000:            # both ends, a stride coprime to every size of the launch, the last lane of workgroups
            idx = np.unique(np.concatenate([idx[:600], idx[-600:], idx[::997], idx[(idx // V) % 256 == 255][::53]]))
        want = np.array([sc.zmin_slot(int(i), n, itemsize, cu_count) for i in idx])
        np.testing.assert_array_equal(slots[idx], want.astype(np.int64), err_msg=str(n))
        assert slots[:, 3].sum() == n % V and slots[:, 0].max() == max(0, (n // V - 1) // T)
    with pytest.raises(IndexError):
        sc.zmin_slot(9, 9, itemsize, cu_count)


@pytest.mark.parametrize("itemsize", [4, 8])
@pytest.mark.parametrize("cu_count", CU_COUNTS)
def test_seam_shapes_and_min_positions_cover_every_slot(cu_count, itemsize):
    V, T = sc.pack_len(itemsize), sc.turn_packs(cu_count)
    shapes = sc.seam_shapes(itemsize, cu_count)
    assert sorted(shapes) == ([1, 2, 3] if itemsize == 4 else [1])         # every nonzero remainder of the type
    for rem, (rows, cols) in shapes.items():
        n = rows * cols
        assert cols % 2 == 1 and cols > 1000 and n % V == rem != 0
        assert 2 * T * V < n < 2 * T * V + 8 * sc.WG_LANES * V + 4 * cols < 3 * T * V    # three turns, the third partial
        if cu_count == 256:                                                # 2.1 M float32 / 1.05 M float64 vertices
            assert 1 < n / (2097152 if itemsize == 4 else 1048576) < 1.01
        pos = sc.min_positions(n, itemsize, cu_count)
        assert list(pos) == sc.POSITIONS and len(set(pos.values())) == len(pos)
        slot = {name: sc.zmin_slot(i, n, itemsize, cu_count) for name, i in pos.items()}
        assert pos["first"] == 0 and slot["first"] == (0, 0, 0, False)
        assert pos["body_last"] == n - rem - 1 and slot["body_last"][0] == 2 and not slot["body_last"][3]
        assert pos["tail_last"] == n - 1 and slot["tail_last"] == (0, 0, 0, True)
        for w in (1, 2, 3):
            assert slot[f"wave{w}"] == (0, 4 + w, w, False)                # past the workgroups a tiny raster fills
        assert slot["last_workgroup"] == (0, 4 * cu_count - 1, 0, False)
        assert slot["turn1"] == (1, 7, 1, False) and slot["turn2"] == (2, 0, 1, False)
        # the enumeration agrees at the full size too
        slots = sc.launch_enumeration(n, itemsize, cu_count)
        for name, i in pos.items():
            assert tuple(slots[i]) == tuple(int(v) for v in slot[name]), name
    two = sc.seam_shapes(itemsize, cu_count, turns=2)[1]
    assert T * V < two[0] * two[1] < 2 * T * V and two[1] % 2 == 1 and (two[0] * two[1]) % V == 1
    assert "turn1" in sc.min_positions(two[0] * two[1], itemsize, cu_count)
    assert "turn2" not in sc.min_positions(two[0] * two[1], itemsize, cu_count)


def test_small_shapes_and_a_raster_without_the_slots():
    assert [r * c for r, c in sc.SMALL_SHAPES] == [4, 6, 9]                # float32: n = V, a tail of 2, two packs + 1
    assert sc.min_positions(4, 4, 256) == {"first": 0, "body_last": 3}
    assert sc.min_positions(6, 4, 256) == {"first": 0, "body_last": 3, "tail_last": 5}
    assert sc.min_positions(9, 8, 256) == {"first": 0, "body_last": 7, "tail_last": 8}
    assert sc.min_positions(3, 4, 256) == {"first": 0, "tail_last": 2}     # n < V: the tail alone


@pytest.mark.parametrize("name", sc.TRANSFORMS)
def test_transforms_do_what_their_names_say(name):
    rows, cols = 1029, 2049
    t = sc.transform(name, rows, cols)
    x = np.arange(cols) * t[0] + t[2]
    y = np.arange(rows) * t[4] + t[5]
    assert t[1] == 0 and t[3] == 0 and x.min() > 7e5 and y.min() > 4e6                 # UTM magnitude
    assert (np.argmin(x) == cols - 1) == (name == "west_up") and (np.argmin(y) == 0) == (name == "south_up")
    # exact products and sums for whole-metre and 2.5 m cells; 0.3 m cells round in most columns
    from fractions import Fraction
    inexact = sum(Fraction(c) * Fraction(t[0]) + Fraction(t[2]) != Fraction(float(x[c])) for c in range(0, cols, 16))
    assert (inexact > cols // 32) == (name == "fine"), inexact


def test_tile_straddling_nodata_crosses_tile_lines():
    rows, cols = 201, 301
    m = sc.tile_straddling_nodata(rows, cols)
    assert m.shape == (rows, cols) and 0.02 < m.mean() < 0.15
    assert m[8, sc.TILE_W - 1] and m[8, sc.TILE_W] and m[8, sc.TILE_W + 1]            # both sides of a column line
    assert m[sc.TILE_H - 1, 30] and m[sc.TILE_H, 30] and m[sc.TILE_H + 1, 30]         # both sides of a row line
    r, c = 3 * sc.TILE_H, 2 * sc.TILE_W
    assert m[r - 1, c - 1] and m[r - 1, c + 1] and m[r + 1, c - 1] and m[r + 1, c + 1]   # four tiles at a corner
    assert m[rows - 1, cols - 1] and not m[0, 0]
