"""GPU tests of the grid projection where a lane's vector meets a row end.  K1's grid form (alp_point_kernels.h) divides once per
lane; a vector that lies in one row reads its x values as one vector of the column table, a vector that crosses a row end walks
its points with an add and a compare (host/alp_plan.h: RowWalk), and rows shorter than a vector keep a division per point.  As in
test_gpu_points_grid.py the same set is created by default and under ALP_NO_POINTS_GRID=1, and u and v must be the SAME BITS,
in both precisions and from both creation paths.  Every output must be finite (a wrong row or column would still be some point
of the set, so a strided sample is also held to the float64 oracle at test_grid_against_oracle's tolerances)."""
import numpy as np
import pytest

from oracle import ref_numpy as orc

pytestmark = pytest.mark.gpu

NP = {"f32": np.float32, "f64": np.float64}
VEC = {"f32": 4, "f64": 2}          # points per 16-byte vector = per lane
WAVE, WG = 64, 256


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def raster(w, n):
    """(xyz absolute float64, camera): n points of a raster with rows of w points, row-major, 1 m apart, seen from the stand-off
    camera of the point-set workloads (the whole raster in front of it), so that every pixel is finite"""
    from alproj_amd import synthetic as syn
    rows = -(-n // w)
    side = max(w, rows, 3)
    ox, oz, oy = syn.ABS_ORIGIN_XZY
    X, Y = np.meshgrid(ox + np.arange(w, dtype=np.float64), oy + (rows - 1 - np.arange(rows, dtype=np.float64)))
    z = oz + 20.0 * np.random.default_rng(w * 7919 + n).standard_normal(rows * w)
    xyz = np.ascontiguousarray(np.stack([X.ravel(), Y.ravel(), z], 1)[:n])
    cam = syn.perturbed(syn.standoff_params(side))
    # the stand-off is 0.65 sides west of the raster and 600 m above it: keep a tiny raster well in front of the camera too
    cam["x"] -= 1500.0
    return xyz, cam


def project(L, xyz, origin, prec, columns, pv):
    mk = (lambda: L.Points.from_columns(*[np.ascontiguousarray(xyz[:, k]) for k in range(3)], origin, prec)) if columns \
        else (lambda: L.Points(xyz, origin, prec))
    with mk() as p:
        w = p.row_length()
        p.project(pv)
        u, v = p.fetch(NP[prec])
    return w, u, v


_ORACLE = {}


def oracle_sample(w, n, xyz, cam, stride):
    """the float64 oracle's pixels of every stride-th point: computed once per shape, shared, never modified"""
    key = (w, n, stride)
    if key not in _ORACLE:
        ref = orc.project_points(xyz[::stride], cam)
        ref.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


def check(L, monkeypatch, w, n, prec):
    """the set of n points in rows of w: grid form against plane form bit for bit from both creation paths, finite everywhere,
    and (float64) a strided sample against the oracle"""
    assert n > w, "a single row is not a grid set"
    xyz, cam = raster(w, n)
    origin = [cam["x"], cam["y"], cam["z"]]
    pv = L.params_vector(cam)
    bits = np.uint32 if prec == "f32" else np.uint64
    for columns in (False, True):
        monkeypatch.delenv("ALP_NO_POINTS_GRID", raising=False)
        got, u, v = project(L, xyz, origin, prec, columns, pv)
        monkeypatch.setenv("ALP_NO_POINTS_GRID", "1")
        got0, u0, v0 = project(L, xyz, origin, prec, columns, pv)
        monkeypatch.delenv("ALP_NO_POINTS_GRID")
        assert (got, got0) == (w, 0), (w, n, prec, columns, got, got0)
        assert u.shape == v.shape == (n,)
        assert np.isfinite(u).all() and np.isfinite(v).all(), (w, n, prec, columns)
        bad = np.flatnonzero((u.view(bits) != u0.view(bits)) | (v.view(bits) != v0.view(bits)))
        assert bad.size == 0, f"w={w} n={n} {prec} columns={columns}: {bad.size} points differ from the plane path, first {bad[:8]}"
        if prec == "f64":
            stride = max(1, n // 997)
            ref = oracle_sample(w, n, xyz, cam, stride)
            np.testing.assert_allclose(np.stack([u[::stride], v[::stride]], 1), ref, rtol=1e-9, atol=1e-7)


def crossing_vectors(w, n, vec):
    """indices of the vectors (= lanes over the flat launch) that hold points of two rows or more"""
    first = np.arange(0, n, vec)
    last = np.minimum(first + vec - 1, n - 1)
    return np.flatnonzero(first // w != last // w)


# ---------------------------------------------------------------- row lengths around the vector width
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_row_lengths_around_the_vector_width(L, monkeypatch, prec):
    """VEC - 1: several row ends per vector (the per-point fallback); VEC: none; VEC + 1, 2 VEC - 1, 2 VEC + 1: the smallest
    rows with exactly one row end in some vectors"""
    vec = VEC[prec]
    for w in (vec - 1, vec, vec + 1, 2 * vec - 1, 2 * vec + 1):
        for n in (w + 1, 2 * w, 2000 * w + w // 2 + 1):
            cross = crossing_vectors(w, n, vec)
            if w % vec == 0:
                assert cross.size == 0
            elif n > 2 * vec:
                assert cross.size > 0
            check(L, monkeypatch, w, n, prec)


# ---------------------------------------------------------------- the crossing lane at the seams of the launch
# where the first crossing vector of the set lies: the last lane of a wave, the first lane of the next wave, the last lane of
# a workgroup, the first lane of the next workgroup
SEAMS = {255: lambda i: i % WAVE == WAVE - 1, 257: lambda i: i % WAVE == 0 and i > 0,
         1023: lambda i: i % WG == WG - 1, 1025: lambda i: i % WG == 0 and i > 0}


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("w", sorted(SEAMS))
def test_crossing_lane_at_wave_and_workgroup_seams(L, monkeypatch, w, prec):
    n = 3 * 1024 + 5
    vec = VEC[prec]
    cross = crossing_vectors(w, n, vec)
    # W = 2^k -+ 1: the first row end lies in vector (2^k / VEC) - 1 resp. 2^k / VEC, a lane on either side of the seam
    assert cross.size > 0 and SEAMS[w](int(cross[0])), (w, prec, cross[:4])
    assert cross.size < len(range(0, n, vec)) // 8        # ... and nearly every other lane takes the one-row form
    check(L, monkeypatch, w, n, prec)


# ---------------------------------------------------------------- the clamp to the last point in the crossing form
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_short_last_rows_and_every_tail(L, monkeypatch, prec):
    """a last row shorter than a vector, down to one point, with every n % VEC: the final vector then crosses a row end AND has
    padding, which must not address the row after the last one"""
    vec = VEC[prec]
    seen_short, seen_one, clamped = set(), set(), set()
    for w in (vec + 1, 2 * vec + 1, 1025):
        for rows in range(2, 2 + vec):
            for tail in sorted({1, vec - 1, max(1, vec - 2)}):             # points in the last row: 1 .. VEC - 1
                n = rows * w + tail
                seen_short.add(n % vec)
                if tail == 1:
                    seen_one.add(n % vec)
                e0 = (n - 1) // vec * vec                                   # the final vector
                if e0 < rows * w and e0 + vec > n:                          # crosses into the last row and runs past it
                    clamped.add(w)
                check(L, monkeypatch, w, n, prec)
    assert seen_short == seen_one == set(range(vec)), (seen_short, seen_one)
    # two points per vector: the second one is the last row's only point, so there is no padding to clamp
    assert clamped == ({vec + 1, 2 * vec + 1, 1025} if vec > 2 else set()), clamped


# ---------------------------------------------------------------- a set that is one vector
def test_one_vector_sets(L, monkeypatch):
    """exactly one lane, whose vector crosses a row end (rows of VEC - 1 points: the crossing walk; shorter rows: the per-point
    fallback), full and with padding"""
    for prec, w, n in (("f32", 3, 4), ("f32", 2, 4), ("f32", 2, 3), ("f32", 1, 4), ("f32", 1, 2), ("f64", 1, 2)):
        assert n <= VEC[prec] and crossing_vectors(w, n, VEC[prec]).tolist() == [0]
        check(L, monkeypatch, w, n, prec)
