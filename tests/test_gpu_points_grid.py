"""GPU tests of the projection's grid form: a point set that is a raster flattened row-major is recognised at creation
(alp_points_layout reports its row length W) and projected from the z plane alone.  Its pixels must be the SAME BITS as the
plane path's (ALP_NO_POINTS_GRID=1), in both precisions, from both creation paths, for every row length around the vector
width and the cap, ragged last rows, row shards and the bench-shaped DSM; sets off the grid must report the plane path."""
import numpy as np
import pytest

from oracle import ref_numpy as orc

pytestmark = pytest.mark.gpu

CAP = 65536                      # alp_points.hip: GRID_MAX_ROW
X0, Y0, Z0 = 732000.0, 4048000.0, 2000.0
NP = {"f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def grid_xyz(w, n, seed=0):
    """n points of a raster with rows of w points, row-major (the last row may be shorter); absolute float64"""
    rows = -(-n // w)
    xs = X0 + np.arange(w, dtype=np.float64) * 1.0
    ys = Y0 + (rows - 1 - np.arange(rows, dtype=np.float64)) * 1.0
    X, Y = np.meshgrid(xs, ys)
    z = Z0 + 50.0 * np.random.default_rng(seed).standard_normal(rows * w)
    return np.ascontiguousarray(np.stack([X.ravel(), Y.ravel(), z], 1)[:n])


def camera(side):
    from alproj_amd import synthetic as syn
    return syn.perturbed(syn.standoff_params(side))


def project(L, xyz, origin, prec, columns, pv):
    """(row length, u, v) of one point set"""
    mk = (lambda: L.Points.from_columns(*[np.ascontiguousarray(xyz[:, k]) for k in range(3)], origin, prec)) if columns \
        else (lambda: L.Points(xyz, origin, prec))
    with mk() as p:
        w = p.row_length()
        p.project(pv)
        u, v = p.fetch(NP[prec])
    return w, u, v


def both_paths(L, monkeypatch, xyz, origin, prec, columns, pv):
    """(row length of the default path, its u, v) after asserting that the plane path gives the same bits"""
    monkeypatch.delenv("ALP_NO_POINTS_GRID", raising=False)
    w, u, v = project(L, xyz, origin, prec, columns, pv)
    monkeypatch.setenv("ALP_NO_POINTS_GRID", "1")
    w0, u0, v0 = project(L, xyz, origin, prec, columns, pv)
    monkeypatch.delenv("ALP_NO_POINTS_GRID")
    assert w0 == 0
    bits = np.uint32 if prec == "f32" else np.uint64
    assert np.array_equal(u.view(bits), u0.view(bits)), "u differs from the plane path"
    assert np.array_equal(v.view(bits), v0.view(bits)), "v differs from the plane path"
    return w, u, v


WIDTHS = (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 10001, CAP - 1, CAP, CAP + 1)


def shapes(w):
    """(label, n): one row; two full rows; three rows with a shorter last one and n not a multiple of 4 where possible"""
    n3 = 2 * w + max(1, w // 2)
    if n3 % 4 == 0 and w > 1:
        n3 -= 1
    return [("1 row", w), ("2 rows", 2 * w), ("3 rows, ragged", n3)]


@pytest.mark.parametrize("columns", [False, True], ids=["rows", "columns"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("w", WIDTHS)
def test_grid_widths_same_bits(L, monkeypatch, w, prec, columns):
    origin = [X0 + 0.5 * w, Y0, Z0]
    for label, n in shapes(w):
        xyz = grid_xyz(w, n, seed=w)
        cam = camera(max(w, 3))
        got, _, _ = both_paths(L, monkeypatch, xyz, origin, prec, columns, L.params_vector(cam))
        expect = w if (n > w and w <= CAP) else 0
        assert got == expect, (label, n, got)


def test_grid_row_shard_and_bench_dsm(L, monkeypatch):
    """a shard of rows from the middle of a DSM, and the 1000 x 1000 DSM as bench.py builds it (local float32 vertices,
    origin at the camera)"""
    from alproj_amd import synthetic as syn
    n_side = 1000
    for rows in ((300, 651), None):
        s = syn.surface(n_side, rows=rows)
        xyz = syn.vert_to_xyz_local(s["vert"])
        base = syn.local_params(syn.standoff_params(n_side), s["offsets"])
        truth = syn.local_params(syn.perturbed(syn.standoff_params(n_side)), s["offsets"])
        for prec in ("f32", "f64"):
            w, _, _ = both_paths(L, monkeypatch, xyz, [base["x"], base["y"], base["z"]], prec, False, L.params_vector(truth))
            assert w == n_side


def test_grid_against_oracle(L, monkeypatch):
    """one grid set in float64 against the float64 oracle, at test_gpu_points' tolerances"""
    from alproj_amd import synthetic as syn
    n = 316
    s = syn.surface(n)
    xyz = syn.vert_to_xyz_abs(s["vert"], s["offsets"])
    cam = syn.perturbed(syn.standoff_params(n))
    w, u, v = both_paths(L, monkeypatch, xyz, [cam["x"], cam["y"], cam["z"]], "f64", False, L.params_vector(cam))
    assert w == n
    np.testing.assert_allclose(np.stack([u, v], 1), orc.project_points(xyz, cam), rtol=1e-9, atol=1e-7)


def off_grid_cases():
    """(label, xyz, origin) of sets that must take the plane path"""
    rng = np.random.default_rng(7)
    w, rows = 1000, 5
    base = grid_xyz(w, w * rows)
    origin = [X0 + 500.0, Y0, Z0]
    out = []
    cloud = np.stack([X0 + rng.uniform(0, 1000, 5000), Y0 + rng.uniform(0, 1000, 5000), Z0 + rng.uniform(0, 50, 5000)], 1)
    out.append(("random cloud", cloud, origin))
    a = base.copy()
    a[(rows - 1) * w + 17, 0] += 0.25                 # one x changed in the last row
    out.append(("x in last row", a, origin))
    a = base.copy()
    a[2 * w + w // 2, 1] += 0.25                      # one y changed mid-row
    out.append(("y mid-row", a, origin))
    a = base.copy()
    a[-1, 1] += 0.25                                  # one y changed in the last element
    out.append(("y last element", a, origin))
    a = base.copy()
    a[:, 1] = np.repeat(np.arange(rows, dtype=np.float64), w)    # row 0 at y = +0.0 ...
    a[5, 1] = -0.0                                               # ... but one -0.0: the same value, other bits
    out.append(("-0.0 against +0.0", a, [X0 + 500.0, 0.0, Z0]))
    out.append(("wider than the cap", grid_xyz(CAP + 1, 3 * (CAP + 1)), origin))
    return out


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_off_grid_plane_path(L, monkeypatch, prec):
    for label, xyz, origin in off_grid_cases():
        w, _, _ = both_paths(L, monkeypatch, xyz, origin, prec, False, L.params_vector(camera(1000)))
        assert w == 0, label
