"""CPU: frequency weights in the oracle's terms.  "Weight w_i" means "row i appears w_i times" for integer weights, so the
oracle of every weighted test is the existing one on row-duplicated tables; g20_weighted.npz holds what the reference returned
on such tables (tests/golden/gen_golden_weighted.py)."""
import os

import numpy as np

from oracle import ref_numpy as orc

G = os.path.join(os.path.dirname(__file__), "golden")
POPULATIONS = {"lf": 9, "gen": 21, "sp": 12}


def g20():
    return np.load(os.path.join(G, "g20_weighted.npz"), allow_pickle=False)


def dup(a, w):
    return np.repeat(np.asarray(a), np.asarray(w).astype(np.int64), axis=0)


def distances(xyz, uv, p):
    prj = orc.project_points(xyz, p)
    return ((uv[:, 0] - prj[:, 0]) ** 2 + (uv[:, 1] - prj[:, 1]) ** 2) ** 0.5


def test_g20_is_data_of_the_stated_shape():
    g = g20()
    w = g["weights"]
    assert g["xyz"].shape == (len(w), 3) and g["uv_obs"].shape == (len(w), 2) and 1000 <= len(w) <= 1200
    assert np.array_equal(w, np.round(w)) and w.min() == 0 and w.max() == 3 and (w == 0).sum() > len(w) // 8
    for name, d in POPULATIONS.items():
        assert g[f"{name}_X"].shape == (140, d) and g[f"{name}_md"].shape == g[f"{name}_hub"].shape == (140,)
        assert np.isfinite(g[f"{name}_md"]).all() and np.isfinite(g[f"{name}_hub"]).all()
    lf = orc.vector_to_params(g["lf_params_init"])
    assert all(lf[k] == 0.0 for k in ("k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2", "s1", "s2", "s3", "s4"))


def test_oracle_on_duplicated_rows_reproduces_g20():
    """at the tolerance tests/test_oracle_golden.py holds g19 to"""
    g = g20()
    xyz, uv = dup(g["xyz"], g["weights"]), dup(g["uv_obs"], g["weights"])
    assert len(xyz) == int(g["weights"].sum())
    for name in POPULATIONS:
        init = orc.vector_to_params(g[f"{name}_params_init"])
        tgt = [str(t) for t in g[f"{name}_targets"]]
        bounds = orc.bounds_to_array(init, tgt)
        np.testing.assert_array_equal(bounds, g[f"{name}_bounds"])
        for tag, fs in (("md", None), ("hub", 10.0)):
            losses, amin = orc.population_losses(xyz, uv, init, tgt, bounds, g[f"{name}_X"], fs)
            np.testing.assert_allclose(losses, g[f"{name}_{tag}"], rtol=1e-12)
            assert amin == int(np.argmin(g[f"{name}_{tag}"])) and losses[3] == losses[7]


def test_the_weighted_sum_formula_is_the_duplicated_rows():
    """sum w_i d_i / W and sum w_i huber(d_i) / W against the oracle on the duplicated tables"""
    g = g20()
    w = g["weights"]
    xyz2, uv2 = dup(g["xyz"], w), dup(g["uv_obs"], w)
    for name in POPULATIONS:
        init = orc.vector_to_params(g[f"{name}_params_init"])
        tgt = [str(t) for t in g[f"{name}_targets"]]
        for x in g[f"{name}_X"][:6]:
            p = orc.candidate_params(init, tgt, g[f"{name}_bounds"], x)
            d = distances(g["xyz"], g["uv_obs"], p)
            hub = np.where(d <= 10.0, 0.5 * d ** 2, 10.0 * (d - 0.5 * 10.0))
            prj = orc.project_points(xyz2, p)
            assert abs(np.sum(w * d) / w.sum() / orc.mean_distance(uv2, prj) - 1) <= 1e-13
            assert abs(np.sum(w * hub) / w.sum() / orc.huber(uv2, prj, 10.0) - 1) <= 1e-13


def test_a_zero_weight_row_at_the_camera_leaves_the_result_finite():
    """the term of a row of weight 0 is SELECTED away, not multiplied by 0 (0 * NaN is NaN): absent, as in the duplicated table"""
    g = g20()
    init = orc.vector_to_params(g["gen_params_init"])
    cam = np.array([[init["x"], init["y"], init["z"]]])
    xyz, uv = np.vstack([g["xyz"], cam]), np.vstack([g["uv_obs"], [[10.0, 10.0]]])
    w = np.append(g["weights"], 0.0)
    with np.errstate(all="ignore"):
        d = distances(xyz, uv, init)
    assert np.isnan(d[-1]) and np.isfinite(d[:-1]).all()
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.sum(w * d))                                   # what a multiplication would give
    selected = np.sum(np.where(w > 0, w * np.where(w > 0, d, 0.0), 0.0)) / w.sum()
    ref = orc.mean_distance(dup(uv, w), orc.project_points(dup(xyz, w), init))
    assert np.isfinite(selected) and abs(selected / ref - 1) <= 1e-13


def test_weights_check_refuses_on_the_host():
    import pytest

    from alproj_amd import _lib
    from alproj_amd.optimize import CMAOptimizer, LsqOptimizer
    for bad in ([1.0, 2.0], [1.0, -1.0, 1.0], [1.0, np.nan, 1.0], [np.inf, 1.0, 1.0], [0.0, 0.0, 0.0], [[1.0, 1.0, 1.0]]):
        with pytest.raises(ValueError):
            _lib.weights_check(bad, 3)
    with pytest.raises(ValueError):
        _lib.weights_check([1e39, 1.0, 1.0], 3, _lib.ALP_F32)           # finite, but not in the float32 the set would store
    with pytest.raises(ValueError):
        _lib.weights_check([1e-60, 0.0, 0.0], 3, _lib.ALP_F32)          # rounds to 0 in float32: no point is left
    assert _lib.weights_check([1, 0, 2], 3).dtype == np.float64
    assert _lib.weights_check(np.array([1, 0, 2], dtype=np.float32), 3).dtype == np.float32
    xyz, uv = np.zeros((3, 3)), np.zeros((3, 2))
    for cls in (CMAOptimizer, LsqOptimizer):
        with pytest.raises(ValueError):
            cls(xyz, uv, {}, weights=[1.0, 1.0])
        assert cls(xyz, uv, {}).weights is None
    o = LsqOptimizer(xyz, uv, {}, weights=[4.0, 0.0, 1.0])
    np.testing.assert_array_equal(o._row_scale(), [2.0, 2.0, 0.0, 0.0, 1.0, 1.0])
    o.target_params = ["pan"]
    with pytest.raises(ValueError, match="method='normal'"):
        o.optimize(method="trf", loss="huber")
