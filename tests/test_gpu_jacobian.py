"""GPU: the exact Jacobian of the projection (alp_jacobian / jacobian_kernel), LsqOptimizer.optimize(jac="analytic") and
parameter_covariance, against the complex-step oracle of tests/test_jacobian_oracle.py (exact to rounding)."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest

from oracle import ref_numpy as orc
from tests import residual_cases as rc
from tests.test_jacobian_oracle import KEYS, TARGETS, cs_jacobian, cs_project

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
POSE_KEYS = ("x", "y", "z", "fov", "pan", "tilt", "roll")
EINVAL = -1          # ALP_EINVAL


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def g5():
    return np.load(os.path.join(G, "g5_population.npz"))


def lens_params():
    """g5's camera: every lens term non-zero"""
    return orc.vector_to_params(g5()["params_init"])


def synthetic(n, seed=1):
    from alproj_amd import synthetic as syn
    p = lens_params()
    return syn.gcp_points(n, p, seed=seed), p


def idx(targets):
    return [KEYS.index(t) for t in targets]


def device_jacobian(L, xyz, p, targets, precision="f64", of_residuals=True):
    with L.Points(xyz, [p["x"], p["y"], p["z"]], precision) as pts:
        return pts.jacobian(L.params_vector(p), idx(targets), of_residuals)


def assert_columns_close(J, ref, tol):
    assert J.shape == ref.shape
    scale = np.abs(ref).max(axis=0)
    assert (scale > 0).all()
    err = (np.abs(J - ref) / scale).max(axis=0)
    assert (err <= tol).all(), dict(zip(range(J.shape[1]), err))


def g5_candidates():
    """three of g5's D = 21 candidates (every lens term non-zero, r2 up to 7.8).  Not candidates 6, 9, 12, 16 and 23: they put
    a GCP within 1e-3 of a pole of the lens ratio (1 + k4 r2 + k5 r4 + k6 r6 or its y form), where the derivative itself is
    ill-conditioned -- the rounding of the point's own coordinates moves it by ~1e-9 (float64) / 3e-4 (float32) of the
    column's largest entry, which is the pole's"""
    g = g5()
    init = orc.vector_to_params(g["params_init"])
    targets = [str(t) for t in g["d21_targets"]]
    return [orc.candidate_params(init, targets, g["d21_bounds"], g["d21_X"][k]) for k in (0, 7, 20)]


# ---------------------------------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("precision,tol", [("f64", 1e-9), ("f32", 1e-5)])
def test_synthetic_gcps_all_23_targets(L, precision, tol):
    xyz, p = synthetic(900)
    J = device_jacobian(L, xyz, p, TARGETS, precision)
    assert J.dtype == np.float64 and J.shape == (1800, 23)
    assert_columns_close(J, cs_jacobian(xyz, orc.params_to_vector(p), TARGETS), tol)


@pytest.mark.parametrize("precision,tol", [("f64", 1e-9), ("f32", 1e-5)])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_g5_candidates_all_23_targets(L, precision, tol, k):
    p = g5_candidates()[k]
    xyz = g5()["xyz"]
    J = device_jacobian(L, xyz, p, TARGETS, precision)
    assert_columns_close(J, cs_jacobian(xyz, orc.params_to_vector(p), TARGETS), tol)


# ---------------------------------------------------------------------------------------------------- 2. subsets, sign
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_subsets_and_order_are_columns_of_the_full_jacobian(L, precision):
    xyz, p = synthetic(3001, seed=5)
    with L.Points(xyz, [p["x"], p["y"], p["z"]], precision) as pts:
        pv = L.params_vector(p)
        full = pts.jacobian(pv, idx(TARGETS))
        sub = pts.jacobian(pv, idx([TARGETS[5], TARGETS[0], TARGETS[12]]))
        np.testing.assert_array_equal(sub, full[:, [5, 0, 12]])
        for cols in ([22, 1, 9, 17], [8], list(range(22, -1, -1))):
            np.testing.assert_array_equal(pts.jacobian(pv, np.array(idx(TARGETS))[cols]), full[:, cols])
        proj = pts.jacobian(pv, idx(TARGETS), of_residuals=False)
        np.testing.assert_array_equal(full, -proj)


# ---------------------------------------------------------------------------------------------------- 3. batched differences
@pytest.mark.parametrize("frame", ["local", "utm"])
@pytest.mark.parametrize("targets", [TARGETS[:21], ["fov", "pan", "tilt", "roll", "k1", "p2", "cx"]])
def test_agrees_with_the_batched_finite_differences(L, targets, frame):
    """1e-5 per column.  In UTM coordinates scipy's relative step on x / y (1.5e-8 x 7e5 m = 1 cm) has a truncation error
    of ~h / (2 depth) = 1e-4 at the nearest GCPs (80 m): the position columns are held to 5e-4 there, the rest to 1e-5"""
    from alproj_amd import optimize as aopt
    xyz, p = synthetic(900, seed=3)
    if frame == "local":                      # the same scene about a camera near the origin: scipy's steps are small
        shift = np.array([p["x"], p["y"], p["z"]]) - np.array([12.5, -3.0, 250.0])
        xyz = xyz - shift
        p = dict(p, x=12.5, y=-3.0, z=250.0)
    u, v = cs_project(xyz, orc.params_to_vector(p).astype(np.complex128))
    uv = np.column_stack([np.real(u), np.real(v)]) + np.random.default_rng(3).normal(0, 0.5, (900, 2))
    o = aopt.LsqOptimizer(pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"]), dict(p))
    o.set_target(targets)
    pts = o._device_points("f64")
    try:
        fd = o._jacobian_function(pts)(o.target_params_init)
        J = pts.jacobian(L.params_vector(p), idx(targets))
    finally:
        pts.close()
    pos = [j for j, t in enumerate(targets) if t in ("x", "y", "z")]
    rest = [j for j in range(len(targets)) if j not in pos]
    assert_columns_close(J[:, rest], fd[:, rest], 1e-5)
    assert_columns_close(J[:, pos], fd[:, pos], 1e-5 if frame == "local" else 5e-4)


# ---------------------------------------------------------------------------------------------------- 4. shapes
D_TARGETS = {1: ["pan"], 7: ["k1", "x", "fov", "s4", "cy", "a2", "roll"], 23: TARGETS}


@pytest.mark.parametrize("n", [1, 255, 256, 257, 10_007, 1_000_003])
def test_shapes(L, n):
    xyz, p = synthetic(n, seed=n)
    pv = orc.params_to_vector(p)
    rows = np.arange(n) if n <= 10_007 else np.unique(np.r_[np.arange(0, n, 997), n - 1])
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f64") as pts:
        for D, targets in D_TARGETS.items():
            J = pts.jacobian(L.params_vector(p), idx(targets))
            assert J.shape == (2 * n, D)
            ref = cs_jacobian(xyz[rows], pv, targets)
            got = J.reshape(n, 2, D)[rows].reshape(-1, D)
            assert_columns_close(got, ref, 1e-9)


def test_ten_million_points_take_several_staging_chunks(L):
    """10 M points at D = 21: 3.4 GB of output, 13 launches of at most 256 MB (chunk = max(1024, (256 MiB // (16 D)) // 1024
    * 1024) points, tests/residual_cases.py); compared on a strided sample of rows, the last 300 and every row within 3 of a
    chunk boundary"""
    n = 10_000_000
    g = g5()
    targets = [str(t) for t in g["d21_targets"]]
    xyz, p = synthetic(n, seed=11)
    p = dict(p, pan=p["pan"] + 0.3, k1=p["k1"] * 1.1)
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f64") as pts:
        L.kernel_timing(True)
        try:
            L.kernel_time_ms()
            J = pts.jacobian(L.params_vector(p), idx(targets))
            _, sections = L.kernel_time_ms()
        finally:
            L.kernel_timing(False)
    assert J.shape == (2 * n, 21)
    assert sections == rc.launches(n, 21) == 13
    rows = np.unique(np.r_[np.arange(0, n, 4099), np.arange(n - 300, n), rc.boundary_points(n, rc.chunk_points(n, 21))])
    got = J.reshape(n, 2, 21)[rows].reshape(-1, 21)
    del J
    assert_columns_close(got, cs_jacobian(xyz[rows], orc.params_to_vector(p), targets), 1e-9)


# ---------------------------------------------------------------------------------------------------- 5. LsqOptimizer
LSQ_KW = {"trf_linear_d7": dict(method="trf"),
          "trf_huber_d7": dict(method="trf", loss="huber", f_scale=5.0),
          "dogbox_softl1_d4": dict(method="dogbox", loss="soft_l1", f_scale=3.0,
                                   bound_widths={"fov": 10, "pan": 10, "tilt": 10, "roll": 10}),
          "trf_cauchy_d4": dict(method="trf", loss="cauchy", f_scale=2.0),
          "lm_d4": dict(method="lm"),
          "trf_linear_dist_d6": dict(method="trf")}


@pytest.mark.parametrize("case", list(LSQ_KW))
def test_g14_with_the_exact_jacobian(L, case):
    """the reference's least-squares runs of g14 (scipy with 2-point differences) reached with jac="analytic", to the
    tolerances of test_gpu_golden_render.py::test_g14_*"""
    from alproj_amd import optimize as aopt
    g = np.load(os.path.join(G, "g14_lsq.npz"))
    keys = [str(k) for k in g["param_keys"]]
    init = dict(zip(keys, g[f"{case}_init"]))
    dfx = pd.DataFrame(g["xyz"], columns=["x", "y", "z"])
    dfu = pd.DataFrame(g["uv_" + str(g[f"{case}_uv"])], columns=["u", "v"])
    targets = [str(t) for t in g[f"{case}_targets"]]
    want = dict(zip(keys, g[f"{case}_params"]))
    o = aopt.LsqOptimizer(dfx, dfu, dict(init))
    o.set_target(targets)
    params, err = o.optimize(jac="analytic", **LSQ_KW[case])
    assert set(params) == set(want)
    for k in targets:
        tol = 2e-4 if k in POSE_KEYS else 2e-6
        assert abs(params[k] - want[k]) <= tol, (k, params[k], want[k])
    assert err == pytest.approx(float(g[f"{case}_error"]), rel=5e-5)


# ---------------------------------------------------------------------------------------------------- 6. covariance
def noisy_gcps(n, p, sigma, seed):
    from alproj_amd import synthetic as syn
    xyz = syn.gcp_points(n, p, seed=1)
    u, v = cs_project(xyz, orc.params_to_vector(p).astype(np.complex128))
    uv = np.column_stack([np.real(u), np.real(v)]) + np.random.default_rng(seed).normal(0, sigma, (n, 2))
    return pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"])


def test_parameter_covariance_against_numpy(L):
    from alproj_amd import optimize as aopt
    p = lens_params()
    targets = ["x", "fov", "pan", "tilt", "roll", "k1", "p1", "cy"]
    dfx, dfu = noisy_gcps(900, p, 0.5, seed=2)
    cov, std = aopt.parameter_covariance(dfx, dfu, p, targets)
    J = cs_jacobian(dfx.to_numpy(), orc.params_to_vector(p), targets)
    r = orc.residual_vector(dfx.to_numpy(), dfu.to_numpy(), p)
    want = np.linalg.inv(J.T @ J) * (r @ r) / (len(r) - len(targets))
    np.testing.assert_allclose(cov, want, rtol=1e-8, atol=1e-8 * np.abs(np.diag(want)).max())
    assert list(std) == targets
    np.testing.assert_allclose([std[t] for t in targets], np.sqrt(np.diag(want)), rtol=1e-8)


def test_parameter_covariance_rank_deficient_is_inf(L):
    """with every lens term zero (a1 = a2 = 0 included) the ratio (1 + k1 r2 + ...) / (1 + k4 r2 + ...) moves with k1 exactly
    as it moves against k4: their columns are exact negatives, and the GCPs cannot determine both"""
    from alproj_amd import optimize as aopt
    p = dict(lens_params(), **{k: 0.0 for k in orc.DIST_KEYS})
    dfx, dfu = noisy_gcps(300, p, 0.5, seed=4)
    cov, std = aopt.parameter_covariance(dfx, dfu, p, ["fov", "k1", "k4"])
    assert np.isinf(cov).all() and all(np.isinf(v) for v in std.values())
    with pytest.raises(ValueError):
        aopt.parameter_covariance(dfx.iloc[:2], dfu.iloc[:2], p, ["fov", "pan", "tilt", "roll", "k1"])


def test_parameter_covariance_predicts_the_scatter_of_the_optimum(L):
    """20 noise seeds (0.5 px, 900 GCPs, targets fov / pan / tilt / roll): the standard deviation of the least-squares pan
    lies within a factor of 1.5 of the predicted std["pan"]"""
    from alproj_amd import optimize as aopt
    p = lens_params()
    targets = ["fov", "pan", "tilt", "roll"]
    pans, predicted = [], None
    for seed in range(20):
        dfx, dfu = noisy_gcps(900, p, 0.5, seed=100 + seed)
        init = dict(p, fov=p["fov"] + 0.5, pan=p["pan"] - 0.4, tilt=p["tilt"] + 0.3, roll=p["roll"] - 0.2)
        o = aopt.LsqOptimizer(dfx, dfu, init)
        o.set_target(targets)
        params, _ = o.optimize(method="trf", jac="analytic", x_scale="jac")
        pans.append(params["pan"])
        if seed == 0:
            predicted = aopt.parameter_covariance(dfx, dfu, params, targets)[1]["pan"]
    spread = float(np.std(pans, ddof=1))
    assert predicted / 1.5 <= spread <= predicted * 1.5, (spread, predicted)


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_error_paths(L):
    xyz, p = synthetic(64)
    lib = L.lib()
    I32 = ctypes.POINTER(ctypes.c_int32)
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f64") as pts:
        pv = L.params_vector(p)
        out = np.empty((128, 24))
        good = np.array(idx(["pan", "tilt"]), dtype=np.int32)

        def call(h, params, targets, D, outp):
            return lib.alp_jacobian(h, params, targets, D, 1, outp)

        tp = good.ctypes.data_as(I32)
        assert call(pts._h, L.as_dp(pv), tp, 2, L.as_dp(out)) == 0
        assert call(None, L.as_dp(pv), tp, 2, L.as_dp(out)) == EINVAL
        assert call(pts._h, None, tp, 2, L.as_dp(out)) == EINVAL
        assert call(pts._h, L.as_dp(pv), None, 2, L.as_dp(out)) == EINVAL
        assert call(pts._h, L.as_dp(pv), tp, 2, None) == EINVAL
        many = np.arange(25, dtype=np.int32)
        for D in (0, 24, -1):
            assert call(pts._h, L.as_dp(pv), many.ctypes.data_as(I32), D, L.as_dp(out)) == EINVAL
        for bad in ([KEYS.index("w")], [KEYS.index("pan"), KEYS.index("h")], [4, 4], [25], [-1]):
            b = np.array(bad, dtype=np.int32)
            assert call(pts._h, L.as_dp(pv), b.ctypes.data_as(I32), len(bad), L.as_dp(out)) == EINVAL, bad
        for bad in (["w"], ["pan", "pan"], []):
            with pytest.raises(L.AlprojHipError) as e:
                pts.jacobian(pv, idx(bad))
            assert e.value.code == EINVAL
    with L.Points(np.zeros((0, 3)), [0, 0, 0], "f64") as empty:
        assert empty.jacobian(pv, idx(["pan"])).shape == (0, 1)
