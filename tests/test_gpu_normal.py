"""GPU: the normal equations formed on the device (alp_normal_equations / normal_kernel), LsqOptimizer.optimize(method="normal")
and parameter_covariance(method="normal").

Against the complex-step oracle of tests/normal_cases.py, each entry normalised by m max|J_i| max|J_j| (G) or m max|J_i| max|r|
(g), m = 2N: twice the per-column tolerance tests/test_gpu_jacobian.py holds the Jacobian kernel to (a product of two factors,
each within that tolerance) -- 2e-9 on a float64 set, 2e-5 on a float32 one; the cost to 1e-9 / 1e-5 relative; the count exactly.
Against the library's own pieces (J and r fetched and contracted on the host) the difference is the order of the additions
alone: two sums of m terms, each within m eps sum|terms| <= m eps (m max max) of the exact value, differ by at most 2 m eps of
the normaliser; the bound is 4 m eps."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest

from oracle import ref_numpy as orc
from tests import normal_cases as nc
from tests.popeval_cases import oracle_r2, pole_a2_steps
from tests.test_jacobian_oracle import KEYS, TARGETS

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
EINVAL, ESTATE = -1, -6
EPS = np.finfo(np.float64).eps
TOL = {"f64": (2e-9, 1e-9), "f32": (2e-5, 1e-5)}


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def test_error_codes_are_the_headers(L):
    src = open(os.path.join(os.path.dirname(G), os.pardir, "include", "alproj_hip.h")).read()
    import re
    assert int(re.search(r"ALP_EINVAL\s*=\s*(-?\d+)", src).group(1)) == EINVAL
    assert int(re.search(r"ALP_ESTATE\s*=\s*(-?\d+)", src).group(1)) == ESTATE


def g5():
    return np.load(os.path.join(G, "g5_population.npz"))


def lens_params():
    return orc.vector_to_params(g5()["params_init"])


def idx(targets):
    return [KEYS.index(t) for t in targets]


def synthetic(n, seed=1, sigma=2.0):
    """n GCPs in g5's camera (every lens term non-zero) and their pixels with `sigma` px of noise"""
    from alproj_amd import synthetic as syn
    p = lens_params()
    xyz = syn.gcp_points(n, p, seed=seed)
    uv = orc.project_points(xyz, p) + np.random.default_rng(seed).normal(0, sigma, (n, 2))
    return xyz, uv, p


def device_sums(L, xyz, uv, p, targets, precision="f64", loss="linear", f_scale=1.0):
    with L.Points(xyz, [p["x"], p["y"], p["z"]], precision) as pts:
        pts.set_observed(uv)
        return pts.normal_equations(L.params_vector(p), idx(targets), loss, f_scale)


def host_pieces(L, pts, pv, targets):
    """the oracle-shaped dict from the library's own Jacobian and residuals, contracted by numpy"""
    J = pts.jacobian(pv, idx(targets), of_residuals=True)
    r = pts.residuals(pv)
    return dict(G=J.T @ J, g=J.T @ r, cost=0.5 * float(r @ r), n=pts.n, Js=J, rs=r)


def assert_reassociation_only(got, ref):
    """test 6's bound: 4 m eps of the normalisers (the cost: of 0.5 m max|r|^2)"""
    Gm, g, cost, n = got
    m = 2 * n
    assert n == ref["n"]
    NG, Ng = nc.normalisers(ref["Js"], ref["rs"])
    tol = 4 * m * EPS
    np.testing.assert_array_equal(Gm, Gm.T)
    with np.errstate(invalid="ignore", divide="ignore"):
        eG = np.where(NG > 0, np.abs(Gm - ref["G"]) / NG, np.abs(Gm - ref["G"]))
        eg = np.where(Ng > 0, np.abs(g - ref["g"]) / Ng, np.abs(g - ref["g"]))
    assert (eG <= tol).all(), (eG.max(), tol)
    assert (eg <= tol).all(), (eg.max(), tol)
    assert abs(cost - ref["cost"]) <= tol * 0.5 * m * np.abs(ref["rs"]).max() ** 2, (cost, ref["cost"])


# ---------------------------------------------------------------------------------------------------- 5. the oracle
def median_scale(xyz, uv, p):
    """f_scale = the median |residual|: half the rows on either branch of huber"""
    r = nc.residual_vector(xyz, uv, orc.params_to_vector(p))
    fs = float(np.median(np.abs(r)))
    z = (r / fs) ** 2
    assert (z <= 1).sum() > len(r) // 4 and (z > 1).sum() > len(r) // 4
    return fs


@pytest.mark.parametrize("loss", nc.LOSSES)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_synthetic_gcps_all_23_targets(L, precision, loss):
    xyz, uv, p = synthetic(900)
    fs = median_scale(xyz, uv, p)
    got = device_sums(L, xyz, uv, p, TARGETS, precision, loss, fs)
    assert got[0].shape == (23, 23) and got[1].shape == (23,)
    nc.assert_sums_close(got, nc.normal_oracle(xyz, uv, orc.params_to_vector(p), TARGETS, loss, fs), *TOL[precision])


def g5_candidates():
    """candidates 0, 7 and 20 of g5's D = 21 population: tests/test_gpu_jacobian.py: g5_candidates says why not the others"""
    g = g5()
    init = orc.vector_to_params(g["params_init"])
    targets = [str(t) for t in g["d21_targets"]]
    return [orc.candidate_params(init, targets, g["d21_bounds"], g["d21_X"][k]) for k in (0, 7, 20)]


@pytest.mark.parametrize("loss", nc.LOSSES)
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_g5_candidates_all_23_targets(L, precision, loss, k):
    p = g5_candidates()[k]
    xyz, uv = g5()["xyz"], g5()["uv_obs"]
    fs = median_scale(xyz, uv, p)
    got = device_sums(L, xyz, uv, p, TARGETS, precision, loss, fs)
    nc.assert_sums_close(got, nc.normal_oracle(xyz, uv, orc.params_to_vector(p), TARGETS, loss, fs), *TOL[precision])


# ---------------------------------------------------------------------------------------------------- 6. the library's pieces
@pytest.mark.parametrize("n", [900, 1_000_003])
def test_equals_the_librarys_jacobian_and_residuals_contracted_on_the_host(L, n):
    xyz, uv, p = synthetic(n, seed=6)
    targets = TARGETS[:21]
    pv = L.params_vector(p)
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f64") as pts:
        pts.set_observed(uv)
        got = pts.normal_equations(pv, idx(targets))
        assert_reassociation_only(got, host_pieces(L, pts, pv, targets))


# ---------------------------------------------------------------------------------------------------- 7. launch shapes
D_TARGETS = {1: ["pan"], 14: TARGETS[:14], 15: TARGETS[4:19], 16: TARGETS[7:23], 23: TARGETS}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 100_003])
def test_launch_shapes(L, n):
    """M = D + 1 on both sides of the 16-wide block edge (15, 16, 17) and at its ends (2, 24), n around a wave, a group and
    several stripes; a call repeated gives the same bits; subsets and permutations of the targets are sub-blocks"""
    xyz, uv, p = synthetic(n, seed=n)
    pv = L.params_vector(p)
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f64") as pts:
        pts.set_observed(uv)
        full = None
        for D, targets in D_TARGETS.items():
            assert len(targets) == D
            got = pts.normal_equations(pv, idx(targets))
            again = pts.normal_equations(pv, idx(targets))
            for a, b in zip(got, again):
                np.testing.assert_array_equal(a, b)
            ref = host_pieces(L, pts, pv, targets)
            assert_reassociation_only(got, ref)
            if D == 23:
                full, full_ref = got, ref
        for cols in ([22, 1, 9, 17], [8], list(range(22, -1, -1)), [5, 0, 12, 16, 15, 17, 3, 21, 2, 20, 7, 8, 9, 10, 11, 13, 19]):
            sub = pts.normal_equations(pv, np.array(idx(TARGETS))[cols])
            ref = dict(G=full[0][np.ix_(cols, cols)], g=full[1][cols], cost=full[2], n=n, Js=full_ref["Js"][:, cols], rs=full_ref["rs"])
            assert_reassociation_only(sub, ref)


def test_empty_set_gives_zeros(L):
    pv = L.params_vector(lens_params())
    with L.Points(np.zeros((0, 3)), [0, 0, 0], "f64") as pts:
        pts.set_observed(np.zeros((0, 2)))
        Gm, g, cost, n = pts.normal_equations(pv, idx(["pan", "k1", "cx"]), "huber", 2.0)
    assert Gm.shape == (3, 3) and not Gm.any() and not g.any() and cost == 0.0 and n == 0


# ---------------------------------------------------------------------------------------------------- 8. errors, non-finite
def test_error_paths(L):
    xyz, uv, p = synthetic(64)
    lib = L.lib()
    I32 = ctypes.POINTER(ctypes.c_int32)
    pv = L.params_vector(p)
    out = np.empty(400)
    good = np.array(idx(["pan", "tilt"]), dtype=np.int32)
    tp = good.ctypes.data_as(I32)
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f64") as pts:
        call = lib.alp_normal_equations
        assert call(pts._h, L.as_dp(pv), tp, 2, 0, 1.0, L.as_dp(out)) == ESTATE          # no observed uv yet: alp_residuals' error
        r = np.empty(128)
        assert lib.alp_residuals(pts._h, L.as_dp(pv), L.as_dp(r)) == ESTATE
        pts.set_observed(uv)
        assert call(pts._h, L.as_dp(pv), tp, 2, 0, 1.0, L.as_dp(out)) == 0
        assert call(None, L.as_dp(pv), tp, 2, 0, 1.0, L.as_dp(out)) == EINVAL
        assert call(pts._h, None, tp, 2, 0, 1.0, L.as_dp(out)) == EINVAL
        assert call(pts._h, L.as_dp(pv), None, 2, 0, 1.0, L.as_dp(out)) == EINVAL
        assert call(pts._h, L.as_dp(pv), tp, 2, 0, 1.0, None) == EINVAL
        many = np.arange(25, dtype=np.int32)
        for D in (0, 24, -1):
            assert call(pts._h, L.as_dp(pv), many.ctypes.data_as(I32), D, 0, 1.0, L.as_dp(out)) == EINVAL
        for bad in ([KEYS.index("w")], [KEYS.index("pan"), KEYS.index("h")], [4, 4], [25], [-1]):
            b = np.array(bad, dtype=np.int32)
            assert call(pts._h, L.as_dp(pv), b.ctypes.data_as(I32), len(bad), 0, 1.0, L.as_dp(out)) == EINVAL, bad
        for loss in (-1, 4, 99):
            assert call(pts._h, L.as_dp(pv), tp, 2, loss, 1.0, L.as_dp(out)) == EINVAL
        for fs in (0.0, -1.0, float("inf"), float("nan")):
            assert call(pts._h, L.as_dp(pv), tp, 2, 2, fs, L.as_dp(out)) == EINVAL
        for loss in range(4):
            assert call(pts._h, L.as_dp(pv), tp, 2, loss, 1.5, L.as_dp(out)) == 0


def pole_problem(L):
    """tests/test_gpu_points.py's construction: k4 = -0.5, k5 = k6 = 0, so den_y = (1 + a2) - r2 / 2 of one chosen vertex is
    zero for exactly one value of 1 + a2; found on the device itself (alp_residuals_batch runs the arithmetic normal_kernel
    takes its residuals from) by stepping 1 + a2 ulp by ulp outward from the oracle's r2 / 2.  -> xyz, uv, truth, vertex, a2"""
    from alproj_amd import synthetic as syn
    truth = dict(syn.truth_params(316), k4=-0.5, k5=0.0, k6=0.0)
    xyz = syn.gcp_points(400, truth, seed=31, margin=-0.25)
    r2 = oracle_r2(xyz, truth)
    i0 = int(np.argmin(np.abs(r2 - 1.4)))
    keep = (np.abs(1 - r2 / 2) > 0.25) & (np.abs(1 + truth["a2"] - r2 / 2) > 0.25)
    keep[i0] = True
    i = int(np.count_nonzero(keep[:i0]))
    xyz, r2 = xyz[keep], r2[keep]
    uv = orc.project_points(xyz, truth) + np.random.default_rng(31).normal(0, 1.0, (len(xyz), 2))
    a2 = pole_a2_steps(r2[i], -0.5, "f64")
    order = np.argsort(np.abs(np.arange(len(a2)) - len(a2) // 2), kind="stable")       # from the centre outward
    with L.Points(xyz[i:i + 1], [truth["x"], truth["y"], truth["z"]], "f64") as one:
        one.set_observed(uv[i:i + 1])
        for c0 in range(0, len(order), 4096):
            sel = order[c0:c0 + 4096]
            cand = np.tile(L.params_vector(truth), (len(sel), 1))
            cand[:, KEYS.index("a2")] = a2[sel]
            res = one.residuals_batch(cand)
            hit = np.flatnonzero(~np.isfinite(res).all(axis=1))
            if len(hit):
                return xyz, uv, truth, i, float(a2[sel[hit[0]]])
    raise AssertionError("no candidate landed on the device's pole")


def test_a_point_on_a_lens_pole(L, monkeypatch):
    from alproj_amd import optimize as aopt
    xyz, uv, truth, i, a2_pole = pole_problem(L)
    targets = ["pan", "a2", "k1", "cx"]
    on = dict(truth, a2=a2_pole)
    Gm, g, cost, n = device_sums(L, xyz, uv, on, targets)
    # the v row of the vertex is infinite: the cost, and every sum a v derivative enters, is not finite; the call returned
    assert n == len(xyz) and not np.isfinite(cost)
    assert not np.isfinite(Gm[1, 1]) and not np.isfinite(g[1])
    # ... and one ulp-scale step away everything is finite again
    off = dict(truth, a2=a2_pole + 2.0 ** -20)
    sums = device_sums(L, xyz, uv, off, targets)
    assert np.isfinite(sums[0]).all() and np.isfinite(sums[1]).all() and np.isfinite(sums[2])

    # optimize(method="normal") next to the pole.  Target a2 alone, start at pole + d, box [pole, pole + 2 d]; the vertex's
    # observed v is what the model gives at pole + d / 4, i.e. 4 x as far out as at the start.  v ~ A / den: the first
    # (nearly undamped) Gauss-Newton step is -(v_obs den / A - 1) den = -3 d, clipped to the lower bound, which is the pole
    # itself: that trial is not finite and must be rejected; damped steps then walk down inside the box.
    d = 2.0 ** -20
    start = a2_pole + d
    assert start - d == a2_pole and start + d > start
    uv2 = uv.copy()
    uv2[i, 1] = orc.project_points(xyz[i:i + 1], dict(truth, a2=a2_pole + d / 4))[0, 1]
    assert np.isfinite(uv2[i, 1]) and abs(uv2[i, 1]) > 1e6
    seen = []
    plain = L.Points.normal_equations

    def recording(self, *a, **k):
        out = plain(self, *a, **k)
        seen.append(out[2])
        return out

    monkeypatch.setattr(L.Points, "normal_equations", recording)
    o = aopt.LsqOptimizer(pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv2, columns=["u", "v"]), dict(truth, a2=start))
    o.set_target(["a2"])
    params, err = o.optimize(method="normal", bound_widths={"a2": d})
    print("pole: costs seen", seen[:6], "result", o.result_)
    assert np.isfinite(seen[0]) and not np.isfinite(seen[1])             # the clipped first trial sat on the pole
    assert np.isfinite(o.result_["cost"]) and o.result_["cost"] < seen[0] and np.isfinite(err)
    assert a2_pole < params["a2"] <= a2_pole + 2 * d
    assert o.result_["evaluations"] > o.result_["iterations"] + 1


# ---------------------------------------------------------------------------------------------------- 9. communicator
def test_world_1_communicator_gives_the_same_bits(L):
    xyz, uv, p = synthetic(70_001, seed=9)
    pv = L.params_vector(p)
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f32") as pts:
        pts.set_observed(uv)
        before = pts.normal_equations(pv, idx(TARGETS), "soft_l1", 1.5)
        L.comm_init(L.comm_unique_id(), 0, 1)
        try:
            assert L.comm_info() == (0, 1)
            during = pts.normal_equations(pv, idx(TARGETS), "soft_l1", 1.5)
        finally:
            L.comm_destroy()
        after = pts.normal_equations(pv, idx(TARGETS), "soft_l1", 1.5)
    for other in (during, after):
        for a, b in zip(before, other):
            np.testing.assert_array_equal(a, b)
    assert before[3] == 70_001


# ---------------------------------------------------------------------------------------------------- 10. the optimiser
def frames(prob):
    return pd.DataFrame(prob["xyz"], columns=["x", "y", "z"]), pd.DataFrame(prob["uv"], columns=["u", "v"])


@pytest.mark.parametrize("case", list(nc.LSQ_KW))
def test_optimize_normal_reaches_the_reference_optimum(L, case):
    from alproj_amd import optimize as aopt
    prob = nc.g14_problem(case)
    kw = nc.LSQ_KW[case]
    loss, f_scale = kw.get("loss", "linear"), kw.get("f_scale", 1.0)
    o = aopt.LsqOptimizer(*frames(prob), dict(prob["init"]))
    o.set_target(prob["targets"])
    params, err = o.optimize(method="normal", bound_widths=nc.widths_of(case), loss=loss, f_scale=f_scale)
    print(case, o.result_)
    assert set(params) == set(prob["want"]) and set(o.result_) == {"cost", "iterations", "evaluations", "status", "grad_norm"}
    assert o.result_["status"] in (1, 2, 3, 4)
    assert o.result_["cost"] == pytest.approx(nc.cost_at(prob, params, loss, f_scale), rel=1e-9)
    nc.assert_reference_optimum(prob, params, err, o.result_["cost"], loss, f_scale)


@pytest.mark.parametrize("name", list(nc.ACTIVE))
def test_optimize_normal_with_active_bounds(L, name):
    from alproj_amd import optimize as aopt
    case, widths = nc.ACTIVE[name]
    prob = nc.g14_problem(case)
    lower, upper = nc.bounds_of(prob, widths)
    o = aopt.LsqOptimizer(*frames(prob), dict(prob["init"]))
    o.set_target(prob["targets"])
    params, err = o.optimize(method="normal", bound_widths=widths)
    print(name, o.result_)
    x = np.array([params[t] for t in prob["targets"]])
    _, scipy_cost = nc.scipy_trf_on_the_oracle(prob, lower, upper)
    nc.assert_active_optimum(x, o.result_["cost"], lower, upper, scipy_cost)


def test_optimize_normal_on_a_float32_set(L):
    """precision="f32" through the public class: the set stores float32 coordinates and pixels, the arithmetic stays float64.
    tests/test_gpu_points.py holds a float32 projection to 1e-5 of the image width; residuals perturbed by at most e = 1e-5 w
    each move the least-squares solution by at most |pinv(J)[k, :]| |dr| <= |pinv(J)[k, :]| e sqrt(m) in parameter k (first
    order; a factor of 2 for the perturbation of J itself), J = the Jacobian at the float64 solution."""
    from alproj_amd import optimize as aopt
    prob = nc.g14_problem("trf_linear_d7")
    got = {}
    for precision in ("f64", "f32"):
        o = aopt.LsqOptimizer(*frames(prob), dict(prob["init"]))
        o.set_target(prob["targets"])
        got[precision] = o.optimize(method="normal", precision=precision)
        assert o.result_["status"] in (1, 2, 3, 4), o.result_
    p64, p32 = got["f64"][0], got["f32"][0]
    with L.Points(prob["xyz"], [p64["x"], p64["y"], p64["z"]], "f64") as pts:
        J = pts.jacobian(L.params_vector(p64), idx(prob["targets"]))
    e = 1e-5 * float(prob["init"]["w"])
    bound = 2 * np.linalg.norm(np.linalg.pinv(J), axis=1) * e * np.sqrt(J.shape[0])
    for k, t in enumerate(prob["targets"]):
        print("  %-5s f32 - f64 %.3g (bound %.3g)" % (t, abs(p32[t] - p64[t]), bound[k]))
        assert abs(p32[t] - p64[t]) <= bound[k], (t, p32[t], p64[t], bound[k])
    assert abs(got["f32"][1] - got["f64"][1]) <= 2 * e


# ---------------------------------------------------------------------------------------------------- 11. covariance
def covariance_cases():
    out = []
    for case in ("trf_linear_d7", "trf_linear_dist_d6"):
        prob = nc.g14_problem(case)
        out.append((case, prob["xyz"], prob["uv"], prob["want"], prob["targets"]))
    g = g5()
    out.append(("g5_d21", g["xyz"], g["uv_obs"], orc.vector_to_params(g["params_init"]), TARGETS[:21]))
    return out


@pytest.mark.parametrize("k", [0, 1, 2], ids=["g14_d7", "g14_d6", "g5_d21"])
def test_parameter_covariance_normal_against_the_default(L, k):
    from alproj_amd import optimize as aopt
    name, xyz, uv, p, targets = covariance_cases()[k]
    dfx, dfu = pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"])
    cov, std = aopt.parameter_covariance(dfx, dfu, p, targets)
    cov_n, std_n = aopt.parameter_covariance(dfx, dfu, p, targets, method="normal")
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f64") as pts:
        J = pts.jacobian(L.params_vector(p), idx(targets))
    kappa = np.linalg.cond(J / np.linalg.norm(J, axis=0))
    s = np.sqrt(np.diag(cov))
    diff = np.abs(cov_n - cov) / np.outer(s, s)
    print("%s: kappa %.3g, max normalised difference %.3g, bound %.3g" % (name, kappa, diff.max(), 100 * kappa ** 2 * EPS))
    assert np.isfinite(cov).all() and np.isfinite(cov_n).all()
    assert (diff <= 100 * kappa ** 2 * EPS).all(), (diff.max(), kappa)
    assert list(std_n) == list(std) == list(targets)
    np.testing.assert_array_equal([std_n[t] for t in targets], np.sqrt(np.diag(cov_n)))


def test_parameter_covariance_normal_rank_deficient_is_inf(L):
    """tests/test_gpu_jacobian.py's case: with every lens term zero the k1 and k4 columns are exact negatives"""
    from alproj_amd import optimize as aopt
    from alproj_amd import synthetic as syn
    p = dict(lens_params(), **{k: 0.0 for k in orc.DIST_KEYS})
    xyz = syn.gcp_points(300, p, seed=1)
    uv = orc.project_points(xyz, p) + np.random.default_rng(4).normal(0, 0.5, (300, 2))
    dfx, dfu = pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"])
    for method in ("svd", "normal"):
        cov, std = aopt.parameter_covariance(dfx, dfu, p, ["fov", "k1", "k4"], method=method)
        assert np.isinf(cov).all() and all(np.isinf(v) for v in std.values()), method
    with pytest.raises(ValueError):
        aopt.parameter_covariance(dfx.iloc[:2], dfu.iloc[:2], p, ["fov", "pan", "tilt", "roll", "k1"], method="normal")
