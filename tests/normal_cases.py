"""Oracle and cases of the normal-equations path (alp_normal_equations, LsqOptimizer.optimize(method="normal"),
parameter_covariance(method="normal")), shared by tests/test_normal_solver.py (CPU) and tests/test_gpu_normal.py (GPU).

- ``normal_oracle``: J^T J, J^T r and the cost from the complex-step Jacobian and the complex-safe projection of
  tests/test_jacobian_oracle.py, with scipy's rho formulas (scipy/optimize/_lsq/least_squares.py: soft_l1, huber, cauchy) and
  the row scaling of its scale_for_robust_loss_function -- the floor under rho' + 2 z rho'' is the 1e-10 the library states.
- ``normal_grid``: the Python restatement of host/alp_plan.h: normal_grid.
- the solver problems: the six least-squares runs of tests/golden/g14_lsq.npz with the options of LSQ_KW
  (tests/test_gpu_golden_render.py), and four problems with narrowed widths whose optimum lies on a bound."""
import os

import numpy as np

from tests.test_jacobian_oracle import KEYS, cs_jacobian, cs_project

G14 = os.path.join(os.path.dirname(__file__), "golden", "g14_lsq.npz")
POSE_KEYS = ("x", "y", "z", "fov", "pan", "tilt", "roll")
LOSSES = ("linear", "soft_l1", "huber", "cauchy")
FLOOR = 1e-10


# ---------------------------------------------------------------------------------------------------- the oracle
def rho(z, loss):
    """(rho, rho', rho'') of scipy's losses at z = (r / f_scale)^2"""
    z = np.asarray(z, dtype=np.float64)
    if loss == "linear":
        return z, np.ones_like(z), np.zeros_like(z)
    if loss == "soft_l1":
        t = 1 + z
        return 2 * (t ** 0.5 - 1), t ** -0.5, -0.5 * t ** -1.5
    if loss == "huber":
        out = np.empty((3,) + z.shape)
        m = z <= 1
        zz = np.where(m, 1.0, z)
        out[0] = np.where(m, z, 2 * zz ** 0.5 - 1)
        out[1] = np.where(m, 1.0, zz ** -0.5)
        out[2] = np.where(m, 0.0, -0.5 * zz ** -1.5)
        return out[0], out[1], out[2]
    if loss == "cauchy":
        t = 1 + z
        return np.log1p(z), 1 / t, -1 / t ** 2
    raise ValueError(loss)


def residual_vector(xyz, uv, pvec):
    u, v = cs_project(xyz, np.asarray(pvec, dtype=np.float64).astype(np.complex128))
    r = np.empty(2 * len(xyz))
    r[0::2] = uv[:, 0] - np.real(u)
    r[1::2] = uv[:, 1] - np.real(v)
    return r


def normal_oracle(xyz, uv, pvec, targets, loss="linear", f_scale=1.0):
    """dict: G = Js^T Js (D, D), g = Js^T rs (D,), cost = 0.5 f_scale^2 sum rho, n, and Js (2N, D), rs (2N,) themselves:
    the rows of the Jacobian of observed - projected and the residuals, scaled for the loss"""
    xyz, uv = np.asarray(xyz, dtype=np.float64), np.asarray(uv, dtype=np.float64)
    J = cs_jacobian(xyz, pvec, list(targets), of_residuals=True)
    r = residual_vector(xyz, uv, pvec)
    z = (r / f_scale) ** 2
    r0, r1, r2 = rho(z, loss)
    s = np.sqrt(np.maximum(r1 + 2 * z * r2, FLOOR))
    Js, rs = J * s[:, None], r * r1 / s
    return dict(G=Js.T @ Js, g=Js.T @ rs, cost=0.5 * f_scale ** 2 * float(np.sum(r0)), n=len(xyz), Js=Js, rs=rs)


def normalisers(Js, rs):
    """(NG (D, D), Ng (D,)): m max|J_i| max|J_j| and m max|J_i| max|r|, m = the number of rows"""
    m = len(rs)
    cj = np.abs(Js).max(axis=0) if m else np.zeros(Js.shape[1])
    return m * np.outer(cj, cj), m * cj * (np.abs(rs).max() if m else 0.0)


def assert_sums_close(got, ref, tol_sum, tol_cost):
    """got = (G, g, cost, n) of Points.normal_equations, ref = normal_oracle's dict (or any dict with G, g, cost, n, Js, rs)"""
    G, g, cost, n = got
    assert n == ref["n"]
    NG, Ng = normalisers(ref["Js"], ref["rs"])
    assert G.shape == ref["G"].shape and g.shape == ref["g"].shape
    np.testing.assert_array_equal(G, G.T)
    eG = np.abs(G - ref["G"]) / NG
    eg = np.abs(g - ref["g"]) / Ng
    print("normal sums: max err G %.3g, g %.3g (tol %.3g); cost rel %.3g (tol %.3g)" %
          (eG.max(), eg.max(), tol_sum, abs(cost - ref["cost"]) / abs(ref["cost"]) if ref["cost"] else 0.0, tol_cost))
    assert (eG <= tol_sum).all(), eG.max()
    assert (eg <= tol_sum).all(), eg.max()
    assert abs(cost - ref["cost"]) <= tol_cost * abs(ref["cost"]), (cost, ref["cost"])


# ---------------------------------------------------------------------------------------------------- the launch plan
WG_PER_CU, MAX_BLOCKS = 6, 2048


def normal_grid(n, cus):
    """(workgroups, groups of 256 points per workgroup) of host/alp_plan.h: normal_grid"""
    groups = -(-n // 256)
    if groups <= 0:
        return 0, 0
    want = min(cus * WG_PER_CU, MAX_BLOCKS, groups)
    per = -(-groups // want)
    return -(-groups // per), per


# ---------------------------------------------------------------------------------------------------- solver problems
LSQ_KW = {"trf_linear_d7": dict(),
          "trf_huber_d7": dict(loss="huber", f_scale=5.0),
          "dogbox_softl1_d4": dict(loss="soft_l1", f_scale=3.0, bound_widths={"fov": 10, "pan": 10, "tilt": 10, "roll": 10}),
          "trf_cauchy_d4": dict(loss="cauchy", f_scale=2.0),
          "lm_d4": dict(unbounded=True),
          "trf_linear_dist_d6": dict()}
ACTIVE = {"d7_pan_fov": ("trf_linear_d7", {"pan": 0.5, "fov": 1.0}),
          "d7_tilt_x": ("trf_linear_d7", {"tilt": 0.25, "x": 1.0}),
          "d4_pan": ("lm_d4", {"pan": 0.5}),
          "d6_k1_a1": ("trf_linear_dist_d6", {"k1": 0.01, "a1": 0.05})}


def g14_problem(case):
    """dict of one g14 run: xyz, uv, init (dict), targets, want (dict: the reference's optimum), error"""
    g = np.load(G14)
    keys = [str(k) for k in g["param_keys"]]
    return dict(xyz=g["xyz"], uv=g["uv_" + str(g[f"{case}_uv"])], init=dict(zip(keys, g[f"{case}_init"])),
                targets=[str(t) for t in g[f"{case}_targets"]], want=dict(zip(keys, g[f"{case}_params"])),
                error=float(g[f"{case}_error"]), keys=keys)


def widths_of(case):
    """the bound_widths argument of a g14 run under method="normal": LSQ_KW's own, all infinite for the unbounded lm run"""
    kw = LSQ_KW[case]
    if kw.get("unbounded"):
        return {t: np.inf for t in g14_problem(case)["targets"]}
    return kw.get("bound_widths")


def oracle_sums(prob, loss="linear", f_scale=1.0):
    """values -> (G, g, cost): the callable normal_lm takes, from normal_oracle"""
    base = np.array([prob["init"][k] for k in KEYS], dtype=np.float64)
    cols = [KEYS.index(t) for t in prob["targets"]]

    def fun(values):
        p = base.copy()
        p[cols] = values
        o = normal_oracle(prob["xyz"], prob["uv"], p, prob["targets"], loss, f_scale)
        return o["G"], o["g"], o["cost"]

    return fun


def cost_at(prob, params, loss="linear", f_scale=1.0):
    p = np.array([params[k] for k in KEYS], dtype=np.float64)
    r = residual_vector(prob["xyz"], prob["uv"], p)
    return 0.5 * f_scale ** 2 * float(np.sum(rho((r / f_scale) ** 2, loss)[0]))


def mean_distance(prob, params):
    p = np.array([params[k] for k in KEYS], dtype=np.float64)
    r = residual_vector(prob["xyz"], prob["uv"], p).reshape(-1, 2)
    return float(np.mean(np.hypot(r[:, 0], r[:, 1])))


def assert_reference_optimum(prob, params, err, cost, loss, f_scale):
    """the limits of tests/test_gpu_golden_render.py::test_g14_*: 2e-4 pose, 2e-6 lens, error rel 5e-5; and the cost is not
    above the cost at the reference's own parameters"""
    for k in prob["targets"]:
        tol = 2e-4 if k in POSE_KEYS else 2e-6
        print("  %-5s deviation %.3g (tol %.3g)" % (k, abs(params[k] - prob["want"][k]), tol))
        assert abs(params[k] - prob["want"][k]) <= tol, (k, params[k], prob["want"][k])
    assert abs(err - prob["error"]) <= 5e-5 * abs(prob["error"]), (err, prob["error"])
    ref_cost = cost_at(prob, prob["want"], loss, f_scale)
    print("  cost %.12g, at the reference's parameters %.12g (rel %.3g)" % (cost, ref_cost, cost / ref_cost - 1))
    assert cost <= ref_cost * (1 + 1e-7), (cost, ref_cost)


def scipy_trf_on_the_oracle(prob, lower, upper):
    """scipy.optimize.least_squares(method="trf") with the complex-step Jacobian, ftol = xtol = gtol = 1e-12 -> (x, cost)"""
    from scipy.optimize import least_squares
    base = np.array([prob["init"][k] for k in KEYS], dtype=np.float64)
    cols = [KEYS.index(t) for t in prob["targets"]]

    def pv(values):
        p = base.copy()
        p[cols] = values
        return p

    res = least_squares(lambda v: residual_vector(prob["xyz"], prob["uv"], pv(v)), base[cols],
                        jac=lambda v: cs_jacobian(prob["xyz"], pv(v), prob["targets"]), method="trf", bounds=(lower, upper),
                        ftol=1e-12, xtol=1e-12, gtol=1e-12)
    return res.x, float(res.cost)


def assert_active_optimum(x, cost, lower, upper, scipy_cost):
    assert ((x >= lower) & (x <= upper)).all(), (x, lower, upper)
    on = (x == lower) | (x == upper)
    print("  on a bound: %d variable(s); cost %.12g, scipy trf %.12g (rel %.3g)" % (on.sum(), cost, scipy_cost, cost / scipy_cost - 1))
    assert on.any()
    assert cost <= scipy_cost * (1 + 1e-9), (cost, scipy_cost)


def bounds_of(prob, widths):
    from alproj_amd import optimize as aopt
    b = aopt.bounds_to_array(prob["init"], prob["targets"], widths)
    return b[:, 0], b[:, 1]
