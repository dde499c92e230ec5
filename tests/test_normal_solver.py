"""CPU: the host half of the normal-equations path.

1. ``normal_lm`` (alproj_amd/optimize.py), fed by the complex-step oracle of tests/normal_cases.py instead of the device,
   reaches the reference's own optima of tests/golden/g14_lsq.npz within the limits tests/test_gpu_golden_render.py holds the
   scipy runs to, at a cost not above the cost at the reference's parameters.
2. With narrowed widths the optimum lies on a bound: in the box, a variable exactly on a bound, cost not above scipy trf's.
3. host/alp_plan.h: normal_grid through the self-checking driver (--plan) against the Python restatement.
4. The refusals of ``Points.normal_equations`` and ``optimize(method="normal")`` come before any GPU call, and the header
   declares the entry point."""
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

from tests import normal_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- 1. reference optima
@pytest.mark.parametrize("case", list(nc.LSQ_KW))
def test_solver_on_the_oracle_reaches_the_reference_optimum(case):
    from alproj_amd import optimize as aopt
    prob = nc.g14_problem(case)
    kw = nc.LSQ_KW[case]
    loss, f_scale = kw.get("loss", "linear"), kw.get("f_scale", 1.0)
    lower, upper = nc.bounds_of(prob, nc.widths_of(case))
    if kw.get("unbounded"):
        assert np.isinf(lower).all() and np.isinf(upper).all()
    x0 = np.array([prob["init"][t] for t in prob["targets"]])
    res = aopt.normal_lm(nc.oracle_sums(prob, loss, f_scale), x0, lower, upper)
    print(case, {k: res[k] for k in ("iterations", "evaluations", "status", "grad_norm")})
    assert res["status"] in (1, 2, 3, 4)
    params = dict(prob["init"], **dict(zip(prob["targets"], res["x"])))
    assert res["cost"] == pytest.approx(nc.cost_at(prob, params, loss, f_scale), rel=1e-12)
    nc.assert_reference_optimum(prob, params, nc.mean_distance(prob, params), res["cost"], loss, f_scale)


# ---------------------------------------------------------------------------------------------------- 2. active bounds
@pytest.mark.parametrize("name", list(nc.ACTIVE))
def test_solver_on_the_oracle_with_active_bounds(name):
    from alproj_amd import optimize as aopt
    case, widths = nc.ACTIVE[name]
    prob = nc.g14_problem(case)
    lower, upper = nc.bounds_of(prob, widths)
    x0 = np.array([prob["init"][t] for t in prob["targets"]])
    res = aopt.normal_lm(nc.oracle_sums(prob), x0, lower, upper)
    print(name, {k: res[k] for k in ("iterations", "evaluations", "status", "grad_norm")})
    xs, scipy_cost = nc.scipy_trf_on_the_oracle(prob, lower, upper)
    print("  max |dx| / width against scipy: %.3g" % np.max(np.abs(res["x"] - xs) / (upper - lower)))
    nc.assert_active_optimum(res["x"], res["cost"], lower, upper, scipy_cost)


def test_solver_stops_at_once_where_the_gradient_vanishes_and_reports_a_cost_that_is_not_finite():
    from alproj_amd import optimize as aopt
    quad = lambda x: (np.eye(2), x.copy(), 0.5 * float(x @ x))
    res = aopt.normal_lm(quad, np.zeros(2), np.full(2, -1.0), np.full(2, 1.0))
    assert res["status"] == 1 and res["evaluations"] == 1 and res["iterations"] == 0
    # the minimum of 0.5 |x|^2 over [0.25, 1] x [-1, 1]: on the first bound
    res = aopt.normal_lm(quad, np.array([0.5, 0.5]), np.array([0.25, -1.0]), np.array([1.0, 1.0]))
    assert res["x"][0] == 0.25 and abs(res["x"][1]) < 1e-9 and res["status"] in (1, 2, 3, 4)
    bad = lambda x: (np.eye(2), x.copy(), float("nan"))
    assert aopt.normal_lm(bad, np.ones(2), np.full(2, -2.0), np.full(2, 2.0))["status"] == -1
    # a trial point whose sums are not finite is rejected: the walk goes on from the last finite point
    def pole(x):
        c = 0.5 * float(x @ x) if x[0] > 0.4 else float("inf")
        return np.eye(2), x.copy(), c
    res = aopt.normal_lm(pole, np.array([0.5, 0.5]), np.full(2, -1.0), np.full(2, 1.0))
    assert np.isfinite(res["cost"]) and res["x"][0] > 0.4 and res["cost"] < 0.5 * 0.5


# ---------------------------------------------------------------------------------------------------- 3. the plan
def test_normal_grid_is_the_restated_rule():
    from alproj_amd import _build
    if _build.host_compiler("clang") is None:
        pytest.skip("no clang compiler")
    exe = _build.build_host("plain", "clang")
    cases = [(n, cu) for n in (0, 1, 255, 256, 257, 10 ** 5, 10 ** 8) for cu in (1, 64, 256, 304, 1024)]
    text = "".join(f"normal,{n},{cu}\n" for n, cu in cases)
    r = subprocess.run([exe, "--plan"], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(cases)
    for (n, cu), g in zip(cases, got):
        assert g == nc.normal_grid(n, cu), (n, cu, g)
        blocks, per = g
        groups = -(-n // 256)
        assert blocks <= min(nc.MAX_BLOCKS, cu * nc.WG_PER_CU)
        assert blocks * per >= groups and (blocks == 0 or (blocks - 1) * per < groups)        # covered, no empty workgroup
    assert nc.normal_grid(10 ** 7, 256) == (1503, 26)
    assert subprocess.run([exe, "--plan", "normal,-1,256"], capture_output=True).returncode == 2


# ---------------------------------------------------------------------------------------------------- 4. refusals
def test_header_declares_the_entry_point_and_cites_the_reference():
    src = open(os.path.join(ROOT, "include", "alproj_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int alp_normal_equations\(", src, flags=re.S)
    assert m, "alp_normal_equations is not declared"
    assert "src/alproj/optimize.py:215-237" in m.group(1) and ":442-539" in m.group(1)
    from alproj_amd import _lib
    assert "alp_normal_equations" in _lib._SIGNATURES
    assert int(re.search(r"#define ALP_ABI_VERSION (\d+)", src).group(1)) == 7


class NoDevice:
    """a Points stand-in whose library must never be reached"""
    n = 10

    class _lib:
        @staticmethod
        def alp_normal_equations(*a):
            raise AssertionError("the library was called")

    _h = None


def test_points_normal_equations_refuses_before_the_library():
    from alproj_amd import _lib
    pv = np.zeros(_lib.NPARAM)
    call = lambda *a, **k: _lib.Points.normal_equations(NoDevice(), *a, **k)
    K = _lib.PARAM_KEYS.index
    for targets in ([K("w")], [K("pan"), K("h")], [K("pan"), K("pan")], [], list(range(21)) + [23, 24, 0], [25], [-1]):
        with pytest.raises(ValueError):
            call(pv, targets)
    for f_scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            call(pv, [K("pan")], "huber", f_scale)
    with pytest.raises(ValueError):
        call(pv, [K("pan")], "arctan", 1.0)
    with pytest.raises(ValueError):
        call(np.zeros(24), [K("pan")])
    with pytest.raises(AssertionError):           # a good call does reach the library
        call(pv, [K("pan")], "cauchy", 2.0)


def test_optimize_normal_refuses_before_any_gpu_call(monkeypatch):
    from alproj_amd import optimize as aopt
    prob = nc.g14_problem("trf_linear_d7")
    dfx = pd.DataFrame(prob["xyz"], columns=["x", "y", "z"])
    dfu = pd.DataFrame(prob["uv"], columns=["u", "v"])

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(aopt.BaseOptimizer, "_device_points", no_device)
    monkeypatch.setattr(aopt._lib, "lib", no_device)

    def opt(targets):
        o = aopt.LsqOptimizer(dfx, dfu, dict(prob["init"]))
        o.set_target(targets)
        return o

    for targets in (["pan", "w"], ["h"], ["pan", "tilt", "pan"]):
        with pytest.raises(ValueError):
            opt(targets).optimize(method="normal")
    for jac in ("analytic", "batched", "2-point", None):
        with pytest.raises(ValueError):
            opt(["pan", "tilt"]).optimize(method="normal", jac=jac)
    for f_scale in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            opt(["pan", "tilt"]).optimize(method="normal", loss="huber", f_scale=f_scale)
    with pytest.raises(ValueError):
        opt(["pan", "tilt"]).optimize(method="normal", loss="arctan")
    with pytest.raises(TypeError):
        opt(["pan", "tilt"]).optimize(method="normal", x_scale="jac")
    with pytest.raises(AssertionError):           # a good call does go on to the device
        opt(["pan", "tilt"]).optimize(method="normal")
    with pytest.raises(ValueError):
        aopt.parameter_covariance(dfx, dfu, prob["init"], ["pan"], method="qr")
