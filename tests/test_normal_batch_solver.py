"""CPU: the host half of the batched normal-equations path.

1. ``normal_lm_batch`` (alproj_amd/optimize.py) on the complex-step oracle of tests/normal_cases.py applied row by row: every
   start ends with the bits ``normal_lm`` run alone from that start ends with -- x, cost, iterations, evaluations, status.
   K = 5 starts by the integer rule (tests/normal_batch_cases.py), on the six g14 runs of nc.LSQ_KW and the four active-bound
   problems of nc.ACTIVE.  The unbounded run (lm_d4) has no box to draw in: its starts are drawn in the box of the default
   widths and solved without bounds.
2. Lockstep accounting: as many ``fun`` calls as the longest start has evaluations, as many rows as all starts have
   evaluations, and call r holds evaluation r of every start that has one, in start order.
3. A start whose first cost is not finite ends with status -1 and leaves the others as they are; a trial that is not finite is
   rejected and the start goes on.
4. host/alp_plan.h: normal_batch_grid through the self-checking driver (--plan) against the restated rule and its invariants.
5. The refusals of ``Points.normal_equations_batch`` and ``optimize(method="normal", starts=...)`` come before any library
   call; the integer draw is reproducible; the header declares the entry point."""
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

from tests import normal_batch_cases as nb
from tests import normal_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 5
KEYS_EQUAL = ("cost", "iterations", "evaluations", "status")

PROBLEMS = {case: (case, nc.widths_of, nc.LSQ_KW[case].get("loss", "linear"), nc.LSQ_KW[case].get("f_scale", 1.0)) for case in nc.LSQ_KW}
PROBLEMS.update({name: (case, (lambda _case, w=widths: w), "linear", 1.0) for name, (case, widths) in nc.ACTIVE.items()})


def problem(name):
    """-> fun (one point, remembered), X0 (K, D), lower, upper"""
    case, widths_of, loss, f_scale = PROBLEMS[name]
    prob = nc.g14_problem(case)
    lower, upper = nc.bounds_of(prob, widths_of(case))
    box = (lower, upper) if np.isfinite(lower).all() else nc.bounds_of(prob, None)
    x_init = np.array([prob["init"][t] for t in prob["targets"]])
    X0 = nb.integer_starts(x_init, box[0], box[1], K, seed=len(name))
    return nb.remembered(nc.oracle_sums(prob, loss, f_scale)), X0, lower, upper


def assert_same_run(got, alone):
    np.testing.assert_array_equal(got["x"], alone["x"])
    for k in KEYS_EQUAL + ("grad_norm",):
        assert type(got[k]) is type(alone[k]), (k, got[k], alone[k])
        np.testing.assert_array_equal(got[k], alone[k], err_msg=k)            # equal values; NaN equals NaN
    assert set(got) == set(alone)


# ---------------------------------------------------------------------------------------------------- 1. + 2.
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_lockstep_runs_are_the_sequential_runs_bit_for_bit(name):
    from alproj_amd import optimize as aopt
    fun, X0, lower, upper = problem(name)
    assert X0.shape[0] == K and (X0[1:] != X0[0]).any(axis=1).all()
    calls = []
    got = aopt.normal_lm_batch(nb.row_by_row(fun, calls), X0, lower, upper)
    assert len(got) == K
    trails = []
    for k in range(K):
        trail = []

        def recording(x, trail=trail):
            trail.append(np.array(x, dtype=np.float64))
            return fun(x)

        alone = aopt.normal_lm(recording, X0[k], lower, upper)
        assert len(trail) == alone["evaluations"]
        assert_same_run(got[k], alone)
        trails.append(trail)
    print(name, "evaluations", [r["evaluations"] for r in got], "status", [r["status"] for r in got], "calls", len(calls))
    assert any(r["status"] in (1, 2, 3, 4) for r in got)
    # the accounting: one call per round, evaluation r of every start that has one, in start order
    assert len(calls) == max(r["evaluations"] for r in got)
    assert sum(len(X) for X in calls) == sum(r["evaluations"] for r in got)
    for r, X in enumerate(calls):
        want = [trails[k][r] for k in range(K) if len(trails[k]) > r]
        np.testing.assert_array_equal(X, np.array(want))


def test_one_start_is_normal_lm_and_max_nfev_counts_per_start():
    from alproj_amd import optimize as aopt
    fun, X0, lower, upper = problem("trf_cauchy_d4")
    one = aopt.normal_lm_batch(nb.row_by_row(fun), X0[:1], lower, upper)
    assert len(one) == 1
    assert_same_run(one[0], aopt.normal_lm(fun, X0[0], lower, upper))
    calls = []
    capped = aopt.normal_lm_batch(nb.row_by_row(fun, calls), X0, lower, upper, max_nfev=6)
    for k in range(K):
        assert capped[k]["evaluations"] <= 6
        assert_same_run(capped[k], aopt.normal_lm(fun, X0[k], lower, upper, max_nfev=6))
    assert [r["status"] for r in capped].count(0) >= 2 and len(calls) == 6
    with pytest.raises(ValueError):
        aopt.normal_lm_batch(nb.row_by_row(fun), X0[0], lower, upper)


# ---------------------------------------------------------------------------------------------------- 3. non-finite
def test_a_start_that_is_not_finite_and_a_trial_that_is_not_finite():
    from alproj_amd import optimize as aopt

    def pole(x):            # tests/test_normal_solver.py's: a wall at x[0] = 0.4
        c = 0.5 * float(x @ x) if x[0] > 0.4 else float("inf")
        return np.eye(2), x.copy(), c

    def bad_beyond(x):      # ... and nothing finite at x[1] > 0.8
        G, g, c = pole(x)
        return (G, g, float("nan")) if x[1] > 0.8 else (G, g, c)

    lower, upper = np.full(2, -1.0), np.full(2, 1.0)
    X0 = np.array([[0.5, 0.5], [0.6, 0.9], [0.9, -0.7], [0.2, 0.1]])
    calls = []
    got = aopt.normal_lm_batch(nb.row_by_row(bad_beyond, calls), X0, lower, upper)
    for k in range(4):
        assert_same_run(got[k], aopt.normal_lm(bad_beyond, X0[k], lower, upper))
    assert got[1]["status"] == -1 and got[1]["evaluations"] == 1 and np.isnan(got[1]["cost"])
    assert got[3]["status"] == -1 and np.isinf(got[3]["cost"])
    np.testing.assert_array_equal(got[1]["x"], X0[1])
    for k in (0, 2):        # rejected the trial beyond the wall and went on
        assert np.isfinite(got[k]["cost"]) and got[k]["x"][0] > 0.4 and got[k]["cost"] < 0.5 * float(X0[k] @ X0[k])
        assert got[k]["evaluations"] > got[k]["iterations"] + 1
    assert len(calls[0]) == 4 and all(len(X) == 2 for X in calls[1:min(got[0]["evaluations"], got[2]["evaluations"])])
    # the others are what they are without the two bad starts
    clean = aopt.normal_lm_batch(nb.row_by_row(bad_beyond), X0[[0, 2]], lower, upper)
    assert_same_run(clean[0], got[0])
    assert_same_run(clean[1], got[2])


# ---------------------------------------------------------------------------------------------------- 4. the plan
def test_normal_batch_grid_is_the_restated_rule():
    from alproj_amd import _build
    if _build.host_compiler("clang") is None:
        pytest.skip("no clang compiler")
    exe = _build.build_host("plain", "clang")
    cases = [(n, B, cu) for n in (0, 1, 255, 256, 257, 1127, 10 ** 5, 10 ** 8) for B in (1, 2, 3, 64, 1000, 1024) for cu in (1, 64, 256, 304)]
    text = "".join(f"normal_batch,{n},{B},{cu}\n" for n, B, cu in cases)
    r = subprocess.run([exe, "--plan"], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(cases)
    for (n, B, cu), g in zip(cases, got):
        assert g == nb.normal_batch_grid(n, B, cu), (n, B, cu, g)
        blocks, per = g
        groups = -(-n // 256)
        if B == 1:
            assert g == nc.normal_grid(n, cu)
        if n == 0:
            assert g == (0, 0)
            continue
        want = min(nc.MAX_BLOCKS, cu * nc.WG_PER_CU)
        assert blocks >= 1 and per >= 1
        assert blocks * per >= groups and (blocks - 1) * per < groups            # every group covered, no empty workgroup
        assert blocks * B < want + B                                             # the partial rows
        assert blocks * B * 300 * 8 <= (nc.MAX_BLOCKS + nb.BATCH_MAX) * 300 * 8
    assert nb.normal_batch_grid(1127, 64, 256) == (5, 1)                         # the GCP size: 320 workgroups instead of 5
    assert nb.normal_batch_grid(10 ** 7, 8, 256) == (192, 204)
    for bad in ("normal_batch,1127,0,256", "normal_batch,1127,-1,256", "normal_batch,1127,1025,256", "normal_batch,-1,1,256",
                "normal_batch,1127,2"):
        assert subprocess.run([exe, "--plan", bad], capture_output=True).returncode == 2, bad


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_header_declares_the_batch_entry_point_and_cites_the_reference():
    src = open(os.path.join(ROOT, "include", "alproj_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int alp_normal_equations_batch\(", src, flags=re.S)
    assert m, "alp_normal_equations_batch is not declared"
    assert "src/alproj/optimize.py:215-237" in m.group(1) and ":442-539" in m.group(1)
    from alproj_amd import _lib
    assert "alp_normal_equations_batch" in _lib._SIGNATURES
    assert len(_lib._SIGNATURES["alp_normal_equations_batch"]) == 8
    assert int(re.search(r"#define ALP_ABI_VERSION (\d+)", src).group(1)) == 7


class NoDevice:
    """a Points stand-in whose library must never be reached"""
    n = 10

    class _lib:
        @staticmethod
        def alp_normal_equations_batch(*a):
            raise AssertionError("the library was called")

    _h = None


def test_points_normal_equations_batch_refuses_before_the_library():
    from alproj_amd import _lib
    cand = np.zeros((3, _lib.NPARAM))
    call = lambda *a, **k: _lib.Points.normal_equations_batch(NoDevice(), *a, **k)
    Kx = _lib.PARAM_KEYS.index
    for targets in ([Kx("w")], [Kx("pan"), Kx("h")], [Kx("pan"), Kx("pan")], [], list(range(21)) + [23, 24, 0], [25], [-1]):
        with pytest.raises(ValueError):
            call(cand, targets)
    for f_scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            call(cand, [Kx("pan")], "huber", f_scale)
    with pytest.raises(ValueError):
        call(cand, [Kx("pan")], "arctan", 1.0)
    for bad in (np.zeros(_lib.NPARAM), np.zeros((3, 24)), np.zeros((0, _lib.NPARAM)), np.zeros((1025, _lib.NPARAM)),
                np.zeros((2, 3, _lib.NPARAM))):
        with pytest.raises(ValueError):
            call(bad, [Kx("pan")])
    for good in (cand, np.zeros((1, _lib.NPARAM)), np.zeros((1024, _lib.NPARAM))):
        with pytest.raises(AssertionError):       # a good call does reach the library
            call(good, [Kx("pan")], "cauchy", 2.0)


def optimizer(targets=("pan", "tilt"), case="trf_linear_d7"):
    from alproj_amd import optimize as aopt
    prob = nc.g14_problem(case)
    o = aopt.LsqOptimizer(pd.DataFrame(prob["xyz"], columns=["x", "y", "z"]), pd.DataFrame(prob["uv"], columns=["u", "v"]),
                          dict(prob["init"]))
    o.set_target(list(targets))
    return o, prob


def test_optimize_starts_refuses_before_any_gpu_call(monkeypatch):
    from alproj_amd import optimize as aopt

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(aopt.BaseOptimizer, "_device_points", no_device)
    monkeypatch.setattr(aopt._lib, "lib", no_device)
    good = dict(nc.g14_problem("trf_linear_d7")["init"])
    for starts in (0, -1, 1025, True, 2.5, "four", [], [good, {"pan": 1.0}], [good, 3.0], np.zeros((2, 3)), np.zeros(2),
                   np.zeros((0, 2)), np.zeros((1025, 2)), [[0.0, float("nan")]], [[0.0, float("inf")]]):
        with pytest.raises(ValueError):
            optimizer()[0].optimize(method="normal", starts=starts)
    with pytest.raises(ValueError):               # the integer form draws in the box
        optimizer()[0].optimize(method="normal", starts=4, bound_widths={"pan": np.inf, "tilt": 1.0})
    for method in ("trf", "dogbox", "lm"):
        with pytest.raises(ValueError):
            optimizer()[0].optimize(method=method, starts=4)
    with pytest.raises(ValueError):
        optimizer(["pan", "w"])[0].optimize(method="normal", starts=4)
    with pytest.raises(ValueError):
        optimizer()[0].optimize(method="normal", starts=4, jac="analytic")
    with pytest.raises(ValueError):
        optimizer()[0].optimize(method="normal", starts=4, loss="arctan")
    with pytest.raises(TypeError):
        optimizer()[0].optimize(method="normal", seed=3)
    for starts in (1, 4, 1024, [good], [good, good], np.zeros((3, 2)), [[0.0, 1.0]]):
        with pytest.raises(AssertionError):       # a good call does go on to the device
            optimizer()[0].optimize(method="normal", starts=starts, seed=1)
    # explicit starts need no finite box
    with pytest.raises(AssertionError):
        optimizer()[0].optimize(method="normal", starts=[good], bound_widths={"pan": np.inf, "tilt": np.inf})


def test_the_start_matrix():
    from alproj_amd import optimize as aopt
    prob_targets = ["fov", "pan", "tilt", "roll"]
    o, prob = optimizer(prob_targets)
    b = aopt.bounds_to_array(prob["init"], prob_targets, None)
    lower, upper = b[:, 0], b[:, 1]
    X = o._start_matrix(8, 5, lower, upper)
    assert X.shape == (8, 4) and X.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(X[0], [prob["init"][t] for t in prob_targets])
    np.testing.assert_array_equal(X, o._start_matrix(8, 5, lower, upper))
    np.testing.assert_array_equal(X, nb.integer_starts(X[0], lower, upper, 8, 5))
    assert ((X >= lower) & (X <= upper)).all() and len({tuple(r) for r in X}) == 8
    assert (o._start_matrix(8, 6, lower, upper)[1:] != X[1:]).all()
    a, c = o._start_matrix(8, None, lower, upper), o._start_matrix(8, None, lower, upper)
    assert (a[1:] != c[1:]).all()                                                 # seed=None draws its own entropy
    np.testing.assert_array_equal(a[0], X[0])
    # explicit starts: dicts by key, arrays as they are, both clipped into the box
    far = dict(prob["init"], pan=prob["init"]["pan"] + 1000.0, fov=prob["init"]["fov"] - 1000.0)
    Xd = o._start_matrix([dict(prob["init"]), far], None, lower, upper)
    np.testing.assert_array_equal(Xd[0], X[0])
    assert Xd[1][1] == upper[1] and Xd[1][0] == lower[0] and Xd[1][2] == X[0][2]
    Xa = o._start_matrix(np.array([X[3], X[0] + 1e6]), None, lower, upper)
    np.testing.assert_array_equal(Xa, [X[3], upper])
    inf = np.full(4, np.inf)
    np.testing.assert_array_equal(o._start_matrix([far], None, -inf, inf)[0], [far[t] for t in prob_targets])
