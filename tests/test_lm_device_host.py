"""CPU: the Levenberg-Marquardt state machine of the least-squares device loop (alproj_amd/csrc/host/alp_lm.h, the code
lm_step_kernel runs) against its specification, alproj_amd/optimize.py: _normal_lm_steps, in lockstep on shared sums; and the
refusals and the interface of LsqOptimizer.optimize(method="normal", device_loop=True).

The C++ is reached through the self-checking driver of the HIP-free host code (csrc/host/alp_host_selfcheck.cpp --lm), built
without HIP by the library's own clang++.  Each round both machines receive the sums evaluated at the Python machine's trial
point; every trial point must agree within 1e-10 of the box width per coordinate (tests/lm_device_cases.py: TRIAL_TOL, and where
it comes from), status, evaluations and iterations must be equal."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from alproj_amd import _build
from tests import lm_device_cases as lc
from tests import normal_batch_cases as nb
from tests import normal_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    return _build.build_host("plain", "clang")


def compare(exe, fun, x0, lower, upper, width, what, **kw):
    ref_trials, rows, ref = lc.lockstep(fun, x0, lower, upper, **kw)
    trials, rec = lc.driver(exe, x0, lower, upper, rows, **kw)
    assert rec["stopped"]
    lc.assert_same_run(trials, rec, ref_trials, ref, width, what)
    return ref


# ---------------------------------------------------------------------------------------------------- the g14 runs
@pytest.mark.parametrize("case", list(nc.LSQ_KW))
def test_state_machine_on_the_g14_runs(exe, case):
    prob = nc.g14_problem(case)
    kw = nc.LSQ_KW[case]
    fun = nb.remembered(nc.oracle_sums(prob, kw.get("loss", "linear"), kw.get("f_scale", 1.0)))
    lower, upper = nc.bounds_of(prob, None)
    starts = nb.integer_starts(np.array([prob["init"][t] for t in prob["targets"]]), lower, upper, 8, 1)
    run_lower, run_upper = nc.bounds_of(prob, nc.widths_of(case))          # the run's own box (infinite for the lm case)
    statuses = []
    for k, x0 in enumerate(starts):
        ref = compare(exe, fun, x0, run_lower, run_upper, upper - lower, "%s start %d" % (case, k))
        statuses.append(ref["status"])
    assert all(s in (1, 2, 3, 4) for s in statuses), statuses


# ---------------------------------------------------------------------------------------------------- bounded linear problems
@pytest.mark.parametrize("D", lc.LINEAR_D)
def test_state_machine_on_bounded_linear_problems(exe, D):
    p = lc.linear_problem(D)
    on_bound = []
    for k, x0 in enumerate(p["starts"]):
        ref = compare(exe, p["fun"], x0, p["lower"], p["upper"], p["width"], "linear D=%d start %d" % (D, k))
        assert ref["status"] in (1, 2, 3, 4)
        on_bound.append(int(((ref["x"] == p["lower"]) | (ref["x"] == p["upper"])).sum()))
    print("D = %d: variables on a bound at the optimum: %s" % (D, on_bound))
    assert min(on_bound) >= 1


# ---------------------------------------------------------------------------------------------------- edge cases
def test_a_start_whose_first_cost_is_not_finite(exe):
    p = lc.linear_problem(2)
    for bad in (float("nan"), float("inf")):
        def fun(x, bad=bad):
            G, g, _ = p["fun"](x)
            return G, g, bad
        ref = compare(exe, fun, p["starts"][0], p["lower"], p["upper"], p["width"], "cost %r at x0" % bad)
        assert ref["status"] == -1 and ref["evaluations"] == 1

    def nan_in_g(x):
        G, g, c = p["fun"](x)
        return G, np.where(np.arange(2) == 1, np.nan, g), c
    assert compare(exe, nan_in_g, p["starts"][0], p["lower"], p["upper"], p["width"], "NaN in g at x0")["status"] == -1


def test_a_trial_that_is_not_finite_is_rejected_and_the_damping_raised(exe):
    p = lc.linear_problem(16)
    calls = []

    def fun(x):
        calls.append(1)
        G, g, c = p["fun"](x)
        if len(calls) in (2, 3):                   # the first two trial points come back unusable
            return G, g, float("nan") if len(calls) == 2 else float("inf")
        return G, g, c
    ref_trials, rows, ref = lc.lockstep(fun, p["starts"][1], p["lower"], p["upper"])
    trials, rec = lc.driver(exe, p["starts"][1], p["lower"], p["upper"], rows)
    lc.assert_same_run(trials, rec, ref_trials, ref, p["width"], "non-finite trials")
    assert ref["status"] in (1, 2, 3, 4) and ref["evaluations"] >= 4 and ref["iterations"] <= ref["evaluations"] - 3
    # the damping after the two rejections: mu_0 * 2 * 4, read off the machine that was starved after them
    _, early = lc.driver(exe, p["starts"][1], p["lower"], p["upper"], rows[:3])
    assert not early["stopped"] and early["status"] == lc.RUNNING and early["evaluations"] == 3 and early["iterations"] == 0
    assert early["mu"] == 1e-3 * float(np.max(np.diag(p["G"]))) * 2.0 * 4.0 and early["nu"] == 8.0


@pytest.mark.parametrize("max_nfev", [1, 2])
def test_max_nfev(exe, max_nfev):
    p = lc.linear_problem(17)
    ref = compare(exe, p["fun"], p["starts"][2], p["lower"], p["upper"], p["width"], "max_nfev %d" % max_nfev, max_nfev=max_nfev)
    assert ref["status"] == 0 and ref["evaluations"] == max_nfev


def test_all_variables_on_bounds_stops_at_once(exe):
    # cost = 0.5 |diag(1, 3) (x - c)|^2 with c far below the box: x0 clipped lies in the lower corner, and both gradient
    # components push outward there
    c, w = np.array([-3.0, -4.0]), np.array([1.0, 9.0])

    def fun(x):
        r = np.asarray(x, dtype=np.float64) - c
        return np.diag(w), w * r, 0.5 * float(r @ (w * r))
    lower, upper = np.full(2, 5.0), np.full(2, 6.0)
    ref = compare(exe, fun, np.zeros(2), lower, upper, upper - lower, "all on bounds")
    assert ref["status"] == 1 and ref["evaluations"] == 1 and (ref["x"] == lower).all() and ref["grad_norm"] == 0.0


# ---------------------------------------------------------------------------------------------------- start counts and stop patterns
def test_stop_sets_fit_their_start_count_and_reach_every_seam():
    """the case helpers of tests/test_gpu_lm_device_starts.py"""
    assert lc.SEAM_K == (1, 63, 64, 65, 255, 256, 257, 513, 1024) and nb.BATCH_MAX == 1024
    for K in lc.SEAM_K:
        sets = lc.stop_sets(K)
        assert list(sets)[:2] == ["none", "all"] and len(sets["none"]) == 0 and np.array_equal(sets["all"], np.arange(K))
        assert len({s.tobytes() for s in sets.values()}) == len(sets)              # no pattern twice
        for name, s in sets.items():
            assert s.dtype == np.int64 and np.array_equal(s, np.unique(s)) and (len(s) == 0 or (0 <= s[0] and s[-1] < K)), (K, name)
        assert lc.seam_slots(K) == sorted({j for j in (0, 63, 64, 65, 255, 256, 257, K - 1) if j < K})
        for j in lc.seam_slots(K):
            if K > 1:
                assert np.array_equal(sets["only %d" % j], [j])
                assert np.array_equal(np.setdiff1d(np.arange(K), sets["all but %d" % j]), [j])
        print("K = %4d: %2d stop sets" % (K, len(sets)))
    assert list(lc.stop_sets(1)) == ["none", "all"]
    sets = lc.stop_sets(1024)
    assert len(sets) == 2 + 2 * 8 + 7
    assert np.array_equal(sets["even"], np.arange(0, 1024, 2)) and np.array_equal(sets["odd"], np.arange(1, 1024, 2))
    assert np.array_equal(sets["first wave"], np.arange(64)) and np.array_equal(sets["first pass"], np.arange(256))
    assert np.array_equal(sets["all but the last wave"], np.arange(960))
    assert np.array_equal(lc.stop_sets(255)["all but the last wave"], np.arange(192))
    for K, name in ((65, "all but 64"), (257, "all but 256"), (513, "all but 512")):          # the same set under its first name
        assert "all but the last wave" not in lc.stop_sets(K) and np.array_equal(lc.stop_sets(K)[name], np.arange(K - 1))
    half = sets["random half"]
    assert len(half) == 512 and 0 < (half % 2).sum() < 512 and all(0 < ((half // 64) == w).sum() < 64 for w in range(16))
    for K in lc.SEAM_K:
        assert len(lc.random_half(K)) == K // 2


def test_the_sparse_survivors_leave_waves_and_a_whole_pass_empty():
    keep = lc.sparse_survivors(1024)
    assert np.array_equal(np.setdiff1d(np.arange(1024), lc.stop_sets(1024)["all but sparse survivors"]), keep)
    per_pass = np.bincount(keep // lc.PASS, minlength=4)
    per_wave = np.bincount(keep // lc.WAVE, minlength=16)
    print("sparse survivors", keep.tolist(), "per pass", per_pass.tolist(), "per wave", per_wave.tolist())
    assert 8 <= len(keep) <= 32
    assert per_pass[2] == 0 and per_pass[:2].all() and per_pass[3] > 0     # a pass with no running start, survivors on both sides
    assert per_wave[3] == 0 and per_wave[:3].all() and per_wave[4] > 0     # the same for a wave inside the first pass
    assert np.diff(keep).max() > lc.PASS                                   # one survivor after a long gap
    for K in lc.SEAM_K:                                                    # the same draw at every start count
        assert np.array_equal(lc.sparse_survivors(K), keep[keep < K])
    assert len(lc.sparse_survivors(513)) > len(lc.sparse_survivors(257)) > 0


def test_the_subset_of_48_slots_sits_on_the_seams():
    slots = lc.subset_slots()
    assert len(slots) == 48 == len(set(slots.tolist())) and np.array_equal(slots, np.sort(slots)) and slots[0] == 0 and slots[-1] == 1023
    for block in (range(0, 8), range(60, 68), range(252, 260), range(508, 516), range(1016, 1024)):
        assert set(block) <= set(slots.tolist())


def test_the_starts_are_distinct_and_prefix_stable_and_the_table_rows_distinct():
    from alproj_amd import resample
    prob = nc.g14_problem("trf_linear_d7")
    lower, upper = nc.bounds_of(prob, None)
    x_init = np.array([prob["init"][t] for t in prob["targets"]])
    assert len(prob["xyz"]) == 400 and len(x_init) == 7
    big = nb.integer_starts(x_init, lower, upper, 1024, 1)
    assert len({row.tobytes() for row in big}) == 1024
    assert ((big >= lower) & (big <= upper)).all()
    for K in lc.SEAM_K:
        assert np.array_equal(nb.integer_starts(x_init, lower, upper, K, 1), big[:K])
    assert np.array_equal(nb.integer_starts(x_init, lower, upper, 8, 1), big[:8])
    for n in (64, 400):
        table = resample.bootstrap_table(n, 257, lc.TABLE_SEED)
        assert table.shape == (257, n) and (table == np.floor(table)).all() and (table.sum(axis=1) == n).all()
        assert len({row.tobytes() for row in table}) == 257


# ---------------------------------------------------------------------------------------------------- interface and refusals
def test_the_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "alproj_hip.h")).read()
    from alproj_amd import _lib
    for name in ("alp_lm_create", "alp_lm_run", "alp_lm_wait", "alp_lm_get", "alp_lm_step_host", "alp_lm_destroy"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _lib._SIGNATURES
    assert re.search(r"#define ALP_ABI_VERSION 7\b", text)
    assert re.search(r"#define ALP_LM_RUNNING \(-2\)", text) and _lib.LM_RUNNING == lc.RUNNING == -2


def optimizer(targets=("pan", "tilt"), case="trf_linear_d7"):
    from alproj_amd import optimize as aopt
    prob = nc.g14_problem(case)
    o = aopt.LsqOptimizer(pd.DataFrame(prob["xyz"], columns=["x", "y", "z"]), pd.DataFrame(prob["uv"], columns=["u", "v"]),
                          dict(prob["init"]))
    o.set_target(list(targets))
    return o, prob


def test_device_loop_refuses_before_any_gpu_call(monkeypatch):
    from alproj_amd import _lib
    from alproj_amd import optimize as aopt

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(aopt.BaseOptimizer, "_device_points", no_device)
    monkeypatch.setattr(aopt._lib, "lib", no_device)
    for method in ("trf", "dogbox", "lm"):
        with pytest.raises(ValueError):
            optimizer()[0].optimize(method=method, device_loop=True)
    for check_every in (0, -1, 2.5, "8", None, True):
        with pytest.raises(ValueError):
            optimizer()[0].optimize(method="normal", starts=4, seed=1, device_loop=True, check_every=check_every)
    with pytest.raises(ValueError):
        optimizer(["pan", "w"])[0].optimize(method="normal", device_loop=True)
    with pytest.raises(ValueError):
        optimizer(["pan", "h"])[0].optimize(method="normal", starts=2, seed=1, device_loop=True)
    with pytest.raises(ValueError):                # 24 targets: one more than alp_normal_equations takes
        optimizer([k for k in _lib.PARAM_KEYS if k != "w"])[0].optimize(method="normal", device_loop=True)
    with pytest.raises(ValueError):
        optimizer()[0].optimize(method="normal", starts=0, device_loop=True)
    for kw in (dict(), dict(starts=1), dict(starts=8, seed=1), dict(starts=8, seed=1, check_every=1), dict(check_every=np.int64(3))):
        with pytest.raises(AssertionError):        # a good call does go on to the device
            optimizer()[0].optimize(method="normal", device_loop=True, **kw)
