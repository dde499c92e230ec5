"""GPU: the device loop of LsqOptimizer.optimize(method="normal", device_loop=True) (alp_lm_*, csrc/alp_lm.hip).

A device run's trajectory is not the host run's (the plan's sines and cosines and the solve round differently; near convergence
`cost_new < cost` is decided at rounding level; the host lockstep shrinks its batch as starts stop).  What is held instead:
- the state machine inside lm_step_kernel to alproj_amd/optimize.py: _normal_lm_steps on shared sums (alp_lm_step_host), every
  trial point within 1e-10 of the box width (tests/lm_device_cases.py: TRIAL_TOL), status / evaluations / iterations equal;
- the evaluation inside the loop to alp_normal_equations_batch at the same trial points;
- independence of the starts, repeatability and independence of check_every: bit for bit;
- the end result to the oracle's cost, the reference's optimum and the host lockstep: final cost rel 1e-8, x within 1e-6 of the
  default box width.  Where these two come from: on the CPU oracle a relative noise of 1e-13 on G and g -- a pessimistic stand-in
  for another sin / cos rounding in the plan -- moved the final costs of the 48 runs (8 starts of each g14 case) by at most 1.3e-10
  relative and x by at most 3.3e-9 of the width, and changed the evaluation count by up to 20 and the status among 2 / 3 / 4; the
  conditions take about 100 x and 300 x over that.  Evaluations and status are printed, not compared."""
import ctypes
import functools

import numpy as np
import pytest

from tests import lm_device_cases as lc
from tests import normal_batch_cases as nb
from tests import normal_cases as nc
from tests.test_gpu_normal import EINVAL, ESTATE, frames, idx, pole_problem
from tests.test_jacobian_oracle import KEYS, TARGETS

pytestmark = pytest.mark.gpu

I32 = ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


@functools.lru_cache(maxsize=None)
def problem(case):
    return nc.g14_problem(case)


def starts_of(prob, K=8):
    lower, upper = nc.bounds_of(prob, None)
    return nb.integer_starts(np.array([prob["init"][t] for t in prob["targets"]]), lower, upper, K, 1), lower, upper


def points_of(L, prob, n=None, precision="f64"):
    xyz, uv = prob["xyz"][:n], prob["uv"][:n]
    pts = L.Points(xyz, [prob["init"]["x"], prob["init"]["y"], prob["init"]["z"]], precision)
    pts.set_observed(uv)
    return pts


def run_to_the_end(loop, check_every=8):
    pending, rounds = loop.K, 0
    while pending:
        loop.run(check_every)
        pending = loop.wait()
        rounds += check_every
        assert rounds <= 100 * loop.D + 2 * check_every
    return loop.get()


def same_bits(a, b, rows=None):
    for key in ("x", "cost", "grad_norm", "iterations", "evaluations", "status", "trial", "mu", "nu"):
        x, y = (a[key], b[key]) if rows is None else (a[key][rows[0]], b[key][rows[1]])
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=key)


# ---------------------------------------------------------------------------------------------------- 1. the state machine
def device_against_python(L, pts, template, targets, fun, X0, lower, upper, width, what):
    """K Python machines and one K-start handle in lockstep: each round every running start receives the sums at the Python
    machine's trial point (the handle through alp_lm_step_host), and the handle's pending trial points must be the Python ones"""
    K, D = X0.shape
    tri = D * (D + 1) // 2
    from alproj_amd import optimize as aopt
    gens = [aopt._normal_lm_steps(x0, lower, upper, max_nfev=None, **lc.TOLS) for x0 in X0]
    trial = {k: next(g) for k, g in enumerate(gens)}
    results, worst, rounds = [None] * K, 0.0, 0
    # the handle's own loss is linear with f_scale 1: its cost is 0.5 * the sum given, exactly, whatever loss `fun` stands for
    with L.LmDevice(pts, template, targets, lower, upper, X0) as loop:
        while trial:
            rec = loop.get()
            assert sorted(trial) == [k for k in range(K) if rec["status"][k] == lc.RUNNING], (rounds, what)
            rows = np.zeros((K, tri + D + 2))
            for k in sorted(trial):
                worst = max(worst, float(np.max(np.abs(rec["trial"][k] - trial[k]) / width)))
                G, g, cost = fun(trial[k])
                rows[k, :tri + D + 1] = lc.pack(G, g, 2.0 * cost)
                try:
                    trial[k] = gens[k].send((G, g, cost))
                except StopIteration as stop:
                    results[k] = stop.value
                    del trial[k]
            rows[:, -1] = pts.n
            loop.step_host(rows)
            rounds += 1
        rec = loop.get()
    print("%s: %d starts, %d rounds, worst trial deviation %.3g of the width (tol %.3g); status %s, evaluations %s" %
          (what, K, rounds, worst, lc.TRIAL_TOL, [r["status"] for r in results], [r["evaluations"] for r in results]))
    assert worst <= lc.TRIAL_TOL
    for k, r in enumerate(results):
        assert (rec["status"][k], rec["evaluations"][k], rec["iterations"][k]) == (r["status"], r["evaluations"], r["iterations"]), k
        assert (np.abs(rec["x"][k] - r["x"]) <= lc.TRIAL_TOL * width).all()
        if np.isfinite(r["cost"]):
            assert rec["cost"][k] == r["cost"]
        assert rec["grad_norm"][k] == r["grad_norm"] or (np.isnan(r["grad_norm"]) and np.isnan(rec["grad_norm"][k]))
    return results


@pytest.mark.parametrize("case", ["trf_linear_d7", "dogbox_softl1_d4", "trf_linear_dist_d6"])
def test_step_host_against_the_python_machine_on_g14(L, case):
    prob = problem(case)
    kw = nc.LSQ_KW[case]
    fun = nb.remembered(nc.oracle_sums(prob, kw.get("loss", "linear"), kw.get("f_scale", 1.0)))
    X0, lower, upper = starts_of(prob)
    run_lower, run_upper = nc.bounds_of(prob, nc.widths_of(case))
    with points_of(L, prob) as pts:
        res = device_against_python(L, pts, L.params_vector(prob["init"]), idx(prob["targets"]), fun, X0, run_lower, run_upper,
                                    upper - lower, case)
    assert all(r["status"] in (1, 2, 3, 4) for r in res)


@pytest.mark.parametrize("D", [1, 16, 17, 23])
def test_step_host_against_the_python_machine_on_bounded_linear_problems(L, D):
    p = lc.linear_problem(D)
    prob = problem("trf_linear_d7")
    with points_of(L, prob, 64) as pts:          # the points only give the handle something to plan for: no evaluation runs
        res = device_against_python(L, pts, L.params_vector(prob["init"]), idx(TARGETS[:D]), p["fun"], p["starts"], p["lower"],
                                    p["upper"], p["width"], "linear D=%d" % D)
    assert all(r["status"] in (1, 2, 3, 4) for r in res)
    assert min(int(((r["x"] == p["lower"]) | (r["x"] == p["upper"])).sum()) for r in res) >= 1


def test_step_host_edge_cases(L):
    """a start whose first cost is not finite, max_nfev = 1 and 2, every variable on a bound: one handle each, against the
    Python machine"""
    from alproj_amd import optimize as aopt
    p = lc.linear_problem(2)
    prob = problem("trf_linear_d7")
    tmpl, targets = L.params_vector(prob["init"]), idx(TARGETS[:2])
    with points_of(L, prob, 64) as pts:
        rows = np.zeros((4, 2 * 3 // 2 + 2 + 2))
        for k, x0 in enumerate(p["starts"]):
            G, g, cost = p["fun"](np.clip(x0, p["lower"], p["upper"]))
            rows[k, :-1] = lc.pack(G, g, 2.0 * cost)
        rows[1, -2] = np.nan
        rows[2, 3] = np.inf                       # in g
        with L.LmDevice(pts, tmpl, targets, p["lower"], p["upper"], p["starts"]) as loop:
            loop.step_host(rows)
            rec = loop.get()
        assert list(rec["status"]) == [lc.RUNNING, -1, -1, lc.RUNNING] and list(rec["evaluations"]) == [1, 1, 1, 1]
        assert np.isnan(rec["cost"][1]) and np.isnan(rec["grad_norm"][1]) and np.isnan(rec["grad_norm"][2])
        np.testing.assert_array_equal(rec["x"], np.clip(p["starts"], p["lower"], p["upper"]))
        for max_nfev in (1, 2):
            ref = [aopt.normal_lm(p["fun"], x0, p["lower"], p["upper"], max_nfev=max_nfev) for x0 in p["starts"]]
            with L.LmDevice(pts, tmpl, targets, p["lower"], p["upper"], p["starts"], max_nfev=max_nfev) as loop:
                for _ in range(max_nfev):
                    rec = loop.get()
                    for k in range(4):
                        G, g, cost = p["fun"](rec["trial"][k])
                        rows[k, :-1] = lc.pack(G, g, 2.0 * cost)
                    loop.step_host(rows)
                rec = loop.get()
            assert list(rec["status"]) == [r["status"] for r in ref] == [0] * 4
            assert list(rec["evaluations"]) == [max_nfev] * 4
            for k in range(4):
                assert (np.abs(rec["x"][k] - ref[k]["x"]) <= lc.TRIAL_TOL * p["width"]).all() and rec["cost"][k] == ref[k]["cost"]
        # every variable on a bound it is pushed against: status 1 at the first evaluation
        c, w = np.array([-3.0, -4.0]), np.array([1.0, 9.0])
        lower, upper = np.full(2, 5.0), np.full(2, 6.0)
        r = lower - c
        one = np.zeros((1, 7))
        one[0, :-1] = lc.pack(np.diag(w), w * r, float(r @ (w * r)))
        with L.LmDevice(pts, tmpl, targets, lower, upper, np.zeros((1, 2))) as loop:
            loop.step_host(one)
            rec = loop.get()
        assert rec["status"][0] == 1 and rec["evaluations"][0] == 1 and rec["grad_norm"][0] == 0.0 and (rec["x"][0] == lower).all()


# ---------------------------------------------------------------------------------------------------- 2. the evaluation in the loop
@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("n", [None, 257, 64])
def test_the_evaluation_inside_the_loop_is_the_batch_call(L, K, n):
    """two identical handles: one runs a round, the other is stepped on alp_normal_equations_batch's sums at the same trial
    points (the host-built plan differs from the device-built one by the device's sin / cos / tan alone).  Three rounds."""
    prob = problem("trf_linear_d7")
    X0, lower, upper = starts_of(prob, K)
    targets = idx(prob["targets"])
    tp = np.array(targets, dtype=np.int32)
    D = len(targets)
    tmpl = L.params_vector(prob["init"])
    with points_of(L, prob, n) as pts:
        assert n is None or pts.n == n
        if n is None:
            assert nb.normal_batch_grid(pts.n, K, 256)[0] >= 2           # more than one stripe per start
        with L.LmDevice(pts, tmpl, targets, lower, upper, X0) as a, L.LmDevice(pts, tmpl, targets, lower, upper, X0) as b:
            for rnd in range(3):
                trial = b.get()["trial"]
                cand = np.tile(tmpl, (K, 1))
                cand[:, targets] = trial
                raw = np.empty((K, D * (D + 1) // 2 + D + 2))
                assert L.lib().alp_normal_equations_batch(pts._h, L.as_dp(cand), K, tp.ctypes.data_as(I32), D, 0, 1.0, L.as_dp(raw)) == 0
                a.run(1)
                a.wait()
                b.step_host(raw)
                ra, rb = a.get(), b.get()
                dev = float(np.max(np.abs(ra["trial"] - rb["trial"]) / (upper - lower)))
                rel = lambda u, v: float(np.max(np.abs(u - v) / np.abs(v)))
                print("round %d: trial deviation %.3g of the width, cost rel %.3g, mu rel %.3g" %
                      (rnd, dev, rel(ra["cost"], rb["cost"]), rel(ra["mu"], rb["mu"])))
                assert dev <= lc.TRIAL_TOL and rel(ra["cost"], rb["cost"]) <= lc.TRIAL_TOL and rel(ra["mu"], rb["mu"]) <= lc.TRIAL_TOL
                np.testing.assert_array_equal(ra["status"], rb["status"])
                np.testing.assert_array_equal(ra["evaluations"], rb["evaluations"])
                assert (ra["evaluations"] == rnd + 1).all()


# ---------------------------------------------------------------------------------------------------- 3. independence
@functools.lru_cache(maxsize=None)
def d7_records(variant, check_every=8):
    """the records of K = 8 runs on trf_linear_d7: "given" = the eight starts, "copies" = start 3 among seven copies of start 0"""
    from alproj_amd import _lib as L
    prob = problem("trf_linear_d7")
    X0, lower, upper = starts_of(prob)
    if variant == "copies":
        X0 = np.array([X0[3] if k == 3 else X0[0] for k in range(8)])
    with points_of(L, prob) as pts:
        with L.LmDevice(pts, L.params_vector(prob["init"]), idx(prob["targets"]), lower, upper, X0) as loop:
            return run_to_the_end(loop, check_every)


def test_a_start_does_not_depend_on_the_others(L):
    given, copies = d7_records("given"), d7_records("copies")
    assert (given["status"] != lc.RUNNING).all() and len(set(given["cost"].tolist())) > 1
    same_bits(given, copies, rows=(3, 3))
    same_bits(given, copies, rows=(0, 0))
    same_bits(copies, copies, rows=(0, 7))


def test_a_run_repeated_and_any_check_every_give_the_same_bits(L):
    given = d7_records("given")
    d7_records.cache_clear()
    same_bits(given, d7_records("given"))
    for check_every in (1, 3, 1000):
        same_bits(given, d7_records("given", check_every))


# ---------------------------------------------------------------------------------------------------- 4. end to end
def lsq(prob):
    from alproj_amd import optimize as aopt
    o = aopt.LsqOptimizer(*frames(prob), dict(prob["init"]))
    o.set_target(prob["targets"])
    return o


@pytest.mark.parametrize("case", list(nc.LSQ_KW))
def test_optimize_device_loop_with_eight_starts(L, case):
    from alproj_amd import optimize as aopt
    prob = problem(case)
    kw = nc.LSQ_KW[case]
    loss, f_scale = kw.get("loss", "linear"), kw.get("f_scale", 1.0)
    lower, upper = nc.bounds_of(prob, None)
    if kw.get("unbounded"):
        starts = nb.integer_starts(np.array([prob["init"][t] for t in prob["targets"]]), lower, upper, 8, 1)
    else:
        starts = 8
    call = dict(method="normal", bound_widths=nc.widths_of(case), loss=loss, f_scale=f_scale, starts=starts, seed=1)
    o = lsq(prob)
    params, err = o.optimize(device_loop=True, **call)
    host = lsq(prob)
    host.optimize(device_loop=False, **call)
    D = len(prob["targets"])
    assert len(o.start_results) == 8
    print(case, "device (status, evaluations):", [(r[2]["status"], r[2]["evaluations"]) for r in o.start_results])
    print(case, "host   (status, evaluations):", [(r[2]["status"], r[2]["evaluations"]) for r in host.start_results])
    for (p, e, res), (hp, he, hres) in zip(o.start_results, host.start_results):
        assert set(p) == set(prob["want"]) and set(res) == {"cost", "iterations", "evaluations", "status", "grad_norm"}
        assert 1 <= res["evaluations"] <= 100 * D
        if np.isfinite(res["cost"]):
            assert res["cost"] == pytest.approx(nc.cost_at(prob, p, loss, f_scale), rel=1e-9)
            assert e == pytest.approx(nc.mean_distance(prob, p), rel=1e-9)
        dx = max(abs(p[t] - hp[t]) / w for t, w in zip(prob["targets"], upper - lower))
        print("   cost %.15g (host %.15g, rel %.3g), x within %.3g of the width" % (res["cost"], hres["cost"], res["cost"] / hres["cost"] - 1, dx))
        assert res["cost"] == pytest.approx(hres["cost"], rel=1e-8)
        assert dx <= 1e-6
    p0, e0, r0 = o.start_results[0]
    assert r0["status"] in (1, 2, 3, 4)
    nc.assert_reference_optimum(prob, p0, e0, r0["cost"], loss, f_scale)
    b = aopt.best_start([r[2]["cost"] for r in o.start_results])
    assert o.result_ == dict(o.start_results[b][2], start=b)
    assert (params, err) == o.start_results[b][:2]


def test_optimize_device_loop_without_starts_is_the_single_run(L):
    prob = problem("trf_linear_d7")
    o = lsq(prob)
    params, err = o.optimize(method="normal", device_loop=True)
    print(o.result_)
    assert set(o.result_) == {"cost", "iterations", "evaluations", "status", "grad_norm"} and o.result_["status"] in (1, 2, 3, 4)
    nc.assert_reference_optimum(prob, params, err, o.result_["cost"], "linear", 1.0)


def test_optimize_device_loop_on_a_float32_set(L):
    from alproj_amd import optimize as aopt
    prob = problem("trf_linear_d7")
    o = lsq(prob)
    params, err = o.optimize(method="normal", precision="f32", starts=8, seed=1, device_loop=True)
    print("f32", o.result_)
    assert o.result_["status"] in (1, 2, 3, 4) and len(o.start_results) == 8 and np.isfinite(err)
    assert o.result_["start"] == aopt.best_start([r[2]["cost"] for r in o.start_results])


def test_world_1_communicator_gives_the_same_bits(L):
    before = d7_records("given")
    d7_records.cache_clear()
    L.comm_init(L.comm_unique_id(), 0, 1)
    try:
        assert L.comm_info() == (0, 1)
        during = d7_records("given")
    finally:
        L.comm_destroy()
    d7_records.cache_clear()
    same_bits(before, during)
    same_bits(before, d7_records("given"))


# ---------------------------------------------------------------------------------------------------- 5. errors, empty set, a pole
def test_error_paths(L):
    prob = problem("trf_linear_d7")
    lib = L.lib()
    tmpl = L.params_vector(prob["init"])
    lo, hi = np.full(25, -1.0), np.full(25, 1.0)
    X0 = np.zeros((1025, 25))
    good = np.array(idx(["pan", "tilt"]), dtype=np.int32)

    def create(pts, targets, D, K, loss=0, f_scale=1.0, max_nfev=200):
        h = ctypes.c_void_p()
        rc = lib.alp_lm_create(pts._h, L.as_dp(tmpl), targets.ctypes.data_as(I32), D, L.as_dp(lo), L.as_dp(hi), L.as_dp(X0), K, loss, f_scale,
                               1e-10, 1e-10, 1e-10, max_nfev, ctypes.byref(h))
        assert (rc == 0) == bool(h)
        if h:
            lib.alp_lm_destroy(h)
        return rc

    xyz, uv = prob["xyz"][:64], prob["uv"][:64]
    with L.Points(xyz, [0.0, 0.0, 0.0], "f64") as pts:
        assert create(pts, good, 2, 3) == ESTATE                  # no observed uv yet
        pts.set_observed(uv)
        assert create(pts, good, 2, 3) == 0 and create(pts, good, 2, 1) == 0 and create(pts, good, 2, 1024) == 0
        for K in (0, 1025, -1):
            assert create(pts, good, 2, K) == EINVAL, K
        many = np.arange(25, dtype=np.int32)
        for D in (0, 24, -1):
            assert create(pts, many, D, 3) == EINVAL, D
        for bad in ([21], [KEYS.index("pan"), 22], [4, 4], [25], [-1]):
            assert create(pts, np.array(bad, dtype=np.int32), len(bad), 3) == EINVAL, bad
        assert create(pts, good, 2, 3, loss=4) == EINVAL and create(pts, good, 2, 3, f_scale=0.0) == EINVAL
        assert create(pts, good, 2, 3, max_nfev=0) == EINVAL
        with L.LmDevice(pts, tmpl, good, lo[:2], hi[:2], X0[:3, :2]) as loop:
            assert lib.alp_lm_wait(loop._h, None) == ESTATE       # nothing enqueued
            assert lib.alp_lm_run(loop._h, 1) == 0
            assert lib.alp_lm_run(loop._h, 1) == ESTATE           # a second run before the wait
            assert lib.alp_lm_get(loop._h, *([None] * 9)) == ESTATE and lib.alp_lm_step_host(loop._h, L.as_dp(np.zeros((3, 7)))) == ESTATE
            assert loop.wait() in (0, 1, 2, 3)
            assert lib.alp_lm_get(loop._h, *([None] * 9)) == 0
            assert lib.alp_lm_run(loop._h, -1) == EINVAL and lib.alp_lm_step_host(loop._h, None) == EINVAL
        assert lib.alp_lm_run(None, 1) == EINVAL and lib.alp_lm_destroy(None) == 0


def test_an_empty_point_set_ends_every_start_at_the_first_evaluation(L):
    prob = problem("trf_linear_d7")
    X0, lower, upper = starts_of(prob, 3)
    with L.Points(np.zeros((0, 3)), [0, 0, 0], "f64") as pts:
        pts.set_observed(np.zeros((0, 2)))
        with L.LmDevice(pts, L.params_vector(prob["init"]), idx(prob["targets"]), lower, upper, X0) as loop:
            loop.run(2)
            assert loop.wait() == 0
            rec = loop.get()
    assert list(rec["status"]) == [1, 1, 1] and list(rec["evaluations"]) == [1, 1, 1] and not rec["cost"].any()
    np.testing.assert_array_equal(rec["x"], X0)


def device_pole_a2(L, xyz, uv, truth, i, a2_pole, targets, centre):
    """the a2 at which vertex i sits on the lens pole under the plan the DEVICE folds (pole_problem finds it under the host's
    fold; the device's sin / cos may move r2 by a few ulps): 1 + a2 stepped ulp by ulp outward from pole_problem's, 1024
    candidates per handle on the one-vertex set, the first whose start ends with status -1"""
    t0 = np.array([1.0 + a2_pole])
    assert t0[0] - 1.0 == a2_pole
    steps = np.arange(-4096, 4097)
    steps = steps[np.argsort(np.abs(steps), kind="stable")]
    a2 = (t0.view(np.int64)[0] + steps).view(np.float64) - 1.0
    inf = np.full(4, np.inf)
    with L.Points(xyz[i:i + 1], [truth["x"], truth["y"], truth["z"]], "f64") as one:
        one.set_observed(uv[i:i + 1])
        for c0 in range(0, len(a2), 1024):
            X0 = np.tile(centre, (len(a2[c0:c0 + 1024]), 1))
            X0[:, 1] = a2[c0:c0 + 1024]
            with L.LmDevice(one, L.params_vector(truth), targets, -inf, inf, X0) as loop:
                loop.run(1)
                loop.wait()
                hit = np.flatnonzero(loop.get()["status"] == -1)
            if len(hit):
                print("the device's pole: %d ulp(s) from the host fold's" % steps[c0 + hit[0]])
                return float(X0[hit[0], 1])
    raise AssertionError("no candidate landed on the device's pole")


def test_a_start_with_a_pole_ends_alone(L):
    xyz, uv, truth, i, a2_pole = pole_problem(L)
    names = ["pan", "a2", "k1", "cx"]
    targets = idx(names)
    centre = np.array([truth[t] for t in names])
    inf = np.full(4, np.inf)
    clean = np.array([centre + [0.01 * k, 0.0, 0.0, 0.0] for k in range(4)])
    with_pole = clean.copy()
    with_pole[2] = centre
    with_pole[2, 1] = device_pole_a2(L, xyz, uv, truth, i, a2_pole, targets, centre)
    recs = []
    with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], "f64") as pts:
        pts.set_observed(uv)
        for X0 in (clean, with_pole):
            with L.LmDevice(pts, L.params_vector(truth), targets, -inf, inf, X0) as loop:
                recs.append(run_to_the_end(loop))
    without, got = recs
    assert got["status"][2] == -1 and got["evaluations"][2] == 1 and not np.isfinite(got["cost"][2])
    assert (without["status"] != -1).all() and (without["status"] != lc.RUNNING).all()
    for k in (0, 1, 3):
        same_bits(without, got, rows=(k, k))
