"""GPU: the least-squares device loop (alp_lm_*, csrc/alp_lm.hip) at every start count and stop pattern.

tests/test_gpu_lm_device.py holds the loop to the Python machine, the oracle's sums and the host lockstep with at most 8 starts:
one wave and one pass of lm_select_kernel, a list that is the identity or nearly so.  Here the same loop runs with up to 1024
starts, and the list loses whole waves and passes.

A start's record (x, cost, grad_norm, iterations, evaluations, status, trial, mu, nu) depends on its X0 (and its weight row
under table rows), the sums fed to it and the launch grid normal_batch_grid(n, K, cus) alone.  So the reference of a handle
is ANOTHER HANDLE WITH THE SAME GRID in which the mechanism under test is idle (no start stopped: list = 0 .. K-1) or small
(K <= 48: one wave), and the comparison is bit for bit (test_gpu_lm_device.same_bits).  Every test computes both grids from the
device's CU count and asserts that they are equal before it compares.

Starts are stopped by force with the edge case of test_step_host_edge_cases: the first evaluation is fed through
alp_lm_step_host, alp_normal_equations_batch's sums at X0 with a NaN in the cost of the starts to stop, which end with status
-1 at once.  Three device rounds follow: in the first a start that the list lost would read whatever the buffer of partial
sums held, from the second on its own stale row.

Problem: g14 trf_linear_d7 (400 points, D = 7); 64 points = one group and one stripe on any device, 400 = two groups, two
stripes for every K <= 1024 on 256 CUs.  Start counts, stop sets and seam slots: tests/lm_device_cases.py."""
import ctypes

import numpy as np
import pytest

from tests import lm_device_cases as lc
from tests import normal_batch_cases as nb
from tests import test_gpu_lm_device as t_lm
from tests.test_gpu_normal import idx

pytestmark = pytest.mark.gpu

I32 = ctypes.POINTER(ctypes.c_int32)
CASE = "trf_linear_d7"
ROUNDS = 3


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def grid_of(L, n, K):
    return nb.normal_batch_grid(n, K, L.device_info()["cu_count"])


def batch_sums(L, pts, tmpl, targets, X, rows=None):
    """alp_normal_equations_batch's rows of sums at the target values X (K, D); ``rows``: alp_normal_equations_batch_rows'
    under these rows of the set's weight table"""
    K, D = X.shape
    tp = np.array(targets, dtype=np.int32)
    cand = np.tile(tmpl, (K, 1))
    cand[:, targets] = X
    raw = np.empty((K, D * (D + 1) // 2 + D + 2))
    if rows is None:
        rc = L.lib().alp_normal_equations_batch(pts._h, L.as_dp(cand), K, tp.ctypes.data_as(I32), D, 0, 1.0, L.as_dp(raw))
    else:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        rc = L.lib().alp_normal_equations_batch_rows(pts._h, L.as_dp(cand), K, rows.ctypes.data_as(I32), tp.ctypes.data_as(I32), D, 0,
                                                     1.0, L.as_dp(raw))
    assert rc == 0
    return raw


def stepped(loop, raw, stop):
    """the first evaluation through alp_lm_step_host -- `raw` with a NaN cost for the starts `stop` -- then ROUNDS device
    rounds -> ([the record after the step and after every round], [wait() of every round])"""
    rows = raw.copy()
    rows[stop, -2] = np.nan
    loop.step_host(rows)
    recs, waits = [loop.get()], []
    for _ in range(ROUNDS):
        loop.run(1)
        waits.append(loop.wait())
        recs.append(loop.get())
    return recs, waits


def same(a, b, rows, what):
    try:
        t_lm.same_bits(a, b, rows=rows)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None


def check_pattern(what, X0, stop, recs, waits, ref):
    """`recs` / `waits` of a handle whose starts `stop` were stopped against `ref`, the records of the handle with no stop"""
    K = len(X0)
    go = np.setdiff1d(np.arange(K), stop)
    assert len(recs) == len(ref) == ROUNDS + 1
    for r, (rec, want) in enumerate(zip(recs, ref)):
        at = "%s, %s" % (what, "after the step" if r == 0 else "round %d" % r)
        same(rec, want, (go, go), at + ", a running start against the handle with no stop")
        assert (rec["status"][stop] == -1).all() and (rec["evaluations"][stop] == 1).all(), at
        assert np.array_equal(rec["x"][stop], X0[stop]), at
        same(rec, recs[0], (stop, stop), at + ", a stopped start against itself after the step")
        if r:
            assert waits[r - 1] == int((rec["status"] == lc.RUNNING).sum()), (at, waits[r - 1])
    if len(stop) == K:
        assert waits == [0] * ROUNDS, what


def forced_stops(L, K, n, precision="f64", names=None):
    """section 1 of the module's docstring for one start count and point set: every stop set of lc.stop_sets(K) (or `names`)"""
    prob = t_lm.problem(CASE)
    X0, lower, upper = t_lm.starts_of(prob, K)
    targets = idx(prob["targets"])
    tmpl = L.params_vector(prob["init"])
    sets = lc.stop_sets(K)
    with t_lm.points_of(L, prob, n, precision) as pts:
        assert n is None or pts.n == n
        points = pts.n
        make = lambda starts: L.LmDevice(pts, tmpl, targets, lower, upper, starts)
        raw = batch_sums(L, pts, tmpl, targets, X0)
        with make(X0) as loop:
            ref, ref_waits = stepped(loop, raw, sets["none"])
        # the reference is worth something: K starts, K problems, nobody stopped by force; and its first starts are the
        # handle of at most 8 starts that tests/test_gpu_lm_device.py holds to the Python machine and the oracle
        assert len(set(ref[-1]["cost"].tolist())) == K and (ref[-1]["status"] != -1).all() and ref[-1]["evaluations"].max() == ROUNDS + 1
        check_pattern("K = %d, none" % K, X0, sets["none"], ref, ref_waits, ref)
        few = min(K, 8)
        if grid_of(L, pts.n, few) == grid_of(L, pts.n, K):
            with make(X0[:few]) as loop:
                small, _ = stepped(loop, raw[:few], sets["none"])
            for r in range(ROUNDS + 1):
                same(ref[r], small[r], (np.arange(few), np.arange(few)), "K = %d against K = %d, round %d" % (K, few, r))
        else:
            print("K = %d against K = %d: another grid on this device, not compared" % (K, few))
        for name in (names or [s for s in sets if s != "none"]):
            stop = sets[name]
            with make(X0) as loop:                           # the same K on the same set: the same grid
                recs, waits = stepped(loop, raw, stop)
            check_pattern("K = %d, %s" % (K, name), X0, stop, recs, waits, ref)
    print("K = %d, n = %d, %s: %d stop sets, %d starts still run in the handle with no stop" %
          (K, points, precision, len(names or sets), ref_waits[-1]))


# ---------------------------------------------------------------------------------------------------- 1. forced stop patterns
@pytest.mark.parametrize("n", [64, None])
@pytest.mark.parametrize("K", lc.SEAM_K)
def test_forced_stop_patterns_at_every_seam(L, K, n):
    forced_stops(L, K, n)


def test_forced_stops_on_a_float32_set(L):
    forced_stops(L, 257, None, "f32", ["random half"])


# ---------------------------------------------------------------------------------------------------- 2. natural stops
MAX_NFEV = 40


def natural_handle(L, pts, X0):
    prob = t_lm.problem(CASE)
    lower, upper = t_lm.starts_of(prob, 1)[1:]
    return L.LmDevice(pts, L.params_vector(prob["init"]), idx(prob["targets"]), lower, upper, X0, max_nfev=MAX_NFEV)


@pytest.mark.parametrize("n", [64, None])
def test_natural_stops_to_the_end(L, n):
    """1024 starts under max_nfev = 40, the host looking after every round: the list thins out as the starts converge, the rest
    end with status 0 at the 40th evaluation.  Then the same run without the host looking, and 48 of its starts alone."""
    K = 1024
    prob = t_lm.problem(CASE)
    X0 = t_lm.starts_of(prob, K)[0]
    with t_lm.points_of(L, prob, n) as pts:
        with natural_handle(L, pts, X0) as loop:
            prev, pending, rounds, stops = loop.get(), K, 0, []
            assert (prev["status"] == lc.RUNNING).all()
            while pending:
                loop.run(1)
                pending = loop.wait()
                rec = loop.get()
                rounds += 1
                running, was_stopped = rec["status"] == lc.RUNNING, prev["status"] != lc.RUNNING
                assert pending == int(running.sum()), rounds
                assert (rec["evaluations"][running] == rounds).all(), rounds
                same(rec, prev, (was_stopped, was_stopped), "round %d, a start that had stopped" % rounds)
                stops.append(int((~running & ~was_stopped).sum()))
                prev = rec
                assert rounds <= MAX_NFEV
        watched = prev
        print("n = %d: starts that stopped in round 1 .. %d: %s" % (pts.n, rounds, stops))
        print("evaluations: count", dict(zip(*[a.tolist() for a in np.unique(watched["evaluations"], return_counts=True)])))
        print("status: count", dict(zip(*[a.tolist() for a in np.unique(watched["status"], return_counts=True)])))
        assert sum(1 for s in stops if s) >= 3                   # else the list was never exercised
        assert set(watched["status"].tolist()) <= {-1, 0, 1, 2, 3, 4} and (watched["evaluations"] <= MAX_NFEV).all()
        assert (watched["evaluations"][watched["status"] == 0] == MAX_NFEV).all() and (watched["evaluations"][watched["status"] == -1] == 1).all()
        with natural_handle(L, pts, X0) as loop:                 # the same K: the same grid
            loop.run(1000)
            assert loop.wait() == 0
            same(loop.get(), watched, None, "check_every = 1000 against check_every = 1")
        slots = lc.subset_slots(K)
        if grid_of(L, pts.n, len(slots)) == grid_of(L, pts.n, K):
            with natural_handle(L, pts, X0[slots]) as loop:
                few = t_lm.run_to_the_end(loop)
            same(few, watched, (np.arange(len(slots)), slots), "48 starts alone against their slots among the 1024")
            print("48 starts alone: the bits of their slots among the 1024; they stopped after", few["evaluations"].tolist())
        else:
            assert n is None                                     # one stripe at 64 points, whatever the device
            print("48 starts alone: another grid than 1024 on this device, the 400-point comparison was not made")


# ---------------------------------------------------------------------------------------------------- 3. table rows
ROW_SLOTS = (0, 64, 256)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("n", [64, None])
def test_forced_stops_under_table_rows(L, n, precision):
    """K = 257 starts under the 257 rows of a bootstrap table: the stop sets that leave start 256 alone in the second pass,
    every other start, and a random half, against the rows handle with no stop; and the running starts among 0, 64 and 256
    against a handle of ONE start on a set whose weight plane is the start's row"""
    from alproj_amd import resample
    K = 257
    prob = t_lm.problem(CASE)
    X0, lower, upper = t_lm.starts_of(prob, K)
    targets = idx(prob["targets"])
    tmpl = L.params_vector(prob["init"])
    sets = lc.stop_sets(K)
    with t_lm.points_of(L, prob, n, precision) as pts, t_lm.points_of(L, prob, n, precision) as plane:
        table = resample.bootstrap_table(pts.n, K, lc.TABLE_SEED)
        assert len({row.tobytes() for row in table}) == K
        pts.set_weight_table(table)
        make = lambda: L.LmDevice(pts, tmpl, targets, lower, upper, X0, weight_rows=True)
        raw = batch_sums(L, pts, tmpl, targets, X0, np.arange(K))
        with make() as loop:
            ref, ref_waits = stepped(loop, raw, sets["none"])
        assert len(set(ref[-1]["cost"].tolist())) == K and (ref[-1]["status"] != -1).all()
        check_pattern("rows, none", X0, sets["none"], ref, ref_waits, ref)
        assert grid_of(L, pts.n, 1) == grid_of(L, pts.n, K)
        alone = {}
        for k in ROW_SLOTS:
            plane.set_weights(table[k])
            with L.LmDevice(plane, tmpl, targets, lower, upper, X0[k:k + 1]) as loop:
                alone[k] = stepped(loop, batch_sums(L, plane, tmpl, targets, X0[k:k + 1]), sets["none"])[0]
        for name in ("all but 256", "odd", "random half"):
            stop = sets[name]
            with make() as loop:
                recs, waits = stepped(loop, raw, stop)
            check_pattern("rows, %s" % name, X0, stop, recs, waits, ref)
            for k in np.setdiff1d(ROW_SLOTS, stop):
                for r in range(ROUNDS + 1):
                    same(recs[r], alone[k][r], (k, 0), "rows, %s, round %d: start %d against the one-start handle on its row" % (name, r, k))
        assert 256 not in sets["all but 256"] and not set(ROW_SLOTS) & set(sets["odd"].tolist())


# ---------------------------------------------------------------------------------------------------- 4. the Python drivers past 256
LOO_N = 300
LOO_FOLDS = (0, 63, 64, 255, 256, 257, 299)


def test_leave_one_out_over_300_points_on_the_device_loop(L):
    """cross_validate(folds="loo", device_loop=True) over 300 points = 300 starts under 300 table rows: folds on the seams are,
    bit for bit, the single weighted fit on the device loop, and lie within assert_close_fits' bounds (the noise study at the
    head of tests/test_gpu_lm_device.py) of the host lockstep's"""
    from alproj_amd import resample
    from tests.test_gpu_weight_table import assert_close_fits, lsq
    prob = t_lm.problem(CASE)
    assert grid_of(L, LOO_N, 1) == grid_of(L, LOO_N, LOO_N)
    dev = lsq(prob, LOO_N).cross_validate(folds="loo", device_loop=True)
    assert len(dev["fold_params"]) == len(dev["fold_results"]) == LOO_N and np.array_equal(dev["labels"], np.arange(LOO_N))
    train, _ = resample.fold_tables(dev["labels"])
    for b in LOO_FOLDS:
        o = lsq(prob, LOO_N, train[b])
        params, _ = o.optimize(method="normal", device_loop=True)
        got = dev["fold_results"][b]
        assert got["status"] in (1, 2, 3, 4), (b, got)
        assert {k: got[k] for k in ("cost", "iterations", "evaluations", "status")} == {k: o.result_[k] for k in ("cost", "iterations", "evaluations", "status")}, b
        assert got["grad_norm"] == o.result_["grad_norm"], b
        assert all(dev["fold_params"][b][t] == params[t] for t in prob["targets"]), b
    host = lsq(prob, LOO_N).cross_validate(folds="loo")
    lower, upper = t_lm.starts_of(prob, 1)[1:]
    rel = max(abs(dev["fold_results"][b]["cost"] / host["fold_results"][b]["cost"] - 1) for b in LOO_FOLDS)
    dx = max(abs(dev["fold_params"][b][t] - host["fold_params"][b][t]) / w for b in LOO_FOLDS for t, w in zip(prob["targets"], upper - lower))
    print("device loop against the host lockstep, folds %s: worst cost rel %.3g (tol 1e-8), worst x %.3g of the width (tol 1e-6)" %
          (list(LOO_FOLDS), rel, dx))
    print("evaluations (device, host):", [(dev["fold_results"][b]["evaluations"], host["fold_results"][b]["evaluations"]) for b in LOO_FOLDS])
    for b in LOO_FOLDS:
        assert_close_fits(prob, dev["fold_params"][b], dev["fold_results"][b]["cost"], host["fold_params"][b], host["fold_results"][b]["cost"],
                          "fold %d" % b)


def test_bootstrap_of_257_resamples_on_the_device_loop(L):
    """the leave-one-out fits above stop together; resamples do not, so here the list thins out under table rows: resamples on
    the seams are, bit for bit, the single weighted fit on the device loop"""
    from tests.test_gpu_weight_table import lsq
    prob = t_lm.problem(CASE)
    assert grid_of(L, LOO_N, 1) == grid_of(L, LOO_N, 257)
    boot = lsq(prob, LOO_N).bootstrap(n_boot=257, seed=lc.TABLE_SEED, device_loop=True)
    evaluations = [r["evaluations"] for r in boot["results"]]
    print("257 resamples: evaluations: count", dict(zip(*[a.tolist() for a in np.unique(evaluations, return_counts=True)])))
    assert boot["samples"].shape == (257, len(prob["targets"]))
    late = np.flatnonzero(np.array(evaluations) > min(evaluations))
    assert 0 < len(late) < 257                                   # else the list was the identity to the end
    for b in sorted({0, 63, 64, 255, 256} | set(late[:8].tolist())):        # the seams, and fits that ran on in a thin list
        o = lsq(prob, LOO_N, boot["counts"][b].astype(np.float64))
        params, _ = o.optimize(method="normal", device_loop=True)
        got = boot["results"][b]
        assert got["status"] in (1, 2, 3, 4), (b, got)
        assert got == o.result_, b
        assert boot["samples"][b].tolist() == [params[t] for t in prob["targets"]], b


def test_optimize_device_loop_with_300_starts(L):
    from alproj_amd import optimize as aopt
    prob = t_lm.problem(CASE)
    o = t_lm.lsq(prob)
    params, err = o.optimize(method="normal", starts=300, device_loop=True, seed=1)
    assert len(o.start_results) == 300
    costs = np.array([r[2]["cost"] for r in o.start_results])
    status = [r[2]["status"] for r in o.start_results]
    print("300 starts: status: count", dict(zip(*[a.tolist() for a in np.unique(status, return_counts=True)])), "best start", o.result_["start"])
    assert set(status) <= {-1, 0, 1, 2, 3, 4}
    assert np.isfinite(costs).any() and o.result_["start"] == int(np.nanargmin(costs)) == aopt.best_start(costs)
    assert (params, err) == o.start_results[o.result_["start"]][:2]
    assert o.result_ == dict(o.start_results[o.result_["start"]][2], start=o.result_["start"])
    # the first eight starts are those of starts=8 (the draw is prefix-stable), the run tests/test_gpu_lm_device.py holds
    if grid_of(L, len(prob["xyz"]), 8) == grid_of(L, len(prob["xyz"]), 300):
        few = t_lm.lsq(prob)
        few.optimize(method="normal", starts=8, device_loop=True, seed=1)
        for k in range(8):                                       # (the mean distance comes from another launch: not compared)
            assert (o.start_results[k][0], o.start_results[k][2]) == (few.start_results[k][0], few.start_results[k][2]), k
    else:
        print("starts=8: another grid than starts=300 on this device, not compared")
