"""GPU: the normal equations of B poses in one launch (alp_normal_equations_batch / normal_poses_kernel) and
LsqOptimizer.optimize(method="normal", starts=...).

A row of the batch against the single call (alp_normal_equations) at the same pose: the per-point arithmetic is the same code,
so the two differ by the order of the additions alone, and only where the points are cut into stripes differently.  A row
depends on its pose and its stripes alone: where B poses get the stripes one pose gets (host/alp_plan.h: normal_batch_grid(n, B,
cus) == normal_batch_grid(n, 1, cus) -- up to 256 points there is one group and so one stripe either way) it is bit for bit.
Elsewhere: both are within 2 m eps of the normalisers
(m = 2N rows, tests/test_gpu_normal.py's derivation) of the library's own Jacobian and residuals contracted on the host, and
the row is held to that file's bound against those, 4 m eps.  Against the complex-step oracle: tests/test_gpu_normal.py's TOL.
Everything else here is bit for bit: a row does not depend on the other rows, on their order or on their number as long as
the stripes stay (host/alp_plan.h: normal_batch_grid), nor on a communicator of one rank."""
import ctypes
import functools

import numpy as np
import pandas as pd
import pytest

from oracle import ref_numpy as orc
from tests import normal_batch_cases as nb
from tests import normal_cases as nc
from tests.test_gpu_normal import (D_TARGETS, EINVAL, ESTATE, TOL, assert_reassociation_only, frames, g5, g5_candidates, host_pieces,
                                   idx, median_scale, pole_problem, synthetic)
from tests.test_jacobian_oracle import KEYS, TARGETS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


@functools.lru_cache(maxsize=None)
def points(n):
    """tests/test_gpu_normal.py: synthetic(n, seed=n), made once per size -> xyz, uv, origin"""
    xyz, uv, p = synthetic(n, seed=n)
    return xyz, uv, [p["x"], p["y"], p["z"]]


@functools.lru_cache(maxsize=None)
def three_poses():
    """g5's candidates 0, 7 and 20 as a (3, 25) matrix"""
    from alproj_amd import _lib
    return np.array([_lib.params_vector(p) for p in g5_candidates()])


def poses(B, seed=0):
    """B distinct poses: the three candidates in turn, each moved by up to 0.05 degrees of pan and tilt"""
    rng = np.random.default_rng(seed)
    cand = three_poses()[np.arange(B) % 3].copy()
    cand[:, KEYS.index("pan")] += rng.uniform(-0.05, 0.05, B)
    cand[:, KEYS.index("tilt")] += rng.uniform(-0.05, 0.05, B)
    assert len({r.tobytes() for r in cand}) == B
    return cand


def row(out, b):
    return out[0][b], out[1][b], float(out[2][b]), out[3]


def assert_same_bits(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


# ---------------------------------------------------------------------------------------------------- 6. B = 1
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_batch_of_one_is_the_single_call_bit_for_bit(L, precision):
    xyz, uv, origin = points(4095)
    fs = 1.7
    with L.Points(xyz, origin, precision) as pts:
        pts.set_observed(uv)
        for loss in nc.LOSSES:
            for pv in three_poses()[:2]:
                one = pts.normal_equations_batch(pv[None, :], idx(TARGETS), loss, fs)
                assert one[0].shape == (1, 23, 23) and one[1].shape == (1, 23) and one[2].shape == (1,) and one[3] == 4095
                assert_same_bits(row(one, 0), pts.normal_equations(pv, idx(TARGETS), loss, fs))


# ---------------------------------------------------------------------------------------------------- 7. rows against single calls
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 100_003])
def test_rows_against_single_calls(L, n):
    xyz, uv, origin = points(n)
    cand = three_poses()
    cus = L.device_info()["cu_count"]
    same_stripes = nb.normal_batch_grid(n, 3, cus) == nb.normal_batch_grid(n, 1, cus)
    assert same_stripes or n > 256
    with L.Points(xyz, origin, "f64") as pts:
        pts.set_observed(uv)
        for D in (1, 15, 16, 23):
            targets = D_TARGETS[D]
            got = pts.normal_equations_batch(cand, idx(targets))
            assert got[0].shape == (3, D, D) and got[1].shape == (3, D) and got[2].shape == (3,) and got[3] == n
            for b in range(3):
                if same_stripes:
                    assert_same_bits(row(got, b), pts.normal_equations(cand[b], idx(targets)))
                else:
                    assert_reassociation_only(row(got, b), host_pieces(L, pts, cand[b], targets))
        assert (got[2][0] != got[2][1]) and (got[2][1] != got[2][2])             # three poses, three costs


def test_rows_of_other_stripes_against_the_host_contraction(L):
    """64 poses over 100 003 points cut a pose's 391 groups into far fewer stripes than one pose gets (24 against 391 on 256
    CUs): the same sums in another order"""
    n, D, B = 100_003, 23, 64
    xyz, uv, origin = points(n)
    cand = poses(B, seed=B)
    cus = L.device_info()["cu_count"]
    assert nb.normal_batch_grid(n, B, cus) != nb.normal_batch_grid(n, 1, cus)
    targets = D_TARGETS[D]
    with L.Points(xyz, origin, "f64") as pts:
        pts.set_observed(uv)
        got = pts.normal_equations_batch(cand, idx(targets))
        assert got[0].shape == (B, D, D) and got[3] == n
        for b in (0, B - 1):
            assert_reassociation_only(row(got, b), host_pieces(L, pts, cand[b], targets))


# ---------------------------------------------------------------------------------------------------- 8. rows against the oracle
@pytest.mark.parametrize("loss", nc.LOSSES)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_rows_against_the_oracle(L, precision, loss):
    xyz, uv = g5()["xyz"], g5()["uv_obs"]
    cands = g5_candidates()
    fs = median_scale(xyz, uv, cands[0])
    origin = [cands[0]["x"], cands[0]["y"], cands[0]["z"]]
    with L.Points(xyz, origin, precision) as pts:
        pts.set_observed(uv)
        got = pts.normal_equations_batch(three_poses(), idx(TARGETS), loss, fs)
    for b, p in enumerate(cands):
        nc.assert_sums_close(row(got, b), nc.normal_oracle(xyz, uv, orc.params_to_vector(p), TARGETS, loss, fs), *TOL[precision])


# ---------------------------------------------------------------------------------------------------- 9. row independence
@pytest.mark.parametrize("B", [2, 64, 1024])
def test_rows_do_not_depend_on_each_other(L, B):
    xyz, uv, origin = points(4095)
    cand = poses(B, seed=B)
    targets = idx(TARGETS)
    with L.Points(xyz, origin, "f64") as pts:
        pts.set_observed(uv)
        got = pts.normal_equations_batch(cand, targets, "huber", 1.7)
        assert got[0].shape == (B, 23, 23) and got[3] == 4095
        assert_same_bits(got, pts.normal_equations_batch(cand, targets, "huber", 1.7))           # the same call, the same bits
        perm = np.random.default_rng(B).permutation(B)
        if (perm == np.arange(B)).all():           # a draw may be the identity (B = 2): take the reversal
            perm = perm[::-1].copy()
        assert (perm != np.arange(B)).any()
        shuffled = pts.normal_equations_batch(cand[perm], targets, "huber", 1.7)
        assert_same_bits(shuffled, (got[0][perm], got[1][perm], got[2][perm], got[3]))
        twice = cand.copy()
        twice[B - 1] = cand[0]
        dup = pts.normal_equations_batch(twice, targets, "huber", 1.7)
        assert_same_bits(row(dup, B - 1), row(dup, 0))
        assert_same_bits(row(dup, 0), row(got, 0))
        if B > 2:
            assert_same_bits(row(dup, 1), row(got, 1))
        assert len({float(c) for c in got[2]}) == B
        # B = 1024 cuts the 16 groups into 2 stripes per pose, the single call into 16: the same sums in another order
        lin = pts.normal_equations_batch(cand, targets)
        for b in (0, B // 2, B - 1):
            assert_reassociation_only(row(lin, b), host_pieces(L, pts, cand[b], TARGETS))
    assert nb.normal_batch_grid(4095, 1024, 256) != nc.normal_grid(4095, 256)


# ---------------------------------------------------------------------------------------------------- 10. a pole in one row
def test_a_pole_in_one_row_stays_in_its_row(L):
    xyz, uv, truth, i, a2_pole = pole_problem(L)
    targets = idx(["pan", "a2", "k1", "cx"])
    clean = np.array([L.params_vector(truth), L.params_vector(dict(truth, pan=truth["pan"] + 0.01))])
    on = L.params_vector(dict(truth, a2=a2_pole))
    off = L.params_vector(dict(truth, a2=a2_pole + 2.0 ** -20))
    with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], "f64") as pts:
        pts.set_observed(uv)
        without = pts.normal_equations_batch(clean, targets)
        with_pole = pts.normal_equations_batch(np.array([clean[0], on, clean[1]]), targets)
        beside = pts.normal_equations_batch(np.array([clean[0], off, clean[1]]), targets)
        single = pts.normal_equations(on, targets)
    assert nb.normal_batch_grid(len(xyz), 2, 256) == nb.normal_batch_grid(len(xyz), 3, 256)    # the same stripes: bit for bit
    assert not np.isfinite(with_pole[2][1]) and not np.isfinite(with_pole[0][1][1, 1]) and not np.isfinite(with_pole[1][1][1])
    assert not np.isfinite(single[2])
    for other in (with_pole, beside):
        assert_same_bits(row(other, 0), row(without, 0))
        assert_same_bits(row(other, 2), row(without, 1))
    assert np.isfinite(beside[0]).all() and np.isfinite(beside[1]).all() and np.isfinite(beside[2]).all()
    assert np.isfinite(without[0]).all() and np.isfinite(without[2]).all()


# ---------------------------------------------------------------------------------------------------- 11. empty, errors, communicator
def test_empty_set_gives_rows_of_zeros(L):
    with L.Points(np.zeros((0, 3)), [0, 0, 0], "f64") as pts:
        pts.set_observed(np.zeros((0, 2)))
        Gm, g, cost, n = pts.normal_equations_batch(three_poses(), idx(["pan", "k1", "cx"]), "huber", 2.0)
        raw = np.full((3, 3 * 4 // 2 + 3 + 2), 7.0)
        tp = np.array(idx(["pan", "k1", "cx"]), dtype=np.int32)
        assert L.lib().alp_normal_equations_batch(pts._h, L.as_dp(three_poses()), 3, tp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 3, 2,
                                                  2.0, L.as_dp(raw)) == 0
    assert Gm.shape == (3, 3, 3) and not Gm.any() and g.shape == (3, 3) and not g.any() and not cost.any() and n == 0
    assert not raw.any()


def test_error_paths(L):
    xyz, uv, _ = points(64)
    lib = L.lib()
    I32 = ctypes.POINTER(ctypes.c_int32)
    cand = three_poses()
    out = np.empty(3 * 400)
    good = np.array(idx(["pan", "tilt"]), dtype=np.int32)
    tp = good.ctypes.data_as(I32)
    with L.Points(xyz, points(64)[2], "f64") as pts:
        call = lib.alp_normal_equations_batch
        assert call(pts._h, L.as_dp(cand), 3, tp, 2, 0, 1.0, L.as_dp(out)) == ESTATE      # no observed uv yet, as the single call
        assert lib.alp_normal_equations(pts._h, L.as_dp(cand[0]), tp, 2, 0, 1.0, L.as_dp(out)) == ESTATE
        pts.set_observed(uv)
        assert call(pts._h, L.as_dp(cand), 3, tp, 2, 0, 1.0, L.as_dp(out)) == 0
        assert call(None, L.as_dp(cand), 3, tp, 2, 0, 1.0, L.as_dp(out)) == EINVAL
        assert call(pts._h, None, 3, tp, 2, 0, 1.0, L.as_dp(out)) == EINVAL
        assert call(pts._h, L.as_dp(cand), 3, None, 2, 0, 1.0, L.as_dp(out)) == EINVAL
        assert call(pts._h, L.as_dp(cand), 3, tp, 2, 0, 1.0, None) == EINVAL
        for B in (0, -1, 1025, -2 ** 40, 2 ** 40):
            assert call(pts._h, L.as_dp(cand), B, tp, 2, 0, 1.0, L.as_dp(out)) == EINVAL, B
        many = np.arange(25, dtype=np.int32)
        for D in (0, 24, -1):
            assert call(pts._h, L.as_dp(cand), 3, many.ctypes.data_as(I32), D, 0, 1.0, L.as_dp(out)) == EINVAL
        for bad in ([KEYS.index("w")], [KEYS.index("pan"), KEYS.index("h")], [4, 4], [25], [-1]):
            b = np.array(bad, dtype=np.int32)
            assert call(pts._h, L.as_dp(cand), 3, b.ctypes.data_as(I32), len(bad), 0, 1.0, L.as_dp(out)) == EINVAL, bad
        for loss in (-1, 4, 99):
            assert call(pts._h, L.as_dp(cand), 3, tp, 2, loss, 1.0, L.as_dp(out)) == EINVAL
        for fs in (0.0, -1.0, float("inf"), float("nan")):
            assert call(pts._h, L.as_dp(cand), 3, tp, 2, 2, fs, L.as_dp(out)) == EINVAL
        for loss in range(4):
            assert call(pts._h, L.as_dp(cand), 3, tp, 2, loss, 1.5, L.as_dp(out)) == 0
        full = np.tile(cand, (342, 1))[:1024]
        big = np.empty((1024, 7))
        assert call(pts._h, L.as_dp(full), 1024, tp, 2, 0, 1.0, L.as_dp(big)) == 0
        np.testing.assert_array_equal(big[3], big[0])
        assert (big[:, 6] == 64).all()                                                     # the count, in every row


def test_world_1_communicator_gives_the_same_bits(L):
    xyz, uv, origin = points(100_003)
    cand = poses(5, seed=11)
    with L.Points(xyz, origin, "f32") as pts:
        pts.set_observed(uv)
        before = pts.normal_equations_batch(cand, idx(TARGETS), "soft_l1", 1.5)
        L.comm_init(L.comm_unique_id(), 0, 1)
        try:
            assert L.comm_info() == (0, 1)
            during = pts.normal_equations_batch(cand, idx(TARGETS), "soft_l1", 1.5)
        finally:
            L.comm_destroy()
        after = pts.normal_equations_batch(cand, idx(TARGETS), "soft_l1", 1.5)
    for other in (during, after):
        assert_same_bits(before, other)
    assert before[3] == 100_003


# ---------------------------------------------------------------------------------------------------- 12. the public multi-start
def check_starts(o, prob, params, err, loss, f_scale, K):
    from alproj_amd import optimize as aopt
    assert len(o.start_results) == K
    costs = [r[2]["cost"] for r in o.start_results]
    for p, e, res in o.start_results:
        assert set(p) == set(prob["want"]) and set(res) == {"cost", "iterations", "evaluations", "status", "grad_norm"}
        if np.isfinite(res["cost"]):
            assert res["cost"] == pytest.approx(nc.cost_at(prob, p, loss, f_scale), rel=1e-9)
            assert e == pytest.approx(nc.mean_distance(prob, p), rel=1e-9)
    b = aopt.best_start(costs)
    assert o.result_ == dict(o.start_results[b][2], start=b)
    assert params == o.start_results[b][0] and err == o.start_results[b][1]
    assert costs[b] == min(c for c in costs if np.isfinite(c))
    return costs


@pytest.mark.parametrize("case", list(nc.LSQ_KW))
def test_optimize_normal_with_eight_starts(L, case):
    from alproj_amd import optimize as aopt
    prob = nc.g14_problem(case)
    kw = nc.LSQ_KW[case]
    loss, f_scale = kw.get("loss", "linear"), kw.get("f_scale", 1.0)
    o = aopt.LsqOptimizer(*frames(prob), dict(prob["init"]))
    o.set_target(prob["targets"])
    if kw.get("unbounded"):
        # no box to draw in: the integer form refuses, explicit starts (the integer rule in the box of the default widths) run
        with pytest.raises(ValueError):
            o.optimize(method="normal", bound_widths=nc.widths_of(case), starts=8, seed=1)
        lower, upper = nc.bounds_of(prob, None)
        starts = nb.integer_starts(np.array([prob["init"][t] for t in prob["targets"]]), lower, upper, 8, 1)
    else:
        starts = 8
    params, err = o.optimize(method="normal", bound_widths=nc.widths_of(case), loss=loss, f_scale=f_scale, starts=starts, seed=1)
    print(case, o.result_, [(r[2]["status"], r[2]["evaluations"], r[2]["cost"]) for r in o.start_results])
    costs = check_starts(o, prob, params, err, loss, f_scale, 8)
    p0, e0, r0 = o.start_results[0]
    assert r0["status"] in (1, 2, 3, 4)
    nc.assert_reference_optimum(prob, p0, e0, r0["cost"], loss, f_scale)
    assert o.result_["cost"] <= r0["cost"] and costs[o.result_["start"]] == o.result_["cost"]
    # the same seed, the same starts, the same bits; start 0 is the single-start run's start
    again = aopt.LsqOptimizer(*frames(prob), dict(prob["init"]))
    again.set_target(prob["targets"])
    assert again.optimize(method="normal", bound_widths=nc.widths_of(case), loss=loss, f_scale=f_scale, starts=starts, seed=1) == (params, err)
    assert again.result_ == o.result_


def test_optimize_normal_polishes_the_starts_of_a_cma_run(L):
    from alproj_amd import optimize as aopt
    prob = nc.g14_problem("trf_linear_d7")
    cma = aopt.CMAOptimizer(*frames(prob), dict(prob["init"]))
    cma.set_target(prob["targets"])
    best_params, _ = cma.optimize(generation=30, population_size=12, seed=3, progress=False, starts=4)
    found = [r[1] for r in cma.start_results]
    assert len(found) == 4 and best_params in found
    o = aopt.LsqOptimizer(*frames(prob), dict(prob["init"]))
    o.set_target(prob["targets"])
    params, err = o.optimize(method="normal", starts=found)
    check_starts(o, prob, params, err, "linear", 1.0, 4)
    alone = aopt.LsqOptimizer(*frames(prob), dict(prob["init"]))
    alone.set_target(prob["targets"])
    alone.optimize(method="normal", starts=[best_params])
    print("polished: all four", o.result_, "the CMA winner alone", alone.result_)
    assert alone.result_["start"] == 0 and len(alone.start_results) == 1
    assert o.result_["cost"] <= alone.result_["cost"]
    # a row does not depend on the others: the winner's run is the same run inside the four
    assert o.start_results[found.index(best_params)][2] == alone.start_results[0][2]
    # ... and a (K, D) array of target values is the same thing as the dicts
    arr = aopt.LsqOptimizer(*frames(prob), dict(prob["init"]))
    arr.set_target(prob["targets"])
    assert arr.optimize(method="normal", starts=np.array([[f[t] for t in prob["targets"]] for f in found])) == (params, err)


def test_optimize_normal_with_starts_on_a_float32_set(L):
    from alproj_amd import optimize as aopt
    prob = nc.g14_problem("trf_linear_d7")
    o = aopt.LsqOptimizer(*frames(prob), dict(prob["init"]))
    o.set_target(prob["targets"])
    params, err = o.optimize(method="normal", precision="f32", starts=8, seed=1)
    print("f32", o.result_)
    assert o.result_["status"] in (1, 2, 3, 4) and len(o.start_results) == 8 and np.isfinite(err)
    assert o.result_["start"] == aopt.best_start([r[2]["cost"] for r in o.start_results])
