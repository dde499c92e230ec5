"""GPU checks of the weight table (alp_points_set_weight_table), the row-weighted normal equations
(alp_normal_equations_batch_rows, alp_lm_create_rows), the assigned residuals (alp_residuals_assigned) and what
LsqOptimizer.cross_validate / .bootstrap build on them.

The reference of a table row is the per-point weight plane: ``set_weights(table[r])`` + ``normal_equations_batch`` -- the same
grid, the same stripes, the same additions, so the comparison is bit for bit.  The weighted plane itself is held to the oracle
on duplicated rows by tests/test_gpu_weighted.py; one test here repeats that for table rows at the same tolerances."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ref_numpy as orc
from tests import lm_device_cases as lc
from tests import normal_batch_cases as nb
from tests import normal_cases as nc
from tests import popeval_cases as pc
from tests import test_gpu_lm_device as t_lm
from tests import test_gpu_normal as t_normal
from tests import test_gpu_normal_batch as t_batch
from tests import test_gpu_weighted as t_w
from tests.test_jacobian_oracle import KEYS, TARGETS

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6
I32 = ctypes.POINTER(ctypes.c_int32)
bits = t_w.bits
D_TARGETS = t_w.D_TARGETS                  # D = 1, 16, 17, 23
STRADDLE = 24 * 256 * 2 + 5                # 49 groups of 256 points: the last stripe of every grid below holds 5 points


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def table_of(n, R, seed=0):
    """R rows of n weights, by row index mod 5: integer counts 0..3 | uniform fractions | a 0/1 mask | integer counts 1..4 |
    fractions with two thirds of the points at 0"""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(R):
        kind = r % 5
        if kind == 0:
            rows.append(rng.integers(0, 4, n).astype(np.float64))
        elif kind == 1:
            rows.append(rng.uniform(0, 3, n))
        elif kind == 2:
            rows.append((rng.uniform(0, 1, n) < 0.7).astype(np.float64))
        elif kind == 3:
            rows.append(rng.integers(1, 5, n).astype(np.float64))
        else:
            rows.append(np.where(rng.uniform(0, 1, n) < 2 / 3, 0.0, rng.uniform(0, 2, n)))
        if not rows[-1].sum() > 0:             # (a handful of points: the reference, set_weights, refuses weights that are all 0)
            rows[-1][0] = 1.0
    return np.array(rows)


def same_rows(got, b, ref, bb):
    """row b of a normal_equations_batch_rows result against row bb of a normal_equations_batch result, bit for bit"""
    for k in range(3):
        assert np.array_equal(bits(got[k][b]), bits(ref[k][bb])), ("G", "g", "cost")[k]


def index_order_sum(stored):
    s = 0.0
    for v in np.asarray(stored, dtype=np.float64):
        s += v
    return s


# ---------------------------------------------------------------------------------------------------- 1. bit equality
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, STRADDLE])
def test_rows_have_the_bits_of_the_weight_plane(L, n, precision):
    """every D, loss and row pattern; B = 1, 3 and 64.  The reference of (B, row r) is computed once per (D, loss)."""
    xyz, uv, origin = t_batch.points(n)
    cus = L.device_info()["cu_count"]
    if n == STRADDLE:
        for B in (1, 3, 64):
            stripes, per = nb.normal_batch_grid(n, B, cus)
            assert stripes > 1 and (stripes - 1) * per * 256 < n < stripes * per * 256        # the last stripe is cut short
    t3, t5 = table_of(n, 3, seed=n), table_of(n, 5, seed=n + 1)
    stored = (lambda t: t.astype(np.float32).astype(np.float64)) if precision == "f32" else (lambda t: t)
    cand = {B: t_batch.poses(B, seed=B) for B in (1, 3, 64)}
    patterns3 = {"identity": [0, 1, 2], "permutation": [2, 0, 1], "all equal": [1, 1, 1]}
    spread = np.arange(64) % 5                                           # R != B, every row repeated
    with L.Points(xyz, origin, precision) as pts:
        pts.set_observed(uv)
        for D, targets in D_TARGETS.items():
            cols = t_normal.idx(targets)
            for loss in nc.LOSSES:
                fs = 1.7
                # the references: the plane holds row r, the batch call runs the same poses
                ref3, ref5 = [], []
                for r in range(3):
                    pts.set_weights(t3[r])
                    ref3.append(pts.normal_equations_batch(cand[3], cols, loss, fs))
                for r in range(5):
                    pts.set_weights(t5[r])
                    ref5.append((pts.normal_equations_batch(cand[64], cols, loss, fs),
                                 pts.normal_equations_batch(cand[1], cols, loss, fs) if r == 3 else None))
                pts.set_weights(None)
                pts.set_weight_table(t3)
                W3 = pts.weight_table_sums()
                for name, rows in patterns3.items():
                    got = pts.normal_equations_batch_rows(cand[3], rows, cols, loss, fs)
                    for b, r in enumerate(rows):
                        same_rows(got, b, ref3[r], b)
                        assert got[3][b] == W3[r], name
                pts.set_weight_table(t5)
                W5 = pts.weight_table_sums()
                got = pts.normal_equations_batch_rows(cand[64], spread, cols, loss, fs)
                for b, r in enumerate(spread):
                    same_rows(got, b, ref5[r][0], b)
                    assert got[3][b] == W5[r]
                got = pts.normal_equations_batch_rows(cand[1], [3], cols, loss, fs)
                same_rows(got, 0, ref5[3][1], 0)
                assert got[3][0] == W5[3]
        # the row sums: exact for integer rows, within n ulp of the float64 sum in index order otherwise
        for t, W in ((t3, W3), (t5, W5)):
            for r, row in enumerate(stored(t)):
                ref = index_order_sum(row)
                if (row == np.floor(row)).all():
                    assert W[r] == ref == row.sum()
                else:
                    assert abs(W[r] - ref) <= n * np.spacing(ref), (r, W[r], ref)


# ---------------------------------------------------------------------------------------------------- 2. the oracle
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("loss", nc.LOSSES)
def test_integer_rows_against_the_oracle_on_repeated_rows(L, loss, precision):
    """tests/test_gpu_weighted.py::test_normal_equations_against_the_oracle_on_duplicated_rows for rows of a table: its set, its
    f_scale, its tolerances (tests/test_gpu_normal.py: TOL)"""
    xyz, uv, p, _ = t_w.weighted_normal_case(900, 4)
    fs = t_w.kink_free_scale(xyz, uv, p)
    table = np.random.default_rng(5).integers(0, 4, (2, 900)).astype(np.float64)
    pv = L.params_vector(p)
    refs = [nc.normal_oracle(np.repeat(xyz, table[r].astype(int), axis=0), np.repeat(uv, table[r].astype(int), axis=0),
                             orc.params_to_vector(p), TARGETS, loss, fs) for r in range(2)]
    with t_w.points(L, xyz, uv, [p["x"], p["y"], p["z"]], precision) as pts:
        pts.set_weight_table(table)
        G, g, cost, W = pts.normal_equations_batch_rows(np.tile(pv, (3, 1)), [1, 0, 1], t_normal.idx(TARGETS), loss, fs)
        for b, r in enumerate([1, 0, 1]):
            assert W[b] == table[r].sum()
            nc.assert_sums_close((G[b], g[b], float(cost[b]), int(W[b])), refs[r], *t_normal.TOL[precision])


# ---------------------------------------------------------------------------------------------------- 3. zero weights
@pytest.mark.parametrize("loss", nc.LOSSES)
def test_zero_weight_rows_and_a_poisoned_point(L, loss):
    t = pc.truth("general")
    xyz, uv = t_w.poisoned_set(t)                     # the last two vertices sit at the camera / on the camera plane
    n = len(xyz) - 2
    pv = L.params_vector(t)
    cols = t_normal.idx(TARGETS)
    w = np.random.default_rng(6).integers(1, 4, len(xyz)).astype(np.float64)
    clean, poisoned = w.copy(), w.copy()
    clean[n:] = 0.0
    table = np.array([clean, np.zeros(len(xyz)), poisoned])
    with t_w.points(L, xyz, uv, pc.origin(), "f64") as pts:
        pts.set_weight_table(table)
        G, g, cost, W = pts.normal_equations_batch_rows(np.tile(pv, (3, 1)), [0, 1, 2], cols, loss, 2.0)
        assert np.isfinite(G[0]).all() and np.isfinite(g[0]).all() and np.isfinite(cost[0]) and W[0] == clean.sum()
        assert cost[0] > 0
        for a in (G[1], g[1], cost[1], W[1]):          # an empty row: exact zeros, count 0
            assert np.array_equal(bits(a), bits(np.zeros_like(a)))
        assert not np.isfinite(G[2]).all() or not np.isfinite(cost[2])      # the control: a positive weight keeps the poison
        with t_w.points(L, xyz[:n], uv[:n], pc.origin(), "f64", w[:n]) as short:
            ref = short.normal_equations_batch(np.tile(pv, (3, 1)), cols, loss, 2.0)
        same_rows((G, g, cost), 0, ref, 0)


# ---------------------------------------------------------------------------------------------------- 4. table state
def test_a_refused_table_leaves_the_old_one_in_force_and_the_plane_alone(L):
    n = 300
    xyz, uv, origin = t_batch.points(257)
    xyz, uv = np.vstack([xyz, xyz[:n - 257] + 1.0]), np.vstack([uv, uv[:n - 257]])
    cand, cols = t_batch.poses(3), t_normal.idx(D_TARGETS[17])
    table, plane = table_of(n, 3, seed=1), np.random.default_rng(2).integers(0, 3, n).astype(np.float64)
    for precision in ("f64", "f32"):
        with L.Points(xyz, origin, precision) as pts:
            pts.set_observed(uv)
            lib = pts._lib
            assert lib.alp_normal_equations_batch_rows(pts._h, L.as_dp(cand), 3, np.zeros(3, np.int32).ctypes.data_as(I32),
                                                       np.array(cols, np.int32).ctypes.data_as(I32), 17, 0, 1.0,
                                                       L.as_dp(np.empty((3, 17 * 9 + 17 + 2)))) == ESTATE      # no table yet
            unweighted = pts.normal_equations_batch(cand, cols, "huber", 1.5)
            pts.set_weights(plane)
            with_plane = pts.normal_equations_batch(cand, cols, "huber", 1.5)
            pts.set_weight_table(table)
            before, sums = pts.normal_equations_batch_rows(cand, [0, 1, 2], cols, "huber", 1.5), pts.weight_table_sums()
            # the table does not disturb the plane's results ...
            for a, b in zip(pts.normal_equations_batch(cand, cols, "huber", 1.5), with_plane):
                assert np.array_equal(bits(a), bits(b))
            assert pts.weight_sum() == plane.sum()
            bad = {"negative": np.where(np.arange(n) == 3, -1.0, table), "nan": np.where(np.arange(n) == n - 1, np.nan, table),
                   "inf": np.where(np.arange(n) == 0, np.inf, table), "R = 0": table[:0], "R = 1025": np.ones((1025, n)),
                   "width": table[:, :-1], "1-d": table[0]}
            for name, t in bad.items():
                with pytest.raises(ValueError):
                    pts.set_weight_table(t)
            # the library itself, behind the Python checks
            for name in ("negative", "nan", "inf"):
                for dt, code in ((np.float64, L.ALP_F64), (np.float32, L.ALP_F32)):
                    t = np.ascontiguousarray(bad[name], dtype=dt)
                    assert lib.alp_points_set_weight_table(pts._h, t.ctypes.data_as(ctypes.c_void_p), 3, code) == EINVAL, name
            big = np.ones((1025, n))
            assert lib.alp_points_set_weight_table(pts._h, big.ctypes.data_as(ctypes.c_void_p), 1025, L.ALP_F64) == EINVAL
            assert lib.alp_points_set_weight_table(pts._h, big.ctypes.data_as(ctypes.c_void_p), 0, L.ALP_F64) == EINVAL
            assert lib.alp_points_set_weight_table(pts._h, table.ctypes.data_as(ctypes.c_void_p), 3, 7) == EINVAL
            if precision == "f32":
                huge = np.where(np.arange(n) == 1, 1e300, table)
                assert lib.alp_points_set_weight_table(pts._h, huge.ctypes.data_as(ctypes.c_void_p), 3, L.ALP_F64) == EINVAL
            with pytest.raises(ValueError):
                pts.normal_equations_batch_rows(cand, [0, 1, 3], cols)
            with pytest.raises(ValueError):
                pts.normal_equations_batch_rows(cand, [0, -1, 2], cols)
            rows = np.array([0, 1, 3], np.int32)
            assert lib.alp_normal_equations_batch_rows(pts._h, L.as_dp(cand), 3, rows.ctypes.data_as(I32), np.array(cols, np.int32).ctypes.data_as(I32),
                                                       17, 0, 1.0, L.as_dp(np.empty((3, 17 * 9 + 17 + 2)))) == EINVAL
            after = pts.normal_equations_batch_rows(cand, [0, 1, 2], cols, "huber", 1.5)
            for a, b in zip(after, before):
                assert np.array_equal(bits(a), bits(b))
            assert np.array_equal(pts.weight_table_sums(), sums)
            # ... nor the plane the table's: another plane, then none
            pts.set_weights(np.ones(n))
            pts.set_weights(None)
            for a, b in zip(pts.normal_equations_batch_rows(cand, [0, 1, 2], cols, "huber", 1.5), before):
                assert np.array_equal(bits(a), bits(b))
            for a, b in zip(pts.normal_equations_batch(cand, cols, "huber", 1.5), unweighted):
                assert np.array_equal(bits(a), bits(b))
            # pending evaluation: ALP_ESTATE, and the table stays
            pts.eval_population_enqueue(cand, L.LOSS_HUBER, 10.0)
            for t in (table, None):
                with pytest.raises(RuntimeError) as e:
                    pts.set_weight_table(t)
                assert e.value.code == ESTATE
            pts.eval_population_wait(3)
            pts.set_weight_table(None)
            with pytest.raises(RuntimeError) as e:
                pts.weight_table_sums()
            assert e.value.code == ESTATE


# ---------------------------------------------------------------------------------------------------- 5. residuals_assigned
@pytest.mark.parametrize("B", [1, 2, 64, 1024])
@pytest.mark.parametrize("n", [1, 64, 257, 1000])
def test_residuals_assigned_are_the_gathered_rows_of_residuals_batch(L, n, B):
    """B = 64 and below: the records are staged in LDS; 1024: read from global memory"""
    xyz, uv, origin = t_batch.points(n)
    cand = t_batch.poses(B, seed=B)
    rng = np.random.default_rng(n + B)
    with L.Points(xyz, origin, "f64") as pts:
        pts.set_observed(uv)
        full = pts.residuals_batch(cand).reshape(B, n, 2)
        some = rng.integers(0, B, n)
        some[rng.uniform(0, 1, n) < 0.3] = -1
        some[0] = -1
        for name, assign in (("one pose", np.full(n, B - 1)), ("round robin", np.arange(n) % B), ("with -1", some)):
            got = pts.residuals_assigned(cand, assign).reshape(n, 2)
            out = assign < 0
            assert np.isnan(got[out]).all(), name
            assert np.array_equal(bits(got[~out]), bits(full[assign[~out], np.flatnonzero(~out)])), name
        with pytest.raises(ValueError):
            pts.residuals_assigned(cand, np.full(n, B))
        bad = np.zeros(n, np.int32)
        bad[n - 1] = B
        out = np.empty(2 * n)
        assert pts._lib.alp_residuals_assigned(pts._h, L.as_dp(cand), B, bad.ctypes.data_as(I32), L.as_dp(out)) == EINVAL


def test_residuals_assigned_on_a_float32_set_is_float64_arithmetic_on_the_stored_points(L):
    xyz, uv, origin = t_batch.points(257)
    cand = t_batch.poses(3)
    assign = np.arange(257) % 3
    with L.Points(xyz, origin, "f32") as p32, L.Points(xyz, origin, "f64") as p64:
        p32.set_observed(uv)
        p64.set_observed(uv)
        got, ref = p32.residuals_assigned(cand, assign), p64.residuals_assigned(cand, assign)
    assert np.isfinite(got).all() and np.abs(got - ref).max() < 0.05 and not np.array_equal(got, ref)


# ---------------------------------------------------------------------------------------------------- 6. the device loop
@pytest.mark.parametrize("n", [None, 257])
def test_the_listed_kernel_of_the_device_loop_under_table_rows(L, n):
    """tests/test_gpu_weighted.py::test_the_listed_kernel_of_the_device_loop_on_a_weighted_set with a row per start: one handle
    runs a round, its twin is stepped on alp_normal_equations_batch_rows' sums at the same trial points"""
    prob = t_lm.problem("trf_linear_d7")
    K = 3
    X0, lower, upper = t_lm.starts_of(prob, K)
    targets = t_normal.idx(prob["targets"])
    tp = np.array(targets, dtype=np.int32)
    rows = np.arange(K, dtype=np.int32)
    D = len(targets)
    tmpl = L.params_vector(prob["init"])
    with t_lm.points_of(L, prob, n) as pts:
        table = table_of(pts.n, K, seed=8)
        with pytest.raises(RuntimeError) as e:                  # no table
            L.LmDevice(pts, tmpl, targets, lower, upper, X0, weight_rows=True)
        assert e.value.code == ESTATE
        pts.set_weight_table(table[:2])
        with pytest.raises(RuntimeError) as e:                  # R != K
            L.LmDevice(pts, tmpl, targets, lower, upper, X0, weight_rows=True)
        assert e.value.code == EINVAL
        pts.set_weight_table(table)
        pts.set_weights(np.full(pts.n, 7.0))                    # the plane is ignored under table rows
        sums = pts.weight_table_sums()
        with L.LmDevice(pts, tmpl, targets, lower, upper, X0, weight_rows=True) as a, \
                L.LmDevice(pts, tmpl, targets, lower, upper, X0, weight_rows=True) as b:
            for rnd in range(3):
                trial = b.get()["trial"]
                cand = np.tile(tmpl, (K, 1))
                cand[:, targets] = trial
                raw = np.empty((K, D * (D + 1) // 2 + D + 2))
                assert L.lib().alp_normal_equations_batch_rows(pts._h, L.as_dp(cand), K, rows.ctypes.data_as(I32), tp.ctypes.data_as(I32), D, 0,
                                                               1.0, L.as_dp(raw)) == 0
                assert np.array_equal(raw[:, -1], sums)
                a.run(1)
                with pytest.raises(RuntimeError) as e:          # rounds are pending
                    pts.set_weight_table(table)
                assert e.value.code == ESTATE
                a.wait()
                b.step_host(raw)
                ra, rb = a.get(), b.get()
                dev = float(np.max(np.abs(ra["trial"] - rb["trial"]) / (upper - lower)))
                rel = lambda u, v: float(np.max(np.abs(u - v) / np.abs(v)))
                print("round %d: trial deviation %.3g of the width, cost rel %.3g" % (rnd, dev, rel(ra["cost"], rb["cost"])))
                assert dev <= lc.TRIAL_TOL and rel(ra["cost"], rb["cost"]) <= lc.TRIAL_TOL and rel(ra["mu"], rb["mu"]) <= lc.TRIAL_TOL
                np.testing.assert_array_equal(ra["status"], rb["status"])
                np.testing.assert_array_equal(ra["evaluations"], rb["evaluations"])
            assert len(set(ra["cost"].tolist())) == K           # three rows, three problems
            pts.set_weight_table(table[:2])                     # another height under a living loop
            with pytest.raises(RuntimeError) as e:
                a.run(1)
            assert e.value.code == ESTATE


# A pose whose plan the host and the device fold to the same bits.  The loop folds a start's plan on the device, the library
# call on the host, and the two differ by the device's sin / cos / tan alone (tests/test_gpu_lm_device.py), so a comparison of
# the two bit for bit needs a pose where those agree: pan = roll = 0 and tilt = -90 (a camera looking straight down) make
# every angle of host/alp_fold.h a zero, whose sine and cosine are exact everywhere, and at fov = 52 on the 5616 x 3744 image
# both tangents of the fold (of 0.4537.. and 0.3025..) lie within 0.06 ulp of a double, which every tangent good to 0.9 ulp
# returns.  None of the four is a target below, so they stay what they are in every round.
NADIR_FOV = 52.0
NADIR_TARGETS = ["x", "y", "z", "a1", "a2", "k1", "k2"]
NADIR_WIDTH = np.array([40.0, 40.0, 40.0, 0.1, 0.1, 0.05, 0.02])


@functools.lru_cache(maxsize=None)
def nadir_problem(n):
    from alproj_amd import synthetic as syn
    p = dict(syn.truth_params(316), pan=0.0, tilt=-90.0, roll=0.0, fov=NADIR_FOV)
    xyz = syn.gcp_points(n, p, seed=7)
    uv = orc.project_points(xyz, p) + np.random.default_rng(7).normal(0, 1.0, (n, 2))
    centre = np.array([float(p[t]) for t in NADIR_TARGETS])
    X0 = centre + np.random.default_rng(8).uniform(-0.25, 0.25, (3, len(NADIR_TARGETS))) * NADIR_WIDTH
    return p, xyz, uv, X0, centre - NADIR_WIDTH, centre + NADIR_WIDTH


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("n", [64, 257])
def test_the_listed_kernel_under_table_rows_after_a_start_has_ended(L, n, precision):
    """A listed launch under table rows in which list[b] != b.  Three device loops of K = 3 starts under a 3-row table; start 0
    of `ended` and `twin` has a NaN coordinate (np.clip keeps it), so it ends at its first evaluation and the two rounds after
    it run list = [1, 2]: workgroup slot b takes start b + 1, its plan, its weight row and its partial rows (257 points: two
    stripes, the second group ragged; 64: one).
      ended  runs its rounds on the device;
      twin   is stepped (alp_lm_step_host) on alp_normal_equations_batch_rows' sums of the trial points of starts 1 and 2 under
             row_of_pose = [1, 2]; the row of start 0: NaN in the first round (what the evaluation at a NaN pose gives), then
             zeros, its own row's weight sum in the count slot;
      whole  is `ended` with a finite start 0: all three starts run, list = [0, 1, 2].
    In every round the records of starts 1 and 2 are the same BIT FOR BIT in all three.  The loop's sums cannot be read back,
    but lm_step_kernel is the same code on the three handles, and one differing bit in G, g or the cost of a round shows in
    cost, x, mu or the next trial point (nadir_problem's pose: the host-built plan of the library call has the bits of the
    device-built one).  The row of sums of the ended start cannot be read either; what it stands for is held: status -1 after
    one evaluation, and a record that never moves again."""
    p, xyz, uv, X0, lower, upper = nadir_problem(n)
    K = 3
    X0_nan = X0.copy()
    X0_nan[0, 0] = np.nan
    targets = t_normal.idx(NADIR_TARGETS)
    tp = np.array(targets, dtype=np.int32)
    rows = np.array([1, 2], dtype=np.int32)
    D = len(targets)
    tmpl = L.params_vector(p)
    with t_w.points(L, xyz, uv, [p["x"], p["y"], p["z"]], precision) as pts:
        pts.set_weight_table(table_of(pts.n, K, seed=9))
        pts.set_weights(np.full(pts.n, 7.0))                    # the plane is ignored under table rows
        sums = pts.weight_table_sums()
        assert len(set(sums.tolist())) == K                     # three rows, three problems
        loop = lambda starts: L.LmDevice(pts, tmpl, targets, lower, upper, starts, weight_rows=True)
        with loop(X0_nan) as ended, loop(X0_nan) as twin, loop(X0) as whole:
            for rnd in range(3):
                rec = twin.get()
                assert (rec["status"][1:] == lc.RUNNING).all() and (rec["status"][0] == lc.RUNNING) == (rnd == 0)
                cand = np.tile(tmpl, (2, 1))
                cand[:, targets] = rec["trial"][1:]
                raw = np.zeros((K, D * (D + 1) // 2 + D + 2))
                assert L.lib().alp_normal_equations_batch_rows(pts._h, L.as_dp(cand), 2, rows.ctypes.data_as(I32), tp.ctypes.data_as(I32), D, 0,
                                                               1.0, L.as_dp(raw[1:])) == 0
                assert np.array_equal(raw[1:, -1], sums[1:])
                if rnd == 0:
                    raw[0] = np.nan
                raw[0, -1] = sums[0]
                ended.run(1)
                assert ended.wait() == 2
                whole.run(1)
                assert whole.wait() == 3
                twin.step_host(raw)
                r_end, rt, rw = ended.get(), twin.get(), whole.get()
                dev = float(np.max(np.abs(r_end["trial"][1:] - rt["trial"][1:]) / (upper - lower)))
                print("round %d: trial deviation of the twin %.3g of the width, cost rel %.3g" %
                      (rnd, dev, float(np.max(np.abs(r_end["cost"][1:] - rt["cost"][1:]) / np.abs(rt["cost"][1:])))))
                assert r_end["status"][0] == -1 and r_end["evaluations"][0] == 1 and not np.isfinite(r_end["cost"][0])
                if rnd == 0:
                    first = r_end
                t_lm.same_bits(r_end, first, rows=(0, 0))
                for k in (1, 2):
                    t_lm.same_bits(r_end, rw, rows=(k, k))
                    t_lm.same_bits(r_end, rt, rows=(k, k))
            assert (r_end["evaluations"][1:] == 3).all() and r_end["cost"][1] != r_end["cost"][2]


def lsq(prob, n=None, weights=None):
    from alproj_amd import optimize as aopt
    sub = dict(prob, xyz=prob["xyz"][:n], uv=prob["uv"][:n])
    o = aopt.LsqOptimizer(*t_normal.frames(sub), dict(prob["init"]), weights=weights)
    o.set_target(prob["targets"])
    return o


def assert_close_fits(prob, p, cost, hp, hcost, what):
    """DESIGN's bounds between two runs of one problem: the final cost to 1e-8 relative, x to 1e-6 of the box width"""
    lower, upper = nc.bounds_of(prob, None)
    dx = max(abs(p[t] - hp[t]) / w for t, w in zip(prob["targets"], upper - lower))
    print("%s: cost %.15g against %.15g (rel %.3g), x within %.3g of the width" % (what, cost, hcost, cost / hcost - 1, dx))
    assert cost == pytest.approx(hcost, rel=1e-8)
    assert dx <= 1e-6


def test_a_device_loop_under_table_rows_against_the_host_lockstep(L):
    from alproj_amd import resample
    prob = t_lm.problem("trf_linear_d7")
    labels = resample.fold_labels(len(prob["xyz"]), 5, 3)
    host = lsq(prob).cross_validate(folds=labels)
    dev = lsq(prob).cross_validate(folds=labels, device_loop=True)
    for b in range(5):
        assert dev["fold_results"][b]["status"] in (1, 2, 3, 4) and host["fold_results"][b]["status"] in (1, 2, 3, 4)
        assert_close_fits(prob, dev["fold_params"][b], dev["fold_results"][b]["cost"], host["fold_params"][b], host["fold_results"][b]["cost"],
                          "fold %d" % b)
    assert dev["rmse"] == pytest.approx(host["rmse"], rel=1e-6)


# ---------------------------------------------------------------------------------------------------- 7. cross_validate
CV_SEED, SUBSET = 3, 200


@functools.lru_cache(maxsize=None)
def cv_run(n, folds=5):
    prob = t_lm.problem("trf_linear_d7")
    o = lsq(prob, n)
    return o, o.cross_validate(folds=folds, seed=CV_SEED)


@functools.lru_cache(maxsize=None)
def single_fit(n, row):
    """LsqOptimizer(weights=row).optimize(method="normal") on the first n points -> (params, cost, status)"""
    o = lsq(t_lm.problem("trf_linear_d7"), n, np.array(row))
    params, _ = o.optimize(method="normal")
    return params, o.result_["cost"], o.result_["status"]


@pytest.mark.parametrize("n", [SUBSET, None])
def test_cross_validate_folds_are_the_weighted_single_fits(L, n):
    from alproj_amd import resample
    prob = t_lm.problem("trf_linear_d7")
    N = len(prob["xyz"][:n])
    assert (N <= 256) == (n is not None)
    o, cv = cv_run(n)
    assert o.cv_ is cv and set(cv) == {"labels", "fold_params", "fold_results", "fold_rmse", "rmse", "residuals", "distance"}
    assert np.array_equal(cv["labels"], resample.fold_labels(N, 5, CV_SEED))
    train, held = resample.fold_tables(cv["labels"])
    assert cv["residuals"].shape == (N, 2) and cv["distance"].shape == (N,) and cv["fold_rmse"].shape == (5,)
    for b in range(5):
        params, cost, status = single_fit(n, tuple(train[b]))
        res = cv["fold_results"][b]
        assert set(res) == {"cost", "iterations", "evaluations", "status", "grad_norm"} and res["status"] in (1, 2, 3, 4)
        if N <= 256:        # one stripe either way: the same additions
            assert res["cost"] == cost and res["status"] == status
            assert all(cv["fold_params"][b][t] == params[t] for t in prob["targets"])
        else:
            assert_close_fits(prob, cv["fold_params"][b], res["cost"], params, cost, "fold %d" % b)


@pytest.mark.parametrize("n", [SUBSET, None])
def test_cross_validate_held_out_figures(L, n):
    from alproj_amd import optimize as aopt
    prob = t_lm.problem("trf_linear_d7")
    sub = dict(prob, xyz=prob["xyz"][:n], uv=prob["uv"][:n])
    obj, img = t_normal.frames(sub)
    _, cv = cv_run(n)
    N = len(obj)
    with t_lm.points_of(L, sub) as pts:        # the set cross_validate built: the same points about the same origin
        for b in range(5):
            mine = cv["labels"] == b
            same_origin = pts.residuals(L.params_vector(cv["fold_params"][b])).reshape(N, 2)
            assert np.array_equal(bits(cv["residuals"][mine]), bits(same_origin[mine]))
            # compute_residuals uploads the points about the FOLD's camera position (x, y, z are targets here), another rounding
            # of the same coordinates: float64 parity is stated to 1e-12 relative (optimize.project), pixels stay below 1e4
            r = aopt.compute_residuals(obj, img, cv["fold_params"][b]).reshape(N, 2)
            dist = np.hypot(r[:, 0], r[:, 1])
            print("fold %d: distance against compute_residuals, max deviation %.3g px (tol 1e-8)" % (b, np.abs(cv["distance"] - dist)[mine].max()))
            assert np.abs(cv["distance"] - dist)[mine].max() <= 1e-8
            assert np.array_equal(bits(cv["distance"][mine]), bits(np.hypot(same_origin[mine, 0], same_origin[mine, 1])))
            assert cv["fold_rmse"][b] == pytest.approx(np.sqrt((cv["residuals"][mine] ** 2).sum() / mine.sum()), rel=1e-12)
    pooled = np.sqrt((cv["residuals"] ** 2).sum() / N)
    print("pooled held-out rmse %.6f px; folds %s" % (cv["rmse"], np.round(cv["fold_rmse"], 4)))
    assert cv["rmse"] == pytest.approx(pooled, rel=1e-12)


def test_cross_validate_leave_one_out(L):
    _, cv = cv_run(12, "loo")
    assert len(cv["fold_params"]) == len(cv["fold_results"]) == 12 and cv["fold_rmse"].shape == (12,)
    assert np.array_equal(np.sort(cv["labels"]), np.arange(12))
    assert np.allclose(cv["fold_rmse"], cv["distance"][np.argsort(cv["labels"])], rtol=1e-12)    # one point per fold
    assert np.isfinite(cv["rmse"])


def test_cross_validate_folds_the_constructor_weights_into_the_table(L):
    from alproj_amd import resample
    prob = t_lm.problem("trf_linear_d7")
    w = np.random.default_rng(4).integers(0, 3, SUBSET).astype(np.float64)
    cv = lsq(prob, SUBSET, w).cross_validate(folds=4, seed=1)
    train, held = resample.fold_tables(resample.fold_labels(SUBSET, 4, 1), w)
    for b in range(4):
        params, cost, _ = single_fit(SUBSET, tuple(train[b]))
        assert cv["fold_results"][b]["cost"] == cost and all(cv["fold_params"][b][t] == params[t] for t in prob["targets"])
    d2 = (cv["residuals"] ** 2).sum(axis=1)
    assert cv["rmse"] == pytest.approx(np.sqrt((w * d2).sum() / w.sum()), rel=1e-12)


# ---------------------------------------------------------------------------------------------------- 8. bootstrap
BOOT_SEED = 11        # with the first 200 points of trf_linear_d7: scipy's trf on the oracle (complex-step Jacobian, the repeated
#                       rows, tolerances 1e-12) converges for every one of the 16 rows, status 3 after 6 evaluations, no variable on a bound


@pytest.mark.parametrize("n", [SUBSET, None])
def test_bootstrap_samples_are_the_weighted_single_fits(L, n):
    from alproj_amd import resample
    prob = t_lm.problem("trf_linear_d7")
    N = len(prob["xyz"][:n])
    o = lsq(prob, n)
    boot = o.bootstrap(n_boot=16, seed=BOOT_SEED)
    assert o.boot_ is boot
    assert {"samples", "mean", "std", "cov", "interval", "results", "counts", "dropped"} <= set(boot)
    assert np.array_equal(boot["counts"], resample.bootstrap_table(N, 16, BOOT_SEED)) and (boot["counts"].sum(axis=1) == N).all()
    assert boot["samples"].shape == (16, 7) and len(boot["results"]) == 16
    print("statuses", [r["status"] for r in boot["results"]], "dropped", boot["dropped"])
    assert boot["dropped"] == 0 and boot["kept"].all()
    for b in range(16):
        params, cost, status = single_fit(n, tuple(boot["counts"][b]))
        got = dict(zip(prob["targets"], boot["samples"][b]))
        if N <= 256:
            assert boot["results"][b]["cost"] == cost and boot["results"][b]["status"] == status
            assert all(got[t] == params[t] for t in prob["targets"])
        else:
            assert_close_fits(prob, got, boot["results"][b]["cost"], params, cost, "resample %d" % b)
    assert np.array_equal(boot["cov"], np.cov(boot["samples"], rowvar=False))
    assert np.array_equal(boot["mean"], boot["samples"].mean(axis=0)) and np.array_equal(boot["std"], boot["samples"].std(axis=0, ddof=1))
    lo, hi = boot["interval"](0.9)
    # (50 (1 - 0.9) is not 5 to the last bit, and numpy interpolates between two samples at the fraction it is given)
    np.testing.assert_allclose(lo, np.percentile(boot["samples"], 5, axis=0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(hi, np.percentile(boot["samples"], 95, axis=0), rtol=1e-12, atol=0)
    assert (lo <= boot["mean"]).all() and (boot["mean"] <= hi).all() and (boot["std"] > 0).all()


def test_bootstrap_reports_what_it_drops(L):
    """max_nfev = 1 stops every fit at its first evaluation with status 0: all dropped, and the statistics say so"""
    boot = lsq(t_lm.problem("trf_linear_d7"), SUBSET).bootstrap(n_boot=4, seed=BOOT_SEED, max_nfev=1)
    assert boot["dropped"] == 4 and not boot["kept"].any()
    assert np.isnan(boot["mean"]).all() and np.isnan(boot["cov"]).all() and np.isnan(boot["interval"]()[0]).all()
    assert [r["status"] for r in boot["results"]] == [0] * 4


# ---------------------------------------------------------------------------------------------------- 9. a communicator of one
def test_world_1_communicator_gives_the_same_bits(L):
    _, before = cv_run(SUBSET)
    L.comm_init(L.comm_unique_id(), 0, 1)
    try:
        assert L.comm_info() == (0, 1)
        during = lsq(t_lm.problem("trf_linear_d7"), SUBSET).cross_validate(folds=5, seed=CV_SEED)
    finally:
        L.comm_destroy()
    for key in ("labels", "fold_rmse", "residuals", "distance"):
        assert np.array_equal(bits(before[key]), bits(during[key])), key
    assert before["rmse"] == during["rmse"] and before["fold_params"] == during["fold_params"]
    assert before["fold_results"] == during["fold_results"]
