"""GPU: per-point frequency weights (alp_points_set_weights) in the population losses, the normal equations and the optimisers.

The oracle is the unweighted one on ROW-DUPLICATED tables: for integer weights "weight w_i" means "row i appears w_i times"
(np.repeat; a row of weight 0 is absent).  tests/golden/g20_weighted.npz holds what the reference itself returned on such
tables.  No tolerance is stated here that an unweighted test of the same path does not state: they are imported."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest

from oracle import ref_numpy as orc
from tests import lm_device_cases as lc
from tests import mend_cases as mc
from tests import normal_cases as nc
from tests import popeval_cases as pc
from tests import test_gpu_cma_device as t_cma
from tests import test_gpu_mend as t_mend
from tests import test_gpu_normal as t_normal
from tests import test_gpu_points as t_points
from tests import test_gpu_popeval_grid as t_grid
from tests.test_jacobian_oracle import KEYS, TARGETS

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
EINVAL, ESTATE = -1, -6
I32 = ctypes.POINTER(ctypes.c_int32)


def marks_of(fn, first):
    """the argvalues of the parametrize mark of test function `fn` whose argnames begin with `first`"""
    return [m.args[1] for m in fn.pytestmark if m.name == "parametrize" and m.args[0].split(",")[0] == first][0]


# float64 rtol of tests/test_gpu_points.py for g19 (the reference's own losses, lens-free) and g5 (with a lens)
F64_RTOL_G19 = dict(marks_of(t_points.test_first_phase_population_golden, "prec"))["f64"]
F64_RTOL_G5 = dict(marks_of(t_points.test_population_golden, "prec"))["f64"]
# test_population_lens_free_variant's variant-to-variant margins (the order of the additions alone differs): its rtol_general
REASSOC_RTOL = {prec: rtol_general for prec, _, rtol_general in marks_of(t_points.test_population_lens_free_variant, "prec")}
assert (F64_RTOL_G19, F64_RTOL_G5, REASSOC_RTOL) == (1e-9, 1e-8, {"f64": 1e-12, "f32": 2e-6})


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def dup(a, w):
    return np.repeat(np.asarray(a), np.asarray(w).astype(np.int64), axis=0)


def points(L, xyz, uv, o, prec, w=None):
    pts = L.Points(xyz, o, prec)
    pts.set_observed(uv)
    if w is not None:
        pts.set_weights(w)
    return pts


def force_grid(monkeypatch, stripes, cols=1):
    monkeypatch.setenv("ALP_POP_GRID", f"{stripes},{cols}")


# ---------------------------------------------------------------------------------------------------- 1. parity with g20
@pytest.fixture(scope="module")
def g20():
    return np.load(os.path.join(G, "g20_weighted.npz"), allow_pickle=False)


G20_VARIANT = {"lf": "lens_free", "gen": "general", "sp": "shared_pose"}


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", list(G20_VARIANT))
def test_g20_parity_with_the_reference_on_duplicated_rows(L, g20, name, prec):
    init = orc.vector_to_params(g20[f"{name}_params_init"])
    tgt = [str(t) for t in g20[f"{name}_targets"]]
    cand = t_points._cand_matrix(L, init, tgt, g20[f"{name}_bounds"], g20[f"{name}_X"])
    w = g20["weights"]
    assert set(np.unique(w)) == {0.0, 1.0, 2.0, 3.0} and (w == 0).sum() > len(w) // 8
    with points(L, g20["xyz"], g20["uv_obs"], [init["x"], init["y"], init["z"]], prec, w) as pts:
        assert pts.weight_sum() == w.sum()
        for tag, kind, fs in (("md", L.LOSS_MEAN_DIST, 0.0), ("hub", L.LOSS_HUBER, 10.0)):
            losses, amin = pts.eval_population(cand, kind, fs)
            assert pts.eval_population_info()[0] == G20_VARIANT[name]
            ref = g20[f"{name}_{tag}"]
            print(f"[g20] {name} {prec} {tag}: max rel {np.abs(losses / ref - 1).max():.3e}")
            if prec == "f64":
                np.testing.assert_allclose(losses, ref, rtol=F64_RTOL_G19 if name == "lf" else F64_RTOL_G5)
            else:
                tol = t_points.f32_loss_tolerance(g20["xyz"], cand)
                assert np.all(np.abs(losses - ref) <= tol * np.abs(ref)), np.abs(losses / ref - 1).max()
                t_points.assert_f32_close(losses, ref, float(init["w"]), f"g20 {name} {tag}")
            assert amin == int(np.argmin(ref))
            assert losses[3] == losses[7]


# ---------------------------------------------------------------------------------------------------- shared inputs
@pytest.fixture(scope="module")
def cases(L):
    """popeval_cases' 67-row set, integer weights 0..3, 130 candidates per variant, and the oracle's per-point distances"""
    xyz, uv = pc.point_set()
    w = np.random.default_rng(20).integers(0, 4, len(xyz)).astype(np.float64)
    pops = {v: pc.population(v, 130) for v in pc.VARIANTS}
    dist = {}
    for v in pc.VARIANTS:
        d = np.empty((2, len(xyz)))
        for i in range(2):
            prj = orc.project_points(xyz, orc.vector_to_params(pops[v][i]))
            d[i] = ((uv[:, 0] - prj[:, 0]) ** 2 + (uv[:, 1] - prj[:, 1]) ** 2) ** 0.5
        dist[v] = d
    return dict(xyz=xyz, uv=uv, o=pc.origin(), w=w, pops=pops, dist=dist)


# ---------------------------------------------------------------------------------------------------- 2. unit weights
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_unit_weights_change_no_bit_of_the_losses(L, cases, variant, prec, monkeypatch):
    cand = cases["pops"][variant]
    n = len(cases["xyz"])
    with points(L, cases["xyz"], cases["uv"], cases["o"], prec) as pts:
        assert pts.weight_sum() == n
        for stripes in (1, 7, 1000):
            force_grid(monkeypatch, stripes)
            for kind, fs in pc.LOSSES.values():
                pts.set_weights(None)
                plain = pts.eval_population(cand, kind, fs)
                assert pts.eval_population_info()[0] == variant
                pts.set_weights(np.ones(n, dtype=np.float32 if stripes == 7 else np.float64))
                assert pts.weight_sum() == n
                unit = pts.eval_population(cand, kind, fs)
                assert pts.eval_population_info()[0] == variant
                pts.set_weights(None)
                assert pts.weight_sum() == n
                again = pts.eval_population(cand, kind, fs)
                for got in (unit, again):
                    assert np.array_equal(bits(got[0]), bits(plain[0])) and got[1] == plain[1], (stripes, kind)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("loss", nc.LOSSES)
def test_unit_weights_change_no_bit_of_the_normal_equations(L, loss, prec):
    xyz, uv, p = t_normal.synthetic(70_001, seed=9)
    pv = L.params_vector(p)
    cand = np.tile(pv, (3, 1))
    cand[:, KEYS.index("pan")] += [0.0, 0.01, -0.02]
    with points(L, xyz, uv, [p["x"], p["y"], p["z"]], prec) as pts:
        plain = pts.normal_equations(pv, t_normal.idx(TARGETS), loss, 1.5), pts.normal_equations_batch(cand, t_normal.idx(TARGETS), loss, 1.5)
        pts.set_weights(np.ones(len(xyz)))
        unit = pts.normal_equations(pv, t_normal.idx(TARGETS), loss, 1.5), pts.normal_equations_batch(cand, t_normal.idx(TARGETS), loss, 1.5)
        pts.set_weights(None)
        again = pts.normal_equations(pv, t_normal.idx(TARGETS), loss, 1.5), pts.normal_equations_batch(cand, t_normal.idx(TARGETS), loss, 1.5)
    for got in (unit, again):
        for a, b in zip(plain, got):
            for x, y in zip(a[:3], b[:3]):
                assert np.array_equal(bits(x), bits(y))
            assert a[3] == b[3] == 70_001
    assert isinstance(unit[0][3], float) and isinstance(plain[0][3], int)


# ---------------------------------------------------------------------------------------------------- 3. device against device
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_weighted_set_against_the_duplicated_set_on_every_grid(L, cases, variant, prec, monkeypatch):
    """the two sets differ in n, so in the order of the additions alone"""
    w = cases["w"]
    worst = 0.0
    with points(L, cases["xyz"], cases["uv"], cases["o"], prec, w) as wp, \
            points(L, dup(cases["xyz"], w), dup(cases["uv"], w), cases["o"], prec) as dp:
        assert wp.weight_sum() == dp.n == w.sum()
        for stripes in t_grid.GRIDS:
            force_grid(monkeypatch, stripes)
            for P in (1, 130):
                cand = cases["pops"][variant][:P]
                for kind, fs in pc.LOSSES.values():
                    got, _ = wp.eval_population(cand, kind, fs, want_argmin=False)
                    info = wp.eval_population_info()
                    assert info[0] == t_grid.expected_variant(variant, P) and info[1] == min(stripes, pc.N_ROWS)
                    ref, _ = dp.eval_population(cand, kind, fs, want_argmin=False)
                    assert dp.eval_population_info()[0] == info[0]
                    worst = max(worst, float(np.abs(got / ref - 1).max()))
                    np.testing.assert_allclose(got, ref, rtol=REASSOC_RTOL[prec], atol=0, err_msg=f"{stripes} stripes, P = {P}")
    print(f"[weighted vs duplicated] {variant} {prec}: worst rel {worst:.3e} (tol {REASSOC_RTOL[prec]:.1e})")


# ---------------------------------------------------------------------------------------------------- 4. seams
HEAVY = 1000.0


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_one_heavy_weight_at_every_seam(L, cases, variant, prec, monkeypatch):
    """weight 1000 on one point, 1 elsewhere: the mean distance moves by that point's oracle term, 999 d_k -- a weight read at
    another index moves it by 999 d_j instead (a relative 0.06 |d_k - d_j| of the loss, against tolerances of 1e-10 and 1e-5)"""
    cand = cases["pops"][variant][:2]
    d = cases["dist"][variant]
    n = d.shape[1]
    kind, fs = pc.LOSSES["mean_dist"]
    tol = np.full(2, t_grid.F64_RTOL) if prec == "f64" else t_points.f32_loss_tolerance(cases["xyz"], cand)
    V = pc.GROUP_ROWS[(variant, prec)]
    checked = 0
    with points(L, cases["xyz"], cases["uv"], cases["o"], prec) as pts:
        for stripes in (1, 5, 23, 67):
            force_grid(monkeypatch, stripes)
            marks = pc.mark_positions(stripes, V)
            for k in marks:
                w = np.ones(n)
                w[k] = HEAVY
                pts.set_weights(w)
                got, _ = pts.eval_population(cand, kind, fs, want_argmin=False)
                assert pts.eval_population_info()[0] == variant
                ref = (d.sum(axis=1) + (HEAVY - 1.0) * d[:, k]) / (n + HEAVY - 1.0)
                assert np.all(np.abs(got - ref) <= tol * ref), (stripes, k, got, ref)
                checked += 1
    assert checked > 200


# ---------------------------------------------------------------------------------------------------- 5. zero weight
def poisoned_set(t, n=2 * 256 + 100):
    """n GCP-like points and, behind them, a vertex AT the camera of pose t and one ON its camera plane (same 256-row)"""
    from alproj_amd import synthetic as syn
    xyz = syn.gcp_points(n, t, seed=21)
    uv = orc.project_points(xyz, t) + np.random.default_rng(21).normal(0, 1.0, (n, 2))
    cam = np.array([t["x"], t["y"], t["z"]])
    rot = orc.extrinsic_mat(t["pan"], t["tilt"], t["roll"], 0.0, 0.0, 0.0)[:3, :3]
    on_plane = cam + np.array([300.0, 100.0, 0.0]) @ rot
    return np.vstack([xyz, cam, on_plane]), np.vstack([uv, [[100.0, 100.0], [900.0, 700.0]]])


def same_camera_population(L, variant, t):
    """candidates that all keep t's camera position and orientation (the planted vertices poison every one of them)"""
    base = L.params_vector(t)
    cand = np.tile(base, (5, 1))
    if variant == "shared_pose":
        cand[:, 9:21] *= 1.0 + np.linspace(-0.01, 0.01, 5)[:, None]
    else:
        cand[:, L.PARAM_KEYS.index("fov")] += np.linspace(-1.0, 1.0, 5)
    return cand


@pytest.mark.parametrize("variant,prec", [("general", "f64"), ("shared_pose", "f64"), ("lens_free", "f64"), ("lens_free", "f32"),
                                          ("general", "f32")])
def test_zero_weight_removes_a_poisoned_point(L, variant, prec):
    t = pc.truth(variant)
    xyz, uv = poisoned_set(t)
    n = len(xyz) - 2
    o = pc.origin()
    cand = same_camera_population(L, variant, t)
    rng = np.random.default_rng(5)
    w = rng.integers(1, 4, len(xyz)).astype(np.float64)
    with points(L, xyz, uv, o, prec) as pts, points(L, xyz[:n], uv[:n], o, prec, w[:n]) as clean:
        for kind, fs in pc.LOSSES.values():
            ref, ref_amin = clean.eval_population(cand, kind, fs)
            assert clean.eval_population_info()[0] == variant and np.isfinite(ref).all()
            w[n:] = 0.0
            pts.set_weights(w)
            got, amin = pts.eval_population(cand, kind, fs)
            assert pts.eval_population_info()[0] == variant
            np.testing.assert_allclose(got, ref, rtol=REASSOC_RTOL[prec], atol=0)
            assert amin == ref_amin
            for k in (n, n + 1):             # either vertex at weight 1 poisons every sum, as it does today: the vertex at the
                w[n:] = 0.0                  # camera is NaN; the one on the camera plane +-inf, NaN, or -- where the device's
                w[k] = 1.0                   # depth comes out as an ulp instead of 0 -- a distance beyond any image
                pts.set_weights(w)
                bad, _ = pts.eval_population(cand, kind, fs, want_argmin=False)
                if k == n:
                    assert np.isnan(bad).all(), bad
                else:
                    assert (~np.isfinite(bad) | (bad > 1e6 * ref)).all(), (bad, ref)
            pts.set_weights(None)
            bad, _ = pts.eval_population(cand, kind, fs, want_argmin=False)
            assert np.isnan(bad).all()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_zero_weight_in_the_second_walk_of_a_lens_free_tile(L, prec):
    """a2 = -1 puts every point of a lens-free candidate on the pole of the y ratio: its sum is +inf, through the second walk
    (the general arithmetic).  The vertex at the camera would turn it into NaN there; at weight 0 it must not."""
    t = pc.truth("lens_free")
    xyz, uv = poisoned_set(t)
    n = len(xyz) - 2
    cand = same_camera_population(L, "lens_free", t)
    cand[1, L.PARAM_KEYS.index("a2")] = -1.0
    cand[3, L.PARAM_KEYS.index("a2")] = -1.0
    w = np.ones(len(xyz))
    w[n:] = 0.0
    with points(L, xyz, uv, pc.origin(), prec, w) as pts:
        for kind, fs in pc.LOSSES.values():
            got, amin = pts.eval_population(cand, kind, fs)
            assert pts.eval_population_info()[0] == "lens_free"
            assert np.isposinf(got[[1, 3]]).all() and np.isfinite(got[[0, 2, 4]]).all(), got
            assert amin in (0, 2, 4)
            w[n] = 1.0
            pts.set_weights(w)
            bad, _ = pts.eval_population(cand, kind, fs, want_argmin=False)
            assert np.isnan(bad).all()
            w[n] = 0.0
            pts.set_weights(w)


@pytest.mark.parametrize("variant", ["general", "shared_pose"])
def test_zero_weight_in_the_second_walk_of_a_float64_tile(L, variant, monkeypatch):
    """test_gpu_popeval_grid's pole vertices at weight 2 and, at weight 0, a vertex at the camera of the pole candidates: a
    candidate the device puts exactly on a pole is +inf through the second walk (a reciprocal per denominator), and would be NaN
    if that walk counted the vertex at the camera"""
    V = pc.GROUP_ROWS[(variant, "f64")]
    xyz, uv, o, nan_at, pole_at, _ = t_grid.second_walk_set(V)
    t = dict(pc.truth("general"), k4=t_grid.POLE_K4, k5=0.0, k6=0.0)
    xyz = np.vstack([xyz, [[t["x"], t["y"], t["z"]]]])
    uv = np.vstack([uv, [[100.0, 100.0]]])
    w = np.ones(len(xyz))
    w[list(pole_at)] = 2.0
    w[-1] = 0.0
    kind, fs = pc.LOSSES["mean_dist"] if variant != "shared_pose" else pc.LOSSES["huber"]
    with points(L, xyz, uv, o, "f64", w) as pts:
        dev, _ = t_grid.pole_candidates(L, pts, monkeypatch, xyz, o, pole_at, "f64", variant, kind, fs)
        cand = np.array(dev + [L.params_vector(t)])
        if variant == "general":          # candidates that differ in a2 alone are the shared-pose variant: one other pan
            cand = np.vstack([cand, L.params_vector(dict(t, pan=t["pan"] + 0.5))])
        got, _ = pts.eval_population(cand, kind, fs, want_argmin=False)
        assert pts.eval_population_info()[0] == variant
        assert np.isposinf(got[:len(dev)]).all() and np.isfinite(got[len(dev):]).all(), got
        w[-1] = 1.0
        pts.set_weights(w)
        bad, _ = pts.eval_population(cand, kind, fs, want_argmin=False)
        assert np.isnan(bad).all(), bad


@pytest.mark.parametrize("loss", nc.LOSSES)
def test_zero_weight_removes_a_poisoned_point_from_the_normal_equations(L, loss):
    t = pc.truth("general")
    xyz, uv = poisoned_set(t)
    n = len(xyz) - 2
    pv = L.params_vector(t)
    cols = t_normal.idx(TARGETS)
    w = np.random.default_rng(6).integers(1, 4, len(xyz)).astype(np.float64)
    with points(L, xyz, uv, pc.origin(), "f64") as pts, points(L, xyz[:n], uv[:n], pc.origin(), "f64", w[:n]) as clean:
        ref = clean.normal_equations(pv, cols, loss, 2.0)
        w[n:] = 0.0
        pts.set_weights(w)
        got = pts.normal_equations(pv, cols, loss, 2.0)
        for a, b in zip(got, ref):          # the same rows in the same groups, and exact zeros behind them
            assert np.array_equal(bits(a), bits(b))
        got_b = pts.normal_equations_batch(np.tile(pv, (2, 1)), cols, loss, 2.0)
        assert np.isfinite(got_b[0]).all() and np.isfinite(got_b[1]).all() and np.isfinite(got_b[2]).all()
        w[n] = 1.0
        pts.set_weights(w)
        bad = pts.normal_equations(pv, cols, loss, 2.0)
        assert not np.isfinite(bad[0]).all() or not np.isfinite(bad[2])


# ---------------------------------------------------------------------------------------------------- 6. normal equations
D_TARGETS = {1: ["pan"], 16: TARGETS[7:23], 17: TARGETS[3:20], 23: TARGETS}


def weighted_normal_case(n, seed):
    xyz, uv, p = t_normal.synthetic(n, seed=seed)
    w = np.random.default_rng(seed).integers(0, 4, n).astype(np.float64)
    return xyz, uv, p, w


def kink_free_scale(xyz, uv, p):
    """f_scale near the median |residual| (half the rows on either branch of huber, as test_gpu_normal.median_scale wants), put
    in the MIDDLE OF THE WIDEST GAP between consecutive sorted |residuals| of the middle fifth.  Huber's row scaling s drops from 1
    to 1e-5 at |r| = f_scale, and a float32 set knows a residual to about 1e-3 px: the plain median leaves the nearest residual
    half an average gap away (5e-5 px on this set), where the float32 set and the float64 oracle put a row on different
    branches -- a property of the inputs, not of the sums under test.  The gap chosen is asserted to be >= 8e-3 px wide."""
    r = np.sort(np.abs(nc.residual_vector(xyz, uv, orc.params_to_vector(p))))
    lo, hi = int(0.4 * len(r)), int(0.6 * len(r))
    k = lo + int(np.argmax(np.diff(r[lo:hi])))
    assert r[k + 1] - r[k] >= 8e-3
    fs = 0.5 * float(r[k] + r[k + 1])
    assert (r <= fs).sum() > len(r) // 4 and (r > fs).sum() > len(r) // 4
    return fs


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("loss", nc.LOSSES)
@pytest.mark.parametrize("D", list(D_TARGETS))
def test_normal_equations_against_the_oracle_on_duplicated_rows(L, D, loss, precision):
    targets = D_TARGETS[D]
    assert len(targets) == D
    xyz, uv, p, w = weighted_normal_case(900, 4)
    fs = kink_free_scale(xyz, uv, p)
    pv = L.params_vector(p)
    ref = nc.normal_oracle(dup(xyz, w), dup(uv, w), orc.params_to_vector(p), targets, loss, fs)
    cand = np.tile(pv, (3, 1))
    with points(L, xyz, uv, [p["x"], p["y"], p["z"]], precision, w) as pts:
        got = pts.normal_equations(pv, t_normal.idx(targets), loss, fs)
        assert isinstance(got[3], float) and got[3] == w.sum() == pts.weight_sum()
        nc.assert_sums_close(got, ref, *t_normal.TOL[precision])
        Gb, gb, cb, nb_ = pts.normal_equations_batch(cand, t_normal.idx(targets), loss, fs)
        assert nb_ == w.sum()
        for b in range(3):
            nc.assert_sums_close((Gb[b], gb[b], float(cb[b]), nb_), ref, *t_normal.TOL[precision])


@pytest.mark.parametrize("n,D", [(1, 17), (255, 23), (256, 16), (257, 23), (4095, 17), (400_003, 1)])
def test_normal_equations_launch_shapes(L, n, D):
    """n on both sides of one 256-point group and, at 400 003 points, two groups per stripe of normal_grid"""
    targets = D_TARGETS[D]
    xyz, uv, p, w = weighted_normal_case(n, n)
    w[0] = 2.0
    if n > 100_000:
        assert nc.normal_grid(n, L.device_info()["cu_count"])[1] >= 2
    pv = L.params_vector(p)
    ref = nc.normal_oracle(dup(xyz, w), dup(uv, w), orc.params_to_vector(p), targets, "soft_l1", 2.0)
    with points(L, xyz, uv, [p["x"], p["y"], p["z"]], "f64", w) as pts:
        got = pts.normal_equations(pv, t_normal.idx(targets), "soft_l1", 2.0)
        nc.assert_sums_close(got, ref, *t_normal.TOL["f64"])
        Gb, gb, cb, nb_ = pts.normal_equations_batch(np.tile(pv, (2, 1)), t_normal.idx(targets), "soft_l1", 2.0)
        nc.assert_sums_close((Gb[1], gb[1], float(cb[1]), nb_), ref, *t_normal.TOL["f64"])


@pytest.mark.parametrize("n", [None, 257])
def test_the_listed_kernel_of_the_device_loop_on_a_weighted_set(L, n):
    """tests/test_gpu_lm_device.py::test_the_evaluation_inside_the_loop_is_the_batch_call on a weighted set: one handle runs a
    round (normal_poses_kernel given the list), its twin is stepped on alp_normal_equations_batch's sums at the same trial points"""
    from tests import test_gpu_lm_device as t_lm
    prob = t_lm.problem("trf_linear_d7")
    K = 3
    X0, lower, upper = t_lm.starts_of(prob, K)
    targets = t_normal.idx(prob["targets"])
    tp = np.array(targets, dtype=np.int32)
    D = len(targets)
    tmpl = L.params_vector(prob["init"])
    with t_lm.points_of(L, prob, n) as pts:
        w = np.random.default_rng(8).integers(0, 4, pts.n).astype(np.float64)
        pts.set_weights(w)
        with L.LmDevice(pts, tmpl, targets, lower, upper, X0) as a, L.LmDevice(pts, tmpl, targets, lower, upper, X0) as b:
            for rnd in range(3):
                trial = b.get()["trial"]
                cand = np.tile(tmpl, (K, 1))
                cand[:, targets] = trial
                raw = np.empty((K, D * (D + 1) // 2 + D + 2))
                assert L.lib().alp_normal_equations_batch(pts._h, L.as_dp(cand), K, tp.ctypes.data_as(I32), D, 0, 1.0, L.as_dp(raw)) == 0
                assert (raw[:, -1] == w.sum()).all()
                a.run(1)
                with pytest.raises(RuntimeError) as e:          # 9: rounds are pending
                    pts.set_weights(w)
                assert e.value.code == ESTATE
                a.wait()
                b.step_host(raw)
                ra, rb = a.get(), b.get()
                dev = float(np.max(np.abs(ra["trial"] - rb["trial"]) / (upper - lower)))
                rel = lambda u, v: float(np.max(np.abs(u - v) / np.abs(v)))
                assert dev <= lc.TRIAL_TOL and rel(ra["cost"], rb["cost"]) <= lc.TRIAL_TOL and rel(ra["mu"], rb["mu"]) <= lc.TRIAL_TOL
                np.testing.assert_array_equal(ra["status"], rb["status"])
        # the cost of the first trial point is the duplicated set's
        ref = nc.normal_oracle(dup(prob["xyz"][:n], w), dup(prob["uv"][:n], w), np.array([prob["init"][k] for k in KEYS]), prob["targets"])
        got = pts.normal_equations(tmpl, targets)
        nc.assert_sums_close(got, ref, *t_normal.TOL["f64"])


# ---------------------------------------------------------------------------------------------------- 7. mend and confirmation
@pytest.mark.parametrize("loss", ["mean_dist", "huber"])
@pytest.mark.parametrize("variant", mc.VARIANTS)
def test_mended_losses_are_the_weighted_float64_losses(L, variant, loss):
    xyz, uv = mc.scene()
    w = np.random.default_rng(12).integers(0, 4, len(xyz)).astype(np.float64)
    w[-2:] = [2.0, 3.0]                        # the planted vertices count: they are what overflows float32
    tame, wild = mc.populations(variant)
    flagged = mc.flagged_sets()["tile_plus_one"]
    cand = mc.mix(tame, wild, flagged)
    ref = mc.mix_losses(mc.oracle(dup(xyz, w), dup(uv, w), tame), mc.oracle(dup(xyz, w), dup(uv, w), wild), flagged)[loss]
    assert mc.argmin_margin(ref)[1] >= mc.MARGIN[(variant, False)]
    with points(L, xyz, uv, mc.ORIGIN, "f32", w) as pts:
        info = t_mend._check_mended(L, pts, cand, flagged, ref, loss, variant)
        assert info[0] == len(flagged)


def test_near_tie_confirmation_on_a_weighted_set(L, g20):
    """candidate 5 is given the winner's parameters with the pan moved by 1e-9 degrees: float32 cannot order the two, so the
    float64 confirmation runs -- on the weighted set -- and picks the one a float64 set of the same weights ranks first"""
    init = orc.vector_to_params(g20["gen_params_init"])
    tgt = [str(t) for t in g20["gen_targets"]]
    cand = t_points._cand_matrix(L, init, tgt, g20["gen_bounds"], g20["gen_X"])
    ref = g20["gen_md"]
    best = int(np.argmin(ref))
    near = cand[best].copy()
    near[L.PARAM_KEYS.index("pan")] += 1e-9          # a loss within float32's noise of the winner's, larger in float64 or equal
    cand[5] = near
    w = g20["weights"]
    o = [init["x"], init["y"], init["z"]]
    with points(L, g20["xyz"], g20["uv_obs"], o, "f32", w) as p32, points(L, g20["xyz"], g20["uv_obs"], o, "f64", w) as p64:
        l32, a32 = p32.eval_population(cand, L.LOSS_MEAN_DIST, 0.0)
        l64, a64 = p64.eval_population(cand, L.LOSS_MEAN_DIST, 0.0)
    assert abs(l32[5] / l32[best] - 1) < 1e-6
    assert a32 in (5, best) and l64[a32] <= l64[[5, best]].min() * (1 + 1e-12)


# ---------------------------------------------------------------------------------------------------- 8. optimisers
@pytest.fixture(scope="module")
def lsq_problem():
    """g14's trf_linear_d7 with integer weights; `dup`: the same problem with its rows duplicated, whose optimum scipy's trf
    finds on the oracle (complex-step Jacobian, tolerances 1e-12)"""
    prob = nc.g14_problem("trf_linear_d7")
    w = np.random.default_rng(14).integers(0, 4, len(prob["xyz"])).astype(np.float64)
    d = dict(prob, xyz=dup(prob["xyz"], w), uv=dup(prob["uv"], w))
    lower, upper = nc.bounds_of(prob, None)
    x, _ = nc.scipy_trf_on_the_oracle(d, lower, upper)
    want = dict(prob["init"])
    want.update(dict(zip(prob["targets"], x)))
    d["want"] = want
    d["error"] = nc.mean_distance(d, want)
    return prob, w, d


def weighted_lsq(prob, w):
    from alproj_amd import optimize as aopt
    o = aopt.LsqOptimizer(*t_normal.frames(prob), dict(prob["init"]), weights=w)
    o.set_target(prob["targets"])
    return o


@pytest.mark.parametrize("how", ["host", "starts", "device_loop"])
def test_optimize_normal_with_weights_reaches_the_optimum_of_the_duplicated_problem(L, lsq_problem, how):
    prob, w, d = lsq_problem
    kw = {"host": {}, "starts": dict(starts=4, seed=1), "device_loop": dict(device_loop=True)}[how]
    o = weighted_lsq(prob, w)
    params, err = o.optimize(method="normal", **kw)
    print(how, o.result_)
    assert o.result_["status"] in (1, 2, 3, 4)
    assert o.result_["cost"] == pytest.approx(nc.cost_at(d, params), rel=1e-9)
    assert err == pytest.approx(nc.mean_distance(d, params), rel=1e-9)
    nc.assert_reference_optimum(d, params, err, o.result_["cost"], "linear", 1.0)


@pytest.mark.parametrize("loss,f_scale", [("soft_l1", 3.0), ("huber", 5.0), ("cauchy", 2.0)])
def test_optimize_normal_with_weights_and_a_robust_loss(L, lsq_problem, loss, f_scale):
    """against the same optimiser on the physically duplicated rows"""
    from alproj_amd import optimize as aopt
    prob, w, d = lsq_problem
    o = weighted_lsq(prob, w)
    params, err = o.optimize(method="normal", loss=loss, f_scale=f_scale)
    r = aopt.LsqOptimizer(*t_normal.frames(d), dict(prob["init"]))
    r.set_target(prob["targets"])
    rp, rerr = r.optimize(method="normal", loss=loss, f_scale=f_scale)
    assert o.result_["cost"] == pytest.approx(nc.cost_at(d, params, loss, f_scale), rel=1e-9)
    assert o.result_["cost"] == pytest.approx(r.result_["cost"], rel=1e-8)       # test_optimize_device_loop_with_eight_starts' margin between two runs
    for k in prob["targets"]:
        assert abs(params[k] - rp[k]) <= (2e-4 if k in nc.POSE_KEYS else 2e-6), (k, params[k], rp[k])
    assert err == pytest.approx(rerr, rel=5e-5)


@pytest.mark.parametrize("jac", ["batched", "analytic"])
def test_trf_linear_with_weights(L, lsq_problem, jac):
    prob, w, d = lsq_problem
    o = weighted_lsq(prob, w)
    params, err = o.optimize(method="trf", loss="linear", jac=jac)
    # the limits of tests/test_gpu_golden_render.py::test_g14_lsq_optimizer_matches_the_reference_run (scipy stops at ftol = 1e-8)
    for k in prob["targets"]:
        tol = 2e-4 if k in nc.POSE_KEYS else 2e-6
        assert abs(params[k] - d["want"][k]) <= tol, (jac, k, params[k], d["want"][k])
    assert abs(err - d["error"]) <= 5e-5 * d["error"], (err, d["error"])
    assert err == pytest.approx(nc.mean_distance(d, params), rel=1e-9)
    with pytest.raises(ValueError, match="method='normal'"):
        o.optimize(method="trf", loss="huber", f_scale=5.0)
    with pytest.raises(ValueError, match="method='normal'"):
        o.optimize(method="dogbox", loss="soft_l1")


@pytest.mark.parametrize("variant,targets,precision,lens_free_start", t_cma.VARIANT_CASES)
def test_cma_device_generations_on_a_weighted_set(L, variant, targets, precision, lens_free_start):
    """tests/test_gpu_cma_device.py::test_generations_match_the_host_path on a weighted set: the device loop's losses are the
    host path's on the same set, and those of the duplicated rows"""
    from alproj_amd import synthetic as syn
    from alproj_amd.optimize import CMAOptimizer, bounds_to_array
    obj, img, init = t_cma._gcp_problem()
    if lens_free_start:
        init = dict(init, **{k: 0.0 for k in syn.TARGETS_D21[9:]})
    w = np.random.default_rng(15).integers(0, 4, len(obj)).astype(np.float64)
    opt = CMAOptimizer(obj, img, init, weights=w)
    opt.set_target(list(targets))
    ref_opt = CMAOptimizer(pd.DataFrame(dup(obj.to_numpy(), w), columns=obj.columns), pd.DataFrame(dup(img.to_numpy(), w), columns=img.columns), init)
    ref_opt.set_target(list(targets))
    D, P = len(targets), 50
    b = bounds_to_array(init, targets)
    lo, hi = b[:, 0], b[:, 1]
    host = t_cma._host_cma(D, P, 11)
    host.set_state(dict(host.get_state(), mean=(opt.target_params_init - lo) / (hi - lo), sigma=0.2))
    with opt._device_points(precision) as pts, ref_opt._device_points(precision) as dpts:
        assert pts.weight_sum() == dpts.n == w.sum()
        with L.CmaDevice(pts, L.params_vector(init), [L.PARAM_KEYS.index(t) for t in targets], lo, hi, host) as loop:
            loop.set_state(host.get_state())
            for g in (0, 1, 2):
                loop.run(1, L.LOSS_HUBER, 10.0)
                with pytest.raises(RuntimeError) as e:          # 9: a generation is pending
                    pts.set_weights(w)
                assert e.value.code == ESTATE
                loop.wait()
                assert pts.eval_population_info()[0] == variant
                X, cand, losses = loop.fetch_last()
                want, _ = pts.eval_population(cand, L.LOSS_HUBER, 10.0, want_argmin=False)
                tol = 1e-6 if precision == "f32" else (1e-10 if variant == "general" else 1e-12)
                np.testing.assert_allclose(losses, want, rtol=tol, atol=0)
                dupl, _ = dpts.eval_population(cand, L.LOSS_HUBER, 10.0, want_argmin=False)
                np.testing.assert_allclose(want, dupl, rtol=REASSOC_RTOL[precision], atol=0)


@pytest.mark.parametrize("kw", [dict(), dict(device_loop=True), dict(starts=3), dict(device_loop=True, starts=3, mend_nonfinite=True, precision="f32")])
def test_cma_optimize_with_weights_is_the_run_on_the_duplicated_rows(L, kw):
    """seeded, a handful of generations: the weighted run and the unweighted run on the duplicated rows see losses that differ in
    the order of the additions alone, so they rank every generation alike and end at the same candidate"""
    from alproj_amd import synthetic as syn
    from alproj_amd.optimize import CMAOptimizer
    obj, img, init = t_cma._gcp_problem()
    w = np.random.default_rng(16).integers(0, 4, len(obj)).astype(np.float64)
    run = dict(generation=6, sigma=0.2, population_size=24, f_scale=10.0, seed=7, progress=False, **kw)
    a = CMAOptimizer(obj, img, init, weights=w)
    a.set_target(list(syn.TARGETS_D9))
    pa, ea = a.optimize(**run)
    b = CMAOptimizer(pd.DataFrame(dup(obj.to_numpy(), w), columns=obj.columns), pd.DataFrame(dup(img.to_numpy(), w), columns=img.columns), init)
    b.set_target(list(syn.TARGETS_D9))
    pb, eb = b.optimize(**run)
    rtol = 1e-9 if kw.get("precision") != "f32" else 1e-4
    for k in syn.TARGETS_D9:
        assert pa[k] == pytest.approx(pb[k], rel=rtol, abs=rtol), (k, pa[k], pb[k])
    assert ea == pytest.approx(eb, rel=rtol)
    xyz, uv = dup(obj.to_numpy(), w), dup(img.to_numpy(), w)
    assert ea == pytest.approx(orc.mean_distance(uv, orc.project_points(xyz, pa)), rel=1e-9)      # the weighted mean distance


# ---------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_previous_weights_in_force(L, cases):
    from alproj_amd.optimize import CMAOptimizer, LsqOptimizer
    xyz, uv, o = cases["xyz"][:700], cases["uv"][:700], cases["o"]
    cand = cases["pops"]["general"][:4]
    w = cases["w"][:700].copy()
    with points(L, xyz, uv, o, "f32", w) as pts:
        before = pts.eval_population(cand, L.LOSS_HUBER, 10.0)[0]
        bad_sets = {"length": w[:-1], "negative": np.where(np.arange(700) == 3, -1.0, w), "nan": np.where(np.arange(700) == 699, np.nan, w),
                    "inf": np.where(np.arange(700) == 0, np.inf, w), "zero": np.zeros(700), "2-d": w.reshape(350, 2)}
        for name, bad in bad_sets.items():
            with pytest.raises(ValueError):
                pts.set_weights(bad)
            assert pts.weight_sum() == w.sum(), name
        # the library itself, behind the Python checks
        for bad in (bad_sets["negative"], bad_sets["nan"], bad_sets["inf"]):
            bad = np.ascontiguousarray(bad, dtype=np.float64)
            assert L.lib().alp_points_set_weights(pts._h, bad.ctypes.data_as(ctypes.c_void_p), L.ALP_F64) == EINVAL
            bad32 = bad.astype(np.float32)
            assert L.lib().alp_points_set_weights(pts._h, bad32.ctypes.data_as(ctypes.c_void_p), L.ALP_F32) == EINVAL
        assert L.lib().alp_points_set_weights(pts._h, w.ctypes.data_as(ctypes.c_void_p), 7) == EINVAL
        huge = np.where(np.arange(700) == 1, 1e300, w)           # finite, but not in the float32 the set stores
        assert L.lib().alp_points_set_weights(pts._h, huge.ctypes.data_as(ctypes.c_void_p), L.ALP_F64) == EINVAL
        assert pts.weight_sum() == w.sum()
        after = pts.eval_population(cand, L.LOSS_HUBER, 10.0)[0]
        assert np.array_equal(bits(before), bits(after))
        # pending evaluation
        pts.eval_population_enqueue(cand, L.LOSS_HUBER, 10.0)
        with pytest.raises(RuntimeError) as e:
            pts.set_weights(w)
        assert e.value.code == ESTATE
        with pytest.raises(RuntimeError) as e:
            pts.set_weights(None)
        assert e.value.code == ESTATE
        pending = pts.eval_population_wait(len(cand))[0]
        assert np.array_equal(bits(pending), bits(before))
        # a float32 set rounds: the sum is that of the rounded weights, in index order
        frac = np.random.default_rng(1).uniform(0, 3, 700)
        pts.set_weights(frac)
        s = 0.0
        for v in frac.astype(np.float32).astype(np.float64):
            s += v
        assert pts.weight_sum() == s
    obj, img = pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"])
    init = pc.truth("general")
    for cls in (CMAOptimizer, LsqOptimizer):
        for name, bad in bad_sets.items():
            with pytest.raises(ValueError):
                cls(obj, img, init, weights=bad)
        assert cls(obj, img, init, weights=list(w)).weights.shape == (700,)


def test_world_1_communicator_gives_the_same_bits(L, cases):
    """the count slot carries W through the all-reduce (a single rank: the sums must keep their bits)"""
    xyz, uv, o, w = cases["xyz"], cases["uv"], cases["o"], cases["w"]
    cand = cases["pops"]["general"]
    pv = cand[0]
    with points(L, xyz, uv, o, "f32", w) as pts:
        pts.set_mend(True)
        before = pts.eval_population(cand, L.LOSS_HUBER, 10.0), pts.normal_equations(pv, t_normal.idx(TARGETS), "soft_l1", 1.5)
        L.comm_init(L.comm_unique_id(), 0, 1)
        try:
            assert L.comm_info() == (0, 1)
            during = pts.eval_population(cand, L.LOSS_HUBER, 10.0), pts.normal_equations(pv, t_normal.idx(TARGETS), "soft_l1", 1.5)
        finally:
            L.comm_destroy()
    assert np.array_equal(bits(before[0][0]), bits(during[0][0])) and before[0][1] == during[0][1]
    for a, b in zip(before[1], during[1]):
        assert np.array_equal(bits(a), bits(b))
    assert before[1][3] == w.sum()
