"""The mend pass of a float32 point set (alp_points_set_mend, alp_eval_population_mended, CMAOptimizer.optimize(...,
mend_nonfinite=True)): every candidate whose float32 loss sum is infinite or NaN gets, on the device, the value float64
arithmetic gives on the stored float32 points.  The scene, the populations and the reasons for the margins: tests/mend_cases.py.

The reference is the float64 oracle on the STORED inputs (the float32-rounded points and observations), the tolerance of a
mended loss rtol 1e-7 -- what tests/test_gpu_points.py::test_population_golden_wild_f64 holds float64 arithmetic to, four decades
above the oracle's own frame noise on this local scene (1e-11).  Every test asserts its precondition: with mend off, the
non-finite float32 losses are exactly the candidates meant to be flagged."""
import numpy as np
import pandas as pd
import pytest

from alproj_amd import _lib
from alproj_amd import synthetic as syn
from alproj_amd.cma import CMA
from alproj_amd.optimize import CMAOptimizer, bounds_to_array
from oracle import ref_numpy as orc
from tests import mend_cases as mc
from tests.popeval_cases import oracle_r2, pole_a2_steps

pytestmark = pytest.mark.gpu

RTOL = 1e-7
ESTATE = -6


@pytest.fixture(scope="module")
def L():
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def seams():
    """the scene, and per variant the tame and the wild population with the oracle's losses of both"""
    xyz, uv = mc.scene()
    out = {"xyz": xyz, "uv": uv}
    for v in mc.VARIANTS:
        tame, wild = mc.populations(v)
        out[v] = (tame, wild, mc.oracle(xyz, uv, tame), mc.oracle(xyz, uv, wild))
    return out


def _points(L, xyz, uv, prec="f32"):
    pts = L.Points(xyz, mc.ORIGIN, prec)
    pts.set_observed(uv)
    return pts


def _check_mended(L, pts, cand, flagged, ref, loss, variant=None):
    """mend off, then mend on, on the same handle: the precondition, the mended losses against the oracle, the other losses bit
    for bit, the count and the argmin.  Returns what eval_population_mended() says."""
    kind, fs = mc.LOSSES[loss]
    intended = np.zeros(len(cand), dtype=bool)
    intended[flagged] = True
    pts.set_mend(False)
    off, _ = pts.eval_population(cand, kind, fs, want_argmin=False)
    if variant is not None:
        assert pts.eval_population_info()[0] == variant
    np.testing.assert_array_equal(~np.isfinite(off), intended, err_msg="precondition: the float32 losses that are not finite")
    assert pts.eval_population_mended()[0] == 0
    pts.set_mend(True)
    on, _ = pts.eval_population(cand, kind, fs, want_argmin=False)
    info = pts.eval_population_mended()
    err = np.abs(on[intended] / ref[intended] - 1.0)
    print(f"mended: {intended.sum()} candidates, largest relative error {err.max() if len(err) else 0.0:.3e}")
    assert np.isfinite(ref[intended]).all()
    np.testing.assert_allclose(on[intended], ref[intended], rtol=RTOL, atol=0)
    np.testing.assert_array_equal(on[~intended], off[~intended])
    assert info[0] == int(intended.sum())
    assert info[2:] == mc.mend_grid(pts.n, len(cand), cu=L.device_info()["cu_count"])
    _, amin = pts.eval_population(cand, kind, fs)
    assert amin == orc.first_argmin(ref)
    return info


@pytest.mark.parametrize("which", ["none", "first", "last", "tile", "tile_plus_one", "all"])
@pytest.mark.parametrize("loss", ["mean_dist", "huber"])
@pytest.mark.parametrize("variant", mc.VARIANTS)
def test_compaction_seams(L, seams, variant, loss, which):
    """P = 300 (tiles of 128 / 128 / 44) with no candidate flagged, the first, the last, exactly one tile's worth, one more, all"""
    tame, wild, tame_l, wild_l = seams[variant]
    flagged = mc.flagged_sets()[which]
    assert len(flagged) == {"none": 0, "first": 1, "last": 1, "tile": 128, "tile_plus_one": 129, "all": mc.P}[which]
    cand = mc.mix(tame, wild, flagged)
    ref = mc.mix_losses(tame_l, wild_l, flagged)[loss]
    assert mc.argmin_margin(ref)[1] >= mc.MARGIN[(variant, len(flagged) == mc.P)]
    with _points(L, seams["xyz"], seams["uv"]) as pts:
        info = _check_mended(L, pts, cand, flagged, ref, loss, variant)
        # the total since mend was enabled: the evaluation without the argmin, then the one with it
        assert info[1] == len(flagged) and pts.eval_population_mended()[1] == 2 * len(flagged)


POINT_SETS = {"below_one_row": dict(head=198), "ragged": dict(), "whole_groups_and_a_tail": dict(extra=5 * 256 - 1127),
              "tiled": dict(copies=3)}


@pytest.mark.parametrize("name", list(POINT_SETS))
def test_point_counts(L, name):
    """n = 200 (below one row of 256), 1129 (ragged), 5 x 256 + 2 (one whole float64 group of five rows and a tail of two
    points), and three offset copies (3383 points: several stripes), each against 140 candidates in two tiles, 61 of them flagged"""
    xyz, uv = mc.scene(**POINT_SETS[name])
    assert len(xyz) == {"below_one_row": 200, "ragged": 1129, "whole_groups_and_a_tail": 1282, "tiled": 3383}[name]
    tame, wild = mc.populations("general", 140)
    others = np.array([i for i in range(140) if i != mc.best(140)])
    flagged = np.sort(np.random.default_rng(8).permutation(others)[:61])
    cand = mc.mix(tame, wild, flagged)
    ref = mc.mix_losses(mc.oracle(xyz, uv, tame), mc.oracle(xyz, uv, wild), flagged)
    with _points(L, xyz, uv) as pts:
        for loss in mc.LOSSES:
            assert mc.argmin_margin(ref[loss])[1] >= mc.MARGIN[("general", False)]
            info = _check_mended(L, pts, cand, flagged, ref[loss], loss, "general")
            if name == "tiled":
                assert info[2] >= 2 and info[3] >= 2


@pytest.mark.parametrize("variant", ["shared_pose", "general"])
@pytest.mark.parametrize("loss", ["mean_dist", "huber"])
def test_exact_pole_is_never_nan(L, loss, variant):
    """the construction of tests/test_gpu_points.py::test_pole_of_one_lens_denominator_is_an_infinite_loss on a float32 set:
    mend off keeps the shared reciprocal's NaN on the device's float32 pole; mend on gives that candidate what float64
    arithmetic gives -- finite next to the float64 pole, +inf on it, never NaN -- and leaves the two sane candidates alone"""
    kind, fs = mc.LOSSES[loss]
    truth = dict(syn.truth_params(316), k4=-0.5, k5=0.0, k6=0.0)
    xyz = syn.gcp_points(400, truth, seed=31, margin=-0.25)
    r2 = oracle_r2(xyz, truth)
    i0 = int(np.argmin(np.abs(r2 - 1.4)))
    keep = (np.abs(1 - r2 / 2) > 0.25) & (np.abs(1 + truth["a2"] - r2 / 2) > 0.25)
    keep[i0] = True
    i = int(np.count_nonzero(keep[:i0]))
    xyz, r2 = xyz[keep], r2[keep]
    uv = orc.project_points(xyz, truth) + np.random.default_rng(31).normal(0, 1.0, (len(xyz), 2))
    a2 = pole_a2_steps(r2[i], -0.5, "f32")
    cand = np.tile(L.params_vector(truth), (len(a2) + 2, 1))
    cand[2:, L.PARAM_KEYS.index("a2")] = a2
    cand[1, L.PARAM_KEYS.index("a1")] += 0.01
    if variant == "general":
        cand[0, L.PARAM_KEYS.index("pan")] += 0.01
    with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], "f32") as pts:
        pts.set_observed(uv)
        off, _ = pts.eval_population(cand, kind, fs, want_argmin=False)
        assert pts.eval_population_info()[0] == variant
        hit = np.flatnonzero(~np.isfinite(off))
        assert len(hit) >= 1 and hit.min() >= 2, "precondition: a candidate on the device's float32 pole, the sane ones finite"
        pts.set_mend(True)
        on, _ = pts.eval_population(cand, kind, fs, want_argmin=False)
        assert pts.eval_population_mended()[0] == len(hit)
        _, amin = pts.eval_population(cand, kind, fs)
    assert not np.isnan(on).any() and np.all(np.isfinite(on) | np.isposinf(on))
    np.testing.assert_array_equal(on[:2], off[:2])
    assert amin in (0, 1)


def test_vertex_at_the_camera_stays_nan(L):
    """a lens-free population with a vertex at a candidate's camera (Q7): the reference's loss is NaN, and so is the mended one;
    a2 = -1 stays +inf; the finite candidate keeps its bits"""
    p = dict(syn.base_params(316), **{k: 0.0 for k in L.DIST_KEYS[2:]})
    xyz = syn.gcp_points(700, p, seed=53)
    uv = orc.project_points(xyz, p) + np.random.default_rng(53).normal(0, 1.0, (700, 2))
    cands = np.stack([L.params_vector(p), L.params_vector(dict(p, x=p["x"] + 1.0)), L.params_vector(dict(p, a2=-1.0, x=p["x"] + 2.0)),
                      L.params_vector(dict(p, pan=p["pan"] + 0.1))])
    xyz[5] = [p["x"], p["y"], p["z"]]
    with np.errstate(all="ignore"):
        ref = np.array([orc.loss_of(xyz, uv, orc.vector_to_params(c), 0, 0.0) for c in cands])
    assert np.isnan(ref[0]) and np.isfinite(ref[1]) and np.isposinf(ref[2]) and np.isnan(ref[3])
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f32") as pts:
        pts.set_observed(uv)
        off, _ = pts.eval_population(cands, L.LOSS_MEAN_DIST, 0.0)
        assert pts.eval_population_info()[0] == "lens_free"
        np.testing.assert_array_equal(np.isfinite(off), [False, True, False, False])
        pts.set_mend(True)
        on, amin = pts.eval_population(cands, L.LOSS_MEAN_DIST, 0.0)
        assert pts.eval_population_mended()[:2] == (3, 3)
    assert np.isnan(on[0]) and np.isnan(on[3]) and np.isposinf(on[2]) and amin == 1
    assert on[1] == off[1]


def test_float64_set_takes_the_setting_and_runs_no_pass(L, seams):
    tame, wild, _, _ = seams["general"]
    cand = mc.mix(tame, wild, mc.flagged_sets()["tile"])
    with _points(L, seams["xyz"], seams["uv"], "f64") as pts:
        off, a0 = pts.eval_population(cand, L.LOSS_HUBER, mc.F_SCALE)
        pts.set_mend(True)
        on, a1 = pts.eval_population(cand, L.LOSS_HUBER, mc.F_SCALE)
        assert pts.eval_population_mended() == (0, 0, 0, 0)
    assert np.isfinite(off).all() and a0 == a1
    np.testing.assert_array_equal(on, off)


def _problem():
    xyz, uv = mc.scene()
    return pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"]), mc.base_params()


def _host_cma(D, P, seed):
    return CMA(mean=np.full(D, 0.5), sigma=1.0, bounds=np.column_stack([np.zeros(D), np.ones(D)]), population_size=P,
               n_max_resampling=100, seed=seed, sampler=_lib.cma_sample)


LENS_AND_FOV = ["fov", "a1", "a2", "k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2", "s1", "s2", "s3", "s4"]
LOOP_TARGETS = {"pose_kept": LENS_AND_FOV, "g5_d21": [str(t) for t in mc.g5()["d21_targets"]]}


@pytest.mark.parametrize("name", list(LOOP_TARGETS))
def test_device_loop_generations_match_the_host_path(L, name):
    """six generations at sigma = 1, pop 256, float32 with mend on: the comparison of
    tests/test_gpu_cma_device.py::test_generations_match_the_host_path against the host path with mend on.  pose_kept: the pose
    stays the scene's, whose planted vertices overflow float32 under any lens that grows with r^4; g5_d21: the camera moves
    too, and the number of flagged candidates varies."""
    obj, img, init = _problem()
    targets = LOOP_TARGETS[name]
    opt = CMAOptimizer(obj, img, init)
    opt.set_target(list(targets))
    D, P = len(targets), 256
    b = bounds_to_array(init, targets)
    lo, hi = b[:, 0], b[:, 1]
    host = _host_cma(D, P, 11)
    host.set_state(dict(host.get_state(), mean=(opt.target_params_init - lo) / (hi - lo), sigma=1.0))
    counts = []
    with opt._device_points("f32") as pts:
        pts.set_mend(True)
        with L.CmaDevice(pts, L.params_vector(init), [L.PARAM_KEYS.index(t) for t in targets], lo, hi, host) as loop:
            loop.set_state(host.get_state())
            for g in range(6):
                st = loop.get_state(eigen=True)
                assert st["g"] == g
                loop.run(1, L.LOSS_HUBER, mc.F_SCALE)
                loop.wait()
                assert pts.eval_population_info()[0] == "general"
                counts.append(pts.eval_population_mended()[:2])
                X, cand, losses = loop.fetch_last()
                ref = L.cma_sample(st["mean"], st["sigma"], st["B"] * st["D"], np.column_stack([np.zeros(D), np.ones(D)]), P, 100,
                                   host._sampler_seed, g)
                np.testing.assert_array_equal(X, ref)
                np.testing.assert_array_equal(cand, opt._candidate_matrix(X * (hi - lo) + lo))
                assert not np.isnan(losses).any(), g
                want, _ = pts.eval_population(cand, L.LOSS_HUBER, mc.F_SCALE, want_argmin=False)
                assert pts.eval_population_mended()[0] == counts[-1][0]         # the host path flags the same candidates
                np.testing.assert_allclose(losses, want, rtol=1e-6, atol=0)
    print(name, "flagged per generation, running total:", counts)
    assert counts[-1][1] > 0 and all(0 <= c <= P for c, _ in counts)
    # the running total: every generation counted twice here (the loop's and the host path's evaluation)
    assert counts[-1][1] == 2 * sum(c for c, _ in counts) - counts[-1][0]


def test_starts_are_single_runs_with_mend(L):
    """optimize(device_loop=True, mend_nonfinite=True, starts=3) is the three single runs (at this point count the launch of
    768 candidates has the stripes of the launch of 256: the float32 sums are the same bits)"""
    obj, img, init = _problem()
    o = CMAOptimizer(obj, img, init)
    o.set_target(list(LENS_AND_FOV))
    kw = dict(generation=6, sigma=1.0, population_size=256, f_scale=mc.F_SCALE, progress=False, device_loop=True, precision="f32",
              mend_nonfinite=True)
    params, err = o.optimize(seed=7, starts=3, **kw)
    multi = list(o.start_results)
    assert np.isfinite(err)
    for k in range(3):
        p1, e1 = o.optimize(seed=7 + k, **kw)
        assert multi[k][1] == p1, k
        assert abs(multi[k][2] - e1) <= 1e-12 * e1, (k, multi[k][2], e1)


def test_world1_communicator_changes_nothing(L, seams):
    """the pass's own all-reduce of P doubles through a world-size-1 communicator: the same bits, on the host path and in the
    device loop"""
    tame, wild, _, _ = seams["general"]
    cand = mc.mix(tame, wild, mc.flagged_sets()["tile_plus_one"])
    obj, img, init = _problem()
    b = bounds_to_array(init, LENS_AND_FOV)
    idx = [L.PARAM_KEYS.index(t) for t in LENS_AND_FOV]

    def run():
        with _points(L, seams["xyz"], seams["uv"]) as pts:
            pts.set_mend(True)
            losses, amin = pts.eval_population(cand, L.LOSS_HUBER, mc.F_SCALE)
            count = pts.eval_population_mended()[0]
            with L.CmaDevice(pts, L.params_vector(init), idx, b[:, 0], b[:, 1], _host_cma(len(idx), 256, 5)) as loop:
                loop.run(2, L.LOSS_HUBER, mc.F_SCALE)
                loop.wait()
                return (losses, amin, count) + tuple(loop.fetch_last()) + (pts.eval_population_mended()[:2],)

    alone = run()
    L.comm_init(L.comm_unique_id(), 0, 1)
    try:
        assert L.comm_info() == (0, 1)
        with_comm = run()
    finally:
        L.comm_destroy()
    assert alone[2] == 129 and alone[6][0] > 0 and np.isfinite(alone[0]).all()
    for a, c in zip(alone, with_comm):
        np.testing.assert_array_equal(a, c)


def test_refusals(L, seams):
    tame, _, _, _ = seams["general"]
    obj, img, init = _problem()
    b = bounds_to_array(init, LENS_AND_FOV)
    with _points(L, seams["xyz"], seams["uv"]) as pts:
        with pytest.raises(L.AlprojHipError) as e:
            pts.eval_population_mended()                      # before any evaluation
        assert e.value.code == ESTATE
        pts.set_mend(True)
        pts.set_mend(False)
        P = pts.eval_population_enqueue(tame[:8], L.LOSS_HUBER, mc.F_SCALE)
        with pytest.raises(L.AlprojHipError) as e:
            pts.set_mend(True)                                # an evaluation is pending
        assert e.value.code == ESTATE
        with pytest.raises(L.AlprojHipError) as e:
            pts.eval_population_mended()
        assert e.value.code == ESTATE
        pts.eval_population_wait(P)
        assert pts.eval_population_mended() == (0, 0, 0, 0)   # an evaluation without the pass
        pts.set_mend(True)
        with L.CmaDevice(pts, L.params_vector(init), [L.PARAM_KEYS.index(t) for t in LENS_AND_FOV], b[:, 0], b[:, 1],
                         _host_cma(len(LENS_AND_FOV), 8, 1)) as loop:
            loop.run(1, L.LOSS_HUBER, mc.F_SCALE)
            with pytest.raises(L.AlprojHipError) as e:
                pts.set_mend(False)                           # a device loop is pending
            assert e.value.code == ESTATE
            loop.wait()
            pts.set_mend(False)
