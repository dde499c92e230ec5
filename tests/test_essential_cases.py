"""CPU: the numpy restatement of the essential-matrix match filter (tests/essential_cases.py) against the constraints an essential
matrix satisfies, the truth of its synthetic scenes and an independent count of the polynomial's real roots, and every edge
case of alproj_amd.gcp.filter_geometric(method="essential") / filter_matches(params=...) that makes no device call.
tests/test_gpu_essential.py holds the device to the restatement."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
import essential_cases as es  # noqa: E402

K = es.K_TRUE
# "to rounding": E has unit norm and a solution is kept only when the Gauss-Newton steps brought the cubics below POLISH_TOL =
# 5e-14 in Euclidean norm; the largest single entry, formed again here from E by another route, gets twice that
CONSTRAINT_TOL = 1e-13


@pytest.fixture(scope="module", params=["general", "planar"])
def solved(request):
    """noise-free scene(200, 0, 0.0, 1), general or planar, 257 numpy-drawn samples and the restatement's solutions: once"""
    planar = request.param == "planar"
    p1, p2, F, _ = es.make_scene(200, 0, 0.0, 1, planar)
    samples = es.draw_samples5(200, 257, 5)
    return {"planar": planar, "p1": p1, "p2": p2, "F": F, "samples": samples, "details": es.solve5_details(p1, p2, samples, K)}


def test_solutions_satisfy_the_epipolar_and_the_essential_constraints(solved):
    a, b = es.normalise(solved["p1"], K), es.normalise(solved["p2"], K)
    worst = [0.0, 0.0, 0.0]
    seen = 0
    for s, d in zip(solved["samples"], solved["details"]):
        assert len(d["F"]) == len(d["E"]) == len(d["z"]) <= 10 and (np.diff(d["z"]) > 0).all()
        for E, F in zip(d["E"], d["F"]):
            epi = np.abs(es._design(a[s], b[s]) @ E.ravel()).max()
            det, trace = es.essential_residuals(E)
            worst = [max(w, v) for w, v in zip(worst, (epi, det, trace))]
            # F is E in pixels: the same matrix up to scale
            back = es.to_essential(F, K)
            assert ec.sign_distance(back / np.sqrt((back * back).sum()), E)[0] <= 1e-12
            assert abs(np.sqrt((F * F).sum()) - 1.0) <= 1e-15
            seen += 1
    print("worst epipolar, det, trace residual", worst, "over", seen, "solutions")
    assert seen > 1200 and max(worst) <= CONSTRAINT_TOL


def test_one_solution_of_every_sample_is_the_truth(solved):
    """Every sample, none left out.  The general scene is where SELF_DISTANCE, and with it the tolerance of the device test, is
    measured.  On the noise-free plane the 10 x 10 part of the cubics is close to singular for one sample in twenty (condition
    numbers of 1e10 and more): the polynomial that comes out of it has lost the true root, the solutions that remain are
    essential matrices through the five matches all the same (the test above), and the truth is then missed by 1e-3 to 2e-2.
    Measured: 12 of 257 samples; the bound is 5 %, and every other sample finds the truth to 1e-10."""
    d = np.array([ec.sign_distance(x["F"], solved["F"]).min() if len(x["F"]) else np.inf for x in solved["details"]])
    missed = d > 1e-10
    print("planar" if solved["planar"] else "general", "worst distance to the truth", d[~missed].max(), "missed", missed.sum(), "of", len(d))
    if solved["planar"]:
        assert missed.mean() <= 0.05
    else:
        assert d.max() <= es.SELF_DISTANCE
        assert es.DEVICE_TOL == 100 * es.SELF_DISTANCE


def test_real_root_count_equals_an_independent_count(solved):
    """numpy.linalg.eigvals on the companion matrix against the sign changes of p between the real roots of p', on every sample
    that ill_conditioned keeps.  The general scene: equal everywhere.  The noise-free plane: its polynomials have coefficients
    over ten decades and roots in clusters, and the two counts differ on 1 of 191 samples (6 against 4 roots, a pair that the
    companion matrix's eigenvalues put off the axis); the bound is 1 %."""
    checked, differ = 0, 0
    for d in solved["details"]:
        if d["p"] is None or d["skip"]:
            continue
        differ += es.count_real_roots(d["p"]) != len(d["roots"])
        assert len(d["roots"]) % 2 == 0                   # degree 10 with real coefficients, no double root among these
        checked += 1
    print("planar" if solved["planar"] else "general", "counts differ on", differ, "of", checked)
    assert checked >= (150 if solved["planar"] else 240)
    assert differ <= (0.01 * checked if solved["planar"] else 0)


@pytest.mark.parametrize("n", sorted(es.SEAM_SEEDS))
def test_launch_seam_cases_are_decided(n):
    """The seeds of the device test's launch seams: at every H the chosen slot cannot hang on a match near the threshold, and
    neither can a count on the restatement's way through the refits (fewer than 8 inliers leave the refit undefined)."""
    p1, p2, samples, Fs = es.seam_case(n)
    for H in es.SEAM_H:
        assert es.choice_is_decided(Fs[:H], p1, p2, 3.0), (n, H)
        for refits in (0, 4):
            want = es.ransac5(p1, p2, samples[:H], K, 3.0, refits=refits, Fs=Fs[:H])
            if refits == 0 or want["chosen_count"] >= 8:
                assert es.path_is_decided(want["path"], p1, p2, 3.0), (n, H, refits)


def test_null_basis_spans_the_null_space_and_refuses_rank_four():
    p1, p2, _, _ = es.scene(50, 0, 0.5, 2)
    a, b = es.normalise(p1, K), es.normalise(p2, K)
    A = es._design(a[:5], b[:5])
    N = es.null_basis(A)
    assert N.shape == (4, 9) and np.abs(A @ N.T).max() <= 1e-14 and np.linalg.matrix_rank(N) == 4
    assert es.null_basis(es._design(a[[0, 1, 2, 3, 3]], b[[0, 1, 2, 3, 3]])) is None
    assert len(es.solve5(p1, p2, np.array([0, 1, 2, 3, 3]), K)) == 0
    q1, q2 = p1.copy(), p2.copy()
    q1[4], q2[4] = q1[1], q2[1]                           # two of the five points coincide
    assert len(es.solve5(q1, q2, np.arange(5), K)) == 0
    assert len(es.solve5(p1, p2, np.arange(5), K)) > 0


def test_essential_projection():
    rng = np.random.default_rng(0)
    E = es.project_essential(rng.standard_normal((3, 3)))
    S = np.linalg.svd(E, compute_uv=False)
    assert abs(S[0] - S[1]) <= 1e-15 and S[2] <= 1e-15
    assert max(es.essential_residuals(E)) <= 1e-15
    np.testing.assert_allclose(es.project_essential(E), E, rtol=0, atol=1e-15)


@pytest.mark.parametrize("n,n_out,threshold,seed,planar", es.RANSAC5_SCENES)
def test_ransac5_restatement_against_the_truth(n, n_out, threshold, seed, planar):
    """The scenes of the device test: every true inlier kept, no outlier kept except at most 2 within threshold of the true
    epipolar lines, and no match within 1 % of threshold^2 (so that two numerical routes give one mask)."""
    p1, p2, F, out = es.make_scene(n, n_out, 0.5, seed, planar)
    r = es.ransac5(p1, p2, es.draw_samples5(n, es.RANSAC5_SAMPLES, 1000 + seed), K, threshold)
    e = es.errors(r["F"], p1, p2)
    assert not (np.abs(e - threshold ** 2) <= 0.01 * threshold ** 2).any()
    assert not r["keep_all"] and r["mask"][~out].all()
    kept = out & r["mask"]
    assert kept.sum() <= 2 and (es.errors(F, p1, p2)[kept] <= threshold ** 2).all()
    assert r["final_count"] == r["mask"].sum() >= r["chosen_count"] >= 5
    assert len(r["refit_counts"]) == min(r["refits_kept"] + 1, 4)
    assert 0 <= r["chosen"] < 10 * es.RANSAC5_SAMPLES
    # the final matrix is essential: chosen from the solver, or projected by the refit
    assert max(es.essential_residuals(es.to_essential(r["F"], K))) <= 1e-9


def test_low_inlier_share_is_where_five_points_pay():
    """w = 0.3: the same number of 8-point samples holds no all-inlier one (probability 0.93 at 1024), so the 8-point filter does
    not find the scene.  (On the planar scene the 8-point filter does keep every true inlier, with any of the fundamental
    matrices that agree with the plane's homography, so that comparison shows nothing and is not made.)"""
    n, n_out, threshold, seed, planar = es.RANSAC5_SCENES[0]
    assert n_out / n == 0.7 and not planar
    p1, p2, _, out = es.make_scene(n, n_out, 0.5, seed, planar)
    r8 = ec.ransac(p1, p2, ec.draw_samples(n, es.RANSAC5_SAMPLES, 1000 + seed), threshold)
    assert not r8["mask"][~out].all()


def test_ransac5_keeps_everything_without_five_inliers():
    p1, p2, _, _ = es.scene(12, 0, 0.5, 3)
    samples = np.tile(np.array([0, 1, 2, 3, 3], dtype=np.int32), (8, 1))          # every sample degenerate: no finite slot
    r = es.ransac5(p1, p2, samples, K, 3.0)
    assert r["keep_all"] and r["mask"].all() and r["chosen"] == 0 and r["chosen_count"] == 0 and r["refit_counts"] == []


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_filter_geometric_essential_without_a_device_call():
    from alproj_amd import gcp
    p = np.arange(8.0).reshape(4, 2)
    for method in ("essential", "Essential"):
        m = gcp.filter_geometric(p, p, method=method)                               # fewer than 5 points: before the focal length
        assert m.dtype == bool and m.all() and m.shape == (4,)
    mask, F, info = gcp.filter_geometric(p, p, method="essential", focal_length=1000.0, return_model=True)
    assert mask.all() and F is None and info == {}
    assert gcp.filter_geometric(np.zeros((0, 2)), np.zeros((0, 2)), method="essential").shape == (0,)
    q = np.arange(20.0).reshape(10, 2)
    with pytest.raises(NotImplementedError, match="stays with the reference"):
        gcp.filter_geometric(q, q, method="essential")
    with pytest.raises(NotImplementedError, match="stays with the reference"):
        gcp.filter_geometric(q, q, method="essential", principal_point=(5.0, 5.0), image_size=(100, 100))
    bad = q.copy()
    bad[3, 1] = np.nan
    for args, kw in (((q, q), {"focal_length": 0.0}), ((q, q), {"focal_length": -5.0}), ((q, q), {"focal_length": np.inf}),
                     ((q, q), {"focal_length": np.nan}), ((q, q), {"principal_point": (1.0, np.nan)}),
                     ((q, q), {"principal_point": (1.0, 2.0, 3.0)}), ((q, q), {"samples": np.zeros((4, 8), dtype=np.int32)}),
                     ((q, q), {"samples": np.zeros((0, 5), dtype=np.int32)}), ((q, q), {"samples": np.zeros(5, dtype=np.int32)}),
                     ((q, q[:9]), {}), ((bad, q), {}), ((q, q), {"threshold": -1.0}), ((q, q), {"hypotheses": 0}), ((q, q), {"refits": 9})):
        kw.setdefault("focal_length", 1000.0)
        with pytest.raises(ValueError):
            gcp.filter_geometric(*args, method="essential", **kw)


class _Recorder:
    """stands in for _lib.essential_ransac: records what the Python layer passes down"""

    def __init__(self):
        self.calls = []

    def __call__(self, p1, p2, focal_length, principal_point, threshold, **kw):
        self.calls.append({"f": float(focal_length), "c": tuple(float(v) for v in principal_point), "threshold": threshold, **kw})
        return {"F": np.eye(3), "mask": np.ones(len(p1), dtype=bool), "info": {"chosen": 0}}


def test_principal_point_defaults_and_params(monkeypatch):
    from alproj_amd import _lib, gcp
    rec = _Recorder()
    monkeypatch.setattr(_lib, "essential_ransac", rec)
    rng = np.random.default_rng(1)
    p1, p2 = rng.uniform(0, 900, (30, 2)), rng.uniform(0, 900, (30, 2))
    gcp.filter_geometric(p1, p2, method="essential", focal_length=1100.0, principal_point=(700.0, 400.0), image_size=(1504, 1000))
    gcp.filter_geometric(p1, p2, method="essential", focal_length=1100.0, image_size=(1505, 1000))
    gcp.filter_geometric(p1, p2, method="essential", focal_length=1100.0)
    assert [c["c"] for c in rec.calls] == [(700.0, 400.0), (752.5, 500.0),
                                           ((p1[:, 0].max() + p1[:, 0].min()) / 2, (p1[:, 1].max() + p1[:, 1].min()) / 2)]
    assert all(c["f"] == 1100.0 and c["threshold"] == 10.0 and c["samples"] is None for c in rec.calls)
    mask, F, info = gcp.filter_geometric(p1, p2, method="essential", focal_length=2.0, principal_point=(1.0, 3.0), return_model=True)
    np.testing.assert_array_equal(info["E"], np.array([[2.0, 0, 1.0], [0, 2.0, 3.0], [0, 0, 1.0]]).T @ np.eye(3) @ np.array([[2.0, 0, 1.0], [0, 2.0, 3.0], [0, 0, 1.0]]))
    # filter_matches: image_match's own derivation (reference gcp.py:466-474)
    del rec.calls[:]
    q1, q2 = p1.astype("int32"), p2.astype("int32")
    params = {"fov": 64.0, "w": 1504, "h": 1000, "cx": 760.0, "cy": 490.0}
    gcp.filter_matches(q1, q2, (1504, 1000), outlier_filter="essential", threshold=3.0, params=params, seed=4, hypotheses=99)
    gcp.filter_matches(q1, q2, (1504, 1000), outlier_filter="essential", params={"fov": 64.0, "w": 1504, "h": 1000})
    gcp.filter_matches(q1, q2, (1500, 1000), outlier_filter="essential", params={"fov": 64.0, "w": 1504})
    f = (1504 / 2) / math.tan(64.0 * math.pi / 180 / 2)
    assert f == (1504 / 2) / math.tan(64.0 * math.pi / 360)
    assert [c["f"] for c in rec.calls] == [f, f, f]
    assert [c["c"] for c in rec.calls] == [(760.0, 490.0), (752.0, 500.0), (750.0, 500.0)]
    assert rec.calls[0]["threshold"] == 3.0 and rec.calls[0]["seed"] == 4 and rec.calls[0]["hypotheses"] == 99
    with pytest.raises(NotImplementedError, match="stays with the reference"):
        gcp.filter_matches(q1, q2, (1504, 1000), outlier_filter="essential", params={"w": 1504, "h": 1000})
    with pytest.raises(NotImplementedError, match="stays with the reference"):
        gcp.filter_matches(q1, q2, (1504, 1000), outlier_filter="essential")
    # params do not disturb the other filters
    assert len(gcp.filter_matches(q1[:3], q2[:3], None, outlier_filter="none", params=params)) == 3


def test_lib_refuses_bad_shapes_before_the_device():
    from alproj_amd import _lib
    p = np.arange(20.0).reshape(10, 2)
    for samples in (np.zeros((4, 8), dtype=np.int32), np.zeros((0, 5), dtype=np.int32), np.zeros(5, dtype=np.int32)):
        with pytest.raises(ValueError, match=r"samples must be \(H, 5\)"):
            _lib.essential_ransac(p, p, 1000.0, (5.0, 5.0), 3.0, samples=samples)
        with pytest.raises(ValueError, match=r"samples must be \(H, 5\)"):
            _lib.epipolar_solve5(p, p, samples, 1000.0, (5.0, 5.0))
    for f in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="focal_length"):
            _lib.essential_ransac(p, p, f, (5.0, 5.0), 3.0)
    with pytest.raises(ValueError):
        _lib.epipolar_samples5(10, 0)
