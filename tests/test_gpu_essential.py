"""GPU: the essential-matrix match filter (alp_epipolar_samples5 / alp_epipolar_solve5 / alp_essential_ransac) and the Python layer
over it (alproj_amd.gcp.filter_geometric(method="essential") / filter_matches(outlier_filter="essential", params=...)) against the
numpy restatement of tests/essential_cases.py and the truth of its synthetic scenes.

what can go wrong                                             where it is held
a repeated or out-of-range index, the 8-wide stream disturbed  test_samples5_*
null space, cubics, elimination, roots, back substitution     test_solve5_equals_the_restatement (sets, order, constraints)
a degenerate sample that is not refused                       test_solve5_degenerate_samples
ten slots per sample in the score, merge and choose           test_ransac5_equals_the_restatement, test_ransac5_launch_seams
the essential refit, its stop, the final mask                 test_ransac5_equals_the_restatement (and the truth)
the device's own draws, no finite slot at all                 test_ransac5_own_draws, test_ransac5_keeps_everything_without_a_finite_slot
K, the defaults and params of the Python layer                test_python_layer_equals_the_restatement
refusals of the C entry points                                test_entry_point_refusals

What makes no device call needs no GPU: tests/test_essential_cases.py."""
import ctypes
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
import essential_cases as es  # noqa: E402
import linalg_cases as lg  # noqa: E402

pytestmark = pytest.mark.gpu

K = es.K_TRUE
F0, C0 = K[0], K[1:]
CONSTRAINT_TOL = 1e-13        # tests/test_essential_cases.py: the same bound holds the restatement (twice the kernel's SOLVE5_POLISH_TOL)


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def solved():
    """scene(200, 0, sigma, 1) for sigma = 0 and 0.5, 257 numpy-drawn samples and the restatement's solutions of each: computed
    once, shared, never changed"""
    out = {}
    for sigma in (0.0, 0.5):
        p1, p2, F, _ = es.scene(200, 0, sigma, 1)
        samples = es.draw_samples5(200, 257, 5)
        Fs, nsol, skip = es.solve5_all(p1, p2, samples, K)
        out[sigma] = {"p1": p1, "p2": p2, "F": F, "samples": samples, "Fs": Fs, "nsol": nsol, "skip": skip}
    return out


@pytest.fixture(scope="module")
def scenes():
    """the whole-filter scenes with their samples and the restatement's slots: computed once, shared, never changed"""
    out = {}
    for n, n_out, threshold, seed, planar in es.RANSAC5_SCENES:
        p1, p2, F, outlier = es.make_scene(n, n_out, 0.5, seed, planar)
        samples = es.draw_samples5(n, es.RANSAC5_SAMPLES, 1000 + seed)
        out[n] = {"p1": p1, "p2": p2, "F": F, "out": outlier, "samples": samples, "threshold": threshold,
                  "Fs": es.solve5_all(p1, p2, samples, K, judge=False)[0]}
    return out


# ------------------------------------------------------------------------------------------------------------ samples
@pytest.mark.parametrize("n", [5, 6, 64, 1000])
def test_samples5_rows_are_distinct_and_in_range(L, n):
    s = L.epipolar_samples5(n, 2048, seed=3)
    assert s.shape == (2048, 5) and s.dtype == np.int32
    assert s.min() >= 0 and s.max() < n
    assert (np.diff(np.sort(s, axis=1), axis=1) > 0).all()
    if n == 5:
        assert (np.sort(s, axis=1) == np.arange(5)).all() and len(np.unique(s, axis=0)) == 120          # every permutation


def test_samples5_are_a_function_of_the_seed_and_leave_the_8_wide_stream_alone(L):
    a = L.epipolar_samples5(1000, 4096, seed=5)
    np.testing.assert_array_equal(a, L.epipolar_samples5(1000, 4096, seed=5))
    for H in (1, 63, 257):                                     # another launch shape: the same rows
        np.testing.assert_array_equal(L.epipolar_samples5(1000, H, seed=5), a[:H])
    for seed in (6, 5 + 2 ** 32):                              # both words of the seed count
        assert (L.epipolar_samples5(1000, 4096, seed=seed) != a).any(axis=1).mean() > 0.99
    eight = L.epipolar_samples(1000, 4096, seed=5)
    assert (eight[:, :5] != a).any(axis=1).mean() > 0.99       # a stream of their own
    # the 8-wide rows of a seed are what they were before the 5-wide stream existed: rows 0, 1 and 4095 of (n = 1000, seed = 5),
    # and every row by the numpy restatement of the draw
    np.testing.assert_array_equal(eight[[0, 1, 4095]], [[542, 903, 515, 304, 108, 338, 538, 862], [764, 518, 403, 72, 925, 77, 563, 583],
                                                        [83, 395, 918, 694, 893, 447, 419, 270]])
    np.testing.assert_array_equal(eight[:300], es.device_samples(1000, 300, 5, 8))
    np.testing.assert_array_equal(a[:300], es.device_samples(1000, 300, 5, 5))
    np.testing.assert_array_equal(L.epipolar_samples5(6, 64, seed=2 ** 40 + 1), es.device_samples(6, 64, 2 ** 40 + 1, 5))
    counts = np.bincount(L.epipolar_samples5(64, 4096, seed=0).ravel(), minlength=64)
    assert counts.min() > 0 and np.abs(counts - 320).max() < 90                                        # 320 each, sigma about 17.7


# ------------------------------------------------------------------------------------------------------------ solve
@pytest.mark.parametrize("sigma", [0.0, 0.5])
@pytest.mark.parametrize("H", [1, 63, 64, 65, 257])
def test_solve5_equals_the_restatement(L, solved, sigma, H):
    """The same solutions in the same slots: nsol, every slot within DEVICE_TOL of the restatement's slot (which makes the device's
    order the restatement's: ascending in the root), NaN in the others; every finite slot an essential matrix through the five
    matches.  Samples whose root count hangs on rounding are left out, and the restatement alone keeps them under 5 %."""
    s = solved[sigma]
    samples, skip = s["samples"][:H], s["skip"][:H]
    assert skip.sum() <= 0.05 * H
    G, nsol = L.epipolar_solve5(s["p1"], s["p2"], samples, F0, C0)
    assert G.shape == (H, 10, 3, 3) and nsol.shape == (H,) and nsol.dtype == np.int32
    a, b = es.normalise(s["p1"], K), es.normalise(s["p2"], K)
    worst, worst_residual = 0.0, 0.0
    for h in range(H):
        k = int(nsol[h])
        assert 0 <= k <= 10 and np.isfinite(G[h, :k]).all() and np.isnan(G[h, k:]).all()
        for F in G[h, :k]:
            E = es.to_essential(F, K)
            E = E / np.sqrt((E * E).sum())
            worst_residual = max(worst_residual, np.abs(es._design(a[samples[h]], b[samples[h]]) @ E.ravel()).max(), *es.essential_residuals(E))
            assert abs(np.sqrt((F * F).sum()) - 1.0) <= 1e-14
        if skip[h]:
            continue
        assert k == s["nsol"][h], f"sample {h}: {k} solutions, the restatement has {s['nsol'][h]}"
        if k:
            worst = max(worst, ec.sign_distance(G[h, :k], s["Fs"][h, :k]).max())
    print(f"sigma {sigma} H {H}: worst slot distance {worst}, worst constraint residual {worst_residual}, left out {skip.sum()}")
    assert worst <= es.DEVICE_TOL
    assert worst_residual <= CONSTRAINT_TOL
    if sigma == 0.0:
        near = np.array([ec.sign_distance(G[h, :nsol[h]], s["F"]).min() for h in range(H) if not skip[h] and nsol[h]])
        assert near.max() <= es.DEVICE_TOL                     # one solution of every sample is the truth


def test_solve5_degenerate_samples(L, solved):
    s = solved[0.5]
    samples = s["samples"][:70].copy()
    samples[3, 4] = samples[3, 1]                              # a repeated index
    samples[66, 0] = samples[66, 2]
    p1, p2 = s["p1"].copy(), s["p2"].copy()
    i, j = samples[40, 0], samples[40, 3]
    p1[j], p2[j] = p1[i], p2[i]                                # five points of which two coincide
    G, nsol = L.epipolar_solve5(p1, p2, samples, F0, C0)
    for h in (3, 40, 66):
        assert nsol[h] == 0 and np.isnan(G[h]).all()
        assert len(es.solve5(p1, p2, samples[h], K)) == 0
    touched = (samples == j).any(axis=1)
    touched[[3, 66]] = True
    clean = ~touched & ~s["skip"][:70]
    np.testing.assert_array_equal(nsol[clean], s["nsol"][:70][clean])
    counts, _ = L.epipolar_score(p1, p2, G.reshape(-1, 3, 3), 3.0)
    assert (counts.reshape(70, 10)[[3, 40, 66]] == 0).all()


# ------------------------------------------------------------------------------------------------------------ the whole filter
def assert_ransac_equal(got, want, what):
    info = got["info"]
    assert info["chosen"] == want["chosen"] and info["chosen_count"] == want["chosen_count"], what
    assert info["refit_counts"] == want["refit_counts"] and info["refits_run"] == len(want["refit_counts"]), what
    assert info["refits_kept"] == want["refits_kept"] and info["final_count"] == want["final_count"], what
    assert info["keep_all"] == want["keep_all"], what
    np.testing.assert_array_equal(got["mask"], want["mask"], err_msg=what)


@pytest.mark.parametrize("n,n_out,threshold,seed,planar", es.RANSAC5_SCENES)
def test_ransac5_equals_the_restatement(L, scenes, n, n_out, threshold, seed, planar):
    """The same samples -> the same chosen slot, the same count after each refit, the same mask.  No match lies within 1 % of
    threshold^2 under the restatement's final F (checked on the CPU), so none is excused.  Against the truth: every true inlier
    kept, at most 2 outliers kept, each within threshold of the true epipolar lines."""
    s = scenes[n]
    p1, p2, out, samples = s["p1"], s["p2"], s["out"], s["samples"]
    want = es.ransac5(p1, p2, samples, K, threshold, Fs=s["Fs"])
    e = es.errors(want["F"], p1, p2)
    assert not (np.abs(e - threshold ** 2) <= 0.01 * threshold ** 2).any()
    got = L.essential_ransac(p1, p2, F0, C0, threshold, samples=samples)
    assert_ransac_equal(got, want, f"scene({n}, {n_out})")
    # the final F itself: the last kept refit against the extended-precision refit on the set it summed over (the tolerance rule
    # of linalg_cases); without a kept refit it is the five-point solver's, held to the restatement as test_solve5_* hold every
    # sample whose root count does not hang on rounding
    d = ec.sign_distance(got["F"], want["F"])[0]
    exact = lg.whole_filter_reference(p1, p2, samples, want, threshold, K)
    if exact is not None:
        ref, kappa, family = exact
        d = ec.sign_distance(got["F"], ref["F"])[0]
        print("distance of the final F to the exact refit", d, "allowed", lg.tolerance(family, kappa))
        assert d <= lg.tolerance(family, kappa)
    else:
        print("distance of the final F to the restatement's", d)
        if not es.solve5_details(p1, p2, samples[want["chosen"] // 10][None], K)[0]["skip"]:
            assert d <= es.DEVICE_TOL
    np.testing.assert_array_equal(got["mask"], es.inliers(got["F"], p1, p2, threshold))
    assert max(es.essential_residuals(es.to_essential(got["F"], K))) <= 1e-9
    assert got["mask"][~out].all()
    kept = out & got["mask"]
    assert kept.sum() <= 2 and (es.errors(s["F"], p1, p2)[kept] <= threshold ** 2).all()
    for refits in (0, 1):
        got = L.essential_ransac(p1, p2, F0, C0, threshold, samples=samples, refits=refits)
        assert_ransac_equal(got, es.ransac5(p1, p2, samples, K, threshold, refits=refits, Fs=s["Fs"]), f"scene({n}, {n_out}) refits {refits}")


@pytest.mark.parametrize("n", [5, 6, 64, 513])
def test_ransac5_launch_seams(L, n):
    """n across the 512-match tile and at the least a sample needs, H = 1, 26 (260 slots cross the 256-hypothesis tile) and 257,
    splits forced to 1 and to the number of match tiles, refits 0 and 4.  At every shape the mask is inliers(F) bit for bit
    whatever the splits, and the chosen slot, the counts and the mask are the restatement's.  The scene and sample seeds are
    chosen on the restatement alone so that no shape needs an excuse (essential_cases.SEAM_SEEDS, choice_is_decided and
    path_is_decided, asserted here and on the CPU).  One thing is left out: with fewer than 8 inliers (n = 5 and 6, and the lone sample of n = 64) the
    refit's 9 x 9 matrix has more than one null vector and which of them comes out is not defined, so refits = 4 is then held
    to the restatement in the chosen slot and its count only."""
    p1, p2, all_samples, Fs_all = es.seam_case(n)
    tiles = (n + 511) // 512
    for H in es.SEAM_H:
        samples, Fs = all_samples[:H], Fs_all[:H]
        assert es.choice_is_decided(Fs, p1, p2, 3.0)
        for refits in (0, 4):
            want = es.ransac5(p1, p2, samples, K, 3.0, refits=refits, Fs=Fs)
            results = [L.essential_ransac(p1, p2, F0, C0, 3.0, samples=samples, refits=refits, splits=sp) for sp in (0, 1, tiles)]
            for got in results:
                assert got["info"]["hyp_tile"] == 256 and got["info"]["workgroups"] == (10 * H + 255) // 256 * got["info"]["splits"]
                np.testing.assert_array_equal(got["mask"], results[0]["mask"])
                np.testing.assert_array_equal(got["F"], results[0]["F"])
                assert got["info"]["chosen"] == results[0]["info"]["chosen"] and got["info"]["refit_counts"] == results[0]["info"]["refit_counts"]
            got = results[0]
            assert not got["info"]["keep_all"]
            np.testing.assert_array_equal(got["mask"], es.inliers(got["F"], p1, p2, 3.0))
            assert got["info"]["final_count"] == got["mask"].sum()
            what = f"n {n} H {H} refits {refits}"
            if refits == 0 or want["chosen_count"] >= 8:
                assert es.path_is_decided(want["path"], p1, p2, 3.0), what
                assert_ransac_equal(got, want, what)
            else:
                assert got["info"]["chosen"] == want["chosen"] and got["info"]["chosen_count"] == want["chosen_count"], what


def test_ransac5_own_draws(L):
    """samples=None draws what alp_epipolar_samples5 draws, whatever the forced splits (1 500 matches: three match tiles); the low
    inlier share, 0.3, at the truth checks of the CPU test"""
    n, n_out, threshold = 1500, 1050, 3.0
    p1, p2, F_true, out = es.scene(n, n_out, 0.5, 2)
    samples = L.epipolar_samples5(n, 4096, seed=9)
    want = L.essential_ransac(p1, p2, F0, C0, threshold, samples=samples)
    for splits in (0, 1, 2, 3):
        got = L.essential_ransac(p1, p2, F0, C0, threshold, hypotheses=4096, seed=9, splits=splits)
        assert got["info"]["chosen"] == want["info"]["chosen"] and got["info"]["refit_counts"] == want["info"]["refit_counts"]
        np.testing.assert_array_equal(got["mask"], want["mask"])
        np.testing.assert_array_equal(got["F"], want["F"])
    np.testing.assert_array_equal(want["mask"], es.inliers(want["F"], p1, p2, threshold))
    assert want["mask"][~out].mean() > 0.98 and want["mask"][out].mean() < 0.03
    kept = out & want["mask"]
    assert (np.sqrt(es.errors(F_true, p1, p2)[kept]) <= 2 * threshold).all()          # what is kept of the outliers lies near the true lines
    other = L.essential_ransac(p1, p2, F0, C0, threshold, hypotheses=4096, seed=10)
    assert other["info"]["chosen"] != want["info"]["chosen"]


def test_ransac5_keeps_everything_without_a_finite_slot(L):
    p1, p2, _, _ = es.scene(12, 0, 0.5, 3)
    samples = np.tile(np.array([0, 1, 2, 3, 3], dtype=np.int32), (8, 1))
    got = L.essential_ransac(p1, p2, F0, C0, 3.0, samples=samples)
    assert got["info"]["keep_all"] and got["mask"].all() and got["info"]["chosen_count"] == 0 and got["info"]["chosen"] == 0
    assert got["info"]["refits_run"] == 0 and got["info"]["refit_counts"] == [] and np.isnan(got["F"]).all()
    from alproj_amd import gcp
    mask, F, info = gcp.filter_geometric(p1, p2, method="essential", threshold=3.0, samples=samples, focal_length=F0, principal_point=C0,
                                         return_model=True)
    assert mask.all() and mask.dtype == bool and info["keep_all"]


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer_equals_the_restatement(L, scenes):
    """int32 points as match_keypoints returns them, K from params as image_match derives it"""
    from alproj_amd import gcp
    s = scenes[es.RANSAC5_SCENES[0][0]]
    q1, q2 = np.float32(s["p1"]).astype("int32"), np.float32(s["p2"]).astype("int32")
    r1, r2 = q1.astype(np.float64), q2.astype(np.float64)
    samples = s["samples"][:512]
    fov = 2.0 * np.degrees(np.arctan((es.WIDTH / 2) / es.FOCAL))
    params = {"fov": fov, "w": es.WIDTH, "h": es.HEIGHT}
    f = (es.WIDTH / 2) / np.tan(fov * np.pi / 180 / 2)
    Kp = (f, es.WIDTH / 2, es.HEIGHT / 2)
    want = es.ransac5(r1, r2, samples, Kp, 3.0)
    e = es.errors(want["F"], r1, r2)
    assert not (np.abs(e - 9.0) <= 0.09).any()
    mask, F, info = gcp.filter_geometric(q1, q2, method="essential", threshold=3.0, samples=samples, focal_length=f,
                                         image_size=(es.WIDTH, es.HEIGHT), return_model=True)
    np.testing.assert_array_equal(mask, want["mask"])
    assert info["chosen"] == want["chosen"] and info["final_count"] == want["final_count"] == mask.sum()
    np.testing.assert_allclose(info["E"], es.to_essential(F, Kp), rtol=0, atol=0)
    assert ec.sign_distance(F, want["F"])[0] <= 1e-9
    for grid in (None, 100):
        got = gcp.filter_matches(q1, q2, (es.WIDTH, es.HEIGHT), outlier_filter="essential", threshold=3.0, spatial_thin_grid=grid,
                                 params=params, samples=samples)
        a, b = q1[want["mask"]], q2[want["mask"]]
        if grid is not None:
            thin = gcp.filter_spatial(a, grid, (es.WIDTH, es.HEIGHT))
            a, b = a[thin], b[thin]
        pd.testing.assert_frame_equal(got, pd.DataFrame(np.hstack((a, b)), columns=["u_org", "v_org", "u_sim", "v_sim"]))
    again = gcp.filter_geometric(q1, q2, method="essential", threshold=3.0, hypotheses=2048, seed=2, focal_length=f)
    np.testing.assert_array_equal(again, gcp.filter_geometric(q1, q2, method="essential", threshold=3.0, hypotheses=2048, seed=2, focal_length=f))
    assert again[~s["out"]].mean() > 0.9 and again[s["out"]].mean() < 0.05


def test_entry_point_refusals(L):
    lib = L.lib()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    p = np.ascontiguousarray(np.random.default_rng(0).uniform(0, 100, (16, 2)))
    P = p.ctypes.data_as(dp)
    s = np.tile(np.arange(5, dtype=np.int32), (4, 1))
    S = s.ctypes.data_as(ip)
    F = np.zeros((4, 90))
    Kc = (ctypes.c_double * 3)(1000.0, 50.0, 50.0)
    out_i = np.zeros(32, dtype=np.int32)
    out_u8 = np.zeros(16, dtype=np.uint8)
    U8 = out_u8.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    EINVAL = -1

    def refused(rc, text):
        assert rc == EINVAL, (rc, text)
        assert text in lib.alp_last_error().decode(), (lib.alp_last_error(), text)

    refused(lib.alp_epipolar_samples5(4, 4, 0, out_i.ctypes.data_as(ip)), "n must be 5..2^20")
    refused(lib.alp_epipolar_samples5(5, 0, 0, out_i.ctypes.data_as(ip)), "H must be 1..2^20")
    refused(lib.alp_epipolar_samples5(5, 4, 0, None), "NULL")
    refused(lib.alp_epipolar_solve5(P, P, 4, S, 4, Kc, F.ctypes.data_as(dp), out_i.ctypes.data_as(ip)), "must be 5..2^20")
    refused(lib.alp_epipolar_solve5(None, P, 16, S, 4, Kc, F.ctypes.data_as(dp), out_i.ctypes.data_as(ip)), "NULL")
    refused(lib.alp_epipolar_solve5(P, P, 16, S, 4, Kc, F.ctypes.data_as(dp), None), "NULL")
    refused(lib.alp_epipolar_solve5(P, P, 16, S, 4, None, F.ctypes.data_as(dp), out_i.ctypes.data_as(ip)), "NULL K")
    refused(lib.alp_epipolar_solve5(P, P, 16, S, 2 ** 20 // 10 + 1, Kc, F.ctypes.data_as(dp), out_i.ctypes.data_as(ip)), "H = 104858")
    for bad in (16, -1):
        t = s.copy()
        t[2, 3] = bad
        refused(lib.alp_epipolar_solve5(P, P, 16, t.ctypes.data_as(ip), 4, Kc, F.ctypes.data_as(dp), out_i.ctypes.data_as(ip)), "sample 3 of hypothesis 2")
        refused(lib.alp_essential_ransac(P, P, 16, t.ctypes.data_as(ip), 4, 0, Kc, 3.0, 4, 0, None, U8, None), "sample 3 of hypothesis 2")
    for f in (0.0, -1.0, float("nan"), float("inf")):
        refused(lib.alp_essential_ransac(P, P, 16, None, 4, 0, (ctypes.c_double * 3)(f, 50.0, 50.0), 3.0, 4, 0, None, U8, None), "focal length")
    refused(lib.alp_essential_ransac(P, P, 16, None, 4, 0, (ctypes.c_double * 3)(1000.0, float("nan"), 50.0), 3.0, 4, 0, None, U8, None), "principal point")
    refused(lib.alp_essential_ransac(P, P, 16, None, 4, 0, None, 3.0, 4, 0, None, U8, None), "NULL K")
    refused(lib.alp_essential_ransac(P, P, 4, None, 4, 0, Kc, 3.0, 4, 0, None, U8, None), "must be 5..2^20")
    refused(lib.alp_essential_ransac(P, None, 16, None, 4, 0, Kc, 3.0, 4, 0, None, U8, None), "NULL")
    refused(lib.alp_essential_ransac(P, P, 16, None, 4, 0, Kc, 3.0, 9, 0, None, U8, None), "refits must be 0..8")
    refused(lib.alp_essential_ransac(P, P, 16, None, 4, 0, Kc, float("inf"), 4, 0, None, U8, None), "threshold")
    refused(lib.alp_essential_ransac(P, P, 16, None, 4, 0, Kc, 3.0, 4, 2, None, U8, None), "only 1 tiles")
    refused(lib.alp_essential_ransac(P, P, 16, None, 0, 0, Kc, 3.0, 4, 0, None, U8, None), "H = 0")
    # 10 * H * n above 2^35: refused on the sizes alone, before any array is read
    refused(lib.alp_essential_ransac(P, P, 2 ** 20, None, 2 ** 13, 0, Kc, 3.0, 4, 0, None, U8, None), "passes 2^35")
    # every output of the whole filter may be NULL
    assert lib.alp_essential_ransac(P, P, 16, None, 4, 0, Kc, 3.0, 4, 0, None, None, None) == 0
