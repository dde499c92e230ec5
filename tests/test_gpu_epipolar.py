"""GPU: the geometric match filter (alp_epipolar_samples / _solve8 / _score / _mask / _ransac), the grid thinning (alp_grid_thin)
and the Python layer over them (alproj_amd.gcp.filter_geometric / filter_spatial / filter_matches) against the numpy restatement
of tests/epipolar_cases.py, the truth of its synthetic scenes, and the reference's own _filter_spatial (tests/golden/g21).

what can go wrong                                             where it is held
a repeated or out-of-range sample index, a seed ignored       test_samples_*
the null vector, rank 2, the denormalisation                  test_solve_recovers_the_truth, test_solve_equals_the_restatement
the error expression's order, the one-division inlier test    test_score_and_mask_bit_for_bit (counts, mask and err: bit equality)
partial tiles of matches and hypotheses, the split merge      test_score_launch_seams, test_score_splits_give_one_answer,
                                                              test_score_beyond_one_wave_of_workgroups
NaN hypotheses, a match exactly on the threshold              test_score_edges
selection, the refit loop and its stop, the final mask        test_ransac_equals_the_restatement (and the truth), test_ransac_large_n
the final F itself, the solve and the refit case by case      test_ransac_equals_the_restatement, tests/test_gpu_epipolar_linalg.py
the device's own draws, too few inliers                       test_ransac_own_draws, test_ransac_keeps_everything_without_eight_inliers
ties and order in the thinning, the rounded root              test_filter_spatial_equals_the_reference, test_grid_thin_edges
lines 507-544 as a whole, refusals of the C entry points      test_filter_matches_reproduces_the_reference_lines, test_entry_point_refusals
the one driver of the four whole filters: text and order      test_whole_filters_refuse_alike
of its refusals

What makes no device call (refusals and edge cases of the Python layer, selection="random") needs no GPU: tests/test_epipolar_cases.py.
"""
import ctypes
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
import linalg_cases as lg  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_filter_spatial.npz")
NAN_F = np.full((3, 3), np.nan)


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def noisy():
    """scene(500, 200, 0.5), 2048 numpy-drawn samples and the restatement's F of each: computed once, shared, never changed"""
    n, n_out, _, seed = ec.RANSAC_SCENES[0]
    p1, p2, F, out = ec.scene(n, n_out, 0.5, seed)
    samples = ec.draw_samples(n, 2048, 1000 + seed)
    Fs = ec.solve8_all(p1, p2, samples)
    return {"p1": p1, "p2": p2, "F": F, "out": out, "samples": samples, "Fs": Fs}


# ------------------------------------------------------------------------------------------------------------ samples
@pytest.mark.parametrize("n", [8, 9, 64, 1000])
def test_samples_rows_are_distinct_and_in_range(L, n):
    s = L.epipolar_samples(n, 2048, seed=3)
    assert s.shape == (2048, 8) and s.dtype == np.int32
    assert s.min() >= 0 and s.max() < n
    assert (np.diff(np.sort(s, axis=1), axis=1) > 0).all()
    if n == 8:
        assert (np.sort(s, axis=1) == np.arange(8)).all() and len(np.unique(s, axis=0)) > 1000         # permutations, not one row


def test_samples_are_a_function_of_the_seed_and_the_hypothesis(L):
    a = L.epipolar_samples(1000, 4096, seed=5)
    np.testing.assert_array_equal(a, L.epipolar_samples(1000, 4096, seed=5))
    for H in (1, 63, 257):                                     # another launch shape: the same rows
        np.testing.assert_array_equal(L.epipolar_samples(1000, H, seed=5), a[:H])
    for seed in (6, 5 + 2 ** 32):                              # both words of the seed count
        assert (L.epipolar_samples(1000, 4096, seed=seed) != a).any(axis=1).mean() > 0.99
    assert len(np.unique(a, axis=0)) == 4096


def test_samples_draw_every_index(L):
    s = L.epipolar_samples(64, 4096, seed=0)
    counts = np.bincount(s.ravel(), minlength=64)
    assert counts.min() > 0
    # 32 768 draws over 64 indices: 512 each, standard deviation about 22.5; five of them
    assert np.abs(counts - 512).max() < 113


# ------------------------------------------------------------------------------------------------------------ solve
def test_solve_recovers_the_truth(L):
    """Noise-free: every sample's F is +-F_true within 1e-9 (numpy's SVD route: 8.5e-13 on such samples, ill-conditioned ones
    included) and singular."""
    p1, p2, F, _ = ec.scene(200, 0, 0.0, 1)
    G = L.epipolar_solve8(p1, p2, ec.draw_samples(200, 2000, 5))
    d = ec.sign_distance(G, F)
    print("worst distance to the truth", d.max(), "worst |det|", np.abs(np.linalg.det(G)).max())
    assert d.max() <= 1e-9
    assert np.abs(np.linalg.det(G)).max() <= 1e-12


def test_solve_equals_the_restatement(L, noisy):
    samples = noisy["samples"].copy()
    samples[100, 7] = samples[100, 2]                          # a repeated point: rank 7
    G = L.epipolar_solve8(noisy["p1"], noisy["p2"], samples)
    keep = np.arange(len(samples)) != 100
    d = ec.sign_distance(G[keep], noisy["Fs"][keep])
    print("worst distance to the restatement", d.max())
    assert d.max() <= 1e-7
    np.testing.assert_allclose(np.sqrt((G[keep] ** 2).sum(axis=(1, 2))), 1.0, rtol=0, atol=1e-14)
    assert np.isnan(G[100]).all() and np.isnan(ec.solve8(noisy["p1"], noisy["p2"], samples[100])).all()
    counts, _ = L.epipolar_score(noisy["p1"], noisy["p2"], G, 3.0)
    assert counts[100] == 0
    np.testing.assert_array_equal(counts, ec.counts(G, noisy["p1"], noisy["p2"], 3.0))


# ------------------------------------------------------------------------------------------------------------ score
def hypotheses(noisy, H):
    """H matrices from the restatement, every 50th one NaN"""
    Fs = noisy["Fs"][np.arange(H) % len(noisy["Fs"])].copy()
    Fs[7::50] = np.nan
    return Fs


def test_score_and_mask_bit_for_bit(L, noisy):
    p1, p2 = noisy["p1"], noisy["p2"]
    Fs = hypotheses(noisy, 300)
    for threshold in (3.0, 10.0, 0.5):
        counts, _ = L.epipolar_score(p1, p2, Fs, threshold)
        np.testing.assert_array_equal(counts, ec.counts(Fs, p1, p2, threshold))
    for F in (Fs[0], Fs[1], noisy["F"], NAN_F):
        mask, err = L.epipolar_mask(p1, p2, F, 3.0)
        np.testing.assert_array_equal(err, ec.errors(F, p1, p2))
        np.testing.assert_array_equal(mask, ec.inliers(F, p1, p2, 3.0))


def scene_of(n):
    p1, p2, _, _ = ec.scene(n, n // 3, 0.5, 100 + n)
    return p1, p2


def test_score_launch_seams(L, noisy):
    _, info = L.epipolar_score(noisy["p1"], noisy["p2"], noisy["Fs"][:1], 3.0)
    tile, htile = info["match_tile"], info["hyp_tile"]
    assert tile >= 64 and htile >= 64
    ns = sorted({8, 9, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 1})
    for n in ns:
        p1, p2 = scene_of(n)
        Fs = hypotheses(noisy, htile + 1)
        counts, info = L.epipolar_score(p1, p2, Fs, 40.0)
        np.testing.assert_array_equal(counts, ec.counts(Fs, p1, p2, 40.0), err_msg=f"n = {n}")
        assert info["match_tiles"] == -(-n // tile) and 1 <= info["splits"] <= info["match_tiles"]
    p1, p2 = scene_of(2 * tile + 1)
    for H in sorted({1, 63, 64, 65, 257, htile - 1, htile, 2 * htile + 1}):
        Fs = hypotheses(noisy, H)
        counts, info = L.epipolar_score(p1, p2, Fs, 40.0)
        np.testing.assert_array_equal(counts, ec.counts(Fs, p1, p2, 40.0), err_msg=f"H = {H}")
        assert info["workgroups"] == -(-H // htile) * info["splits"]


def test_score_splits_give_one_answer(L, noisy):
    _, info = L.epipolar_score(noisy["p1"], noisy["p2"], noisy["Fs"][:1], 3.0)
    tile = info["match_tile"]
    p1, p2 = scene_of(7 * tile - 5)
    Fs = hypotheses(noisy, 300)
    want = ec.counts(Fs, p1, p2, 25.0)
    assert want.max() > want.min()
    for splits in (0, 1, 2, 3, 7):
        counts, info = L.epipolar_score(p1, p2, Fs, 25.0, splits=splits)
        np.testing.assert_array_equal(counts, want, err_msg=f"splits = {splits}")
        assert splits == 0 or info["splits"] == splits
    with pytest.raises(L.AlprojHipError, match="only 7 tiles"):
        L.epipolar_score(p1, p2, Fs, 25.0, splits=8)


def test_score_beyond_one_wave_of_workgroups(L, noisy):
    """600 000 hypotheses of 256 per workgroup: 2344 workgroups, more than 256 CUs hold at once at 8 per CU"""
    p1, p2 = scene_of(64)
    base = hypotheses(noisy, 300)
    want = ec.counts(base, p1, p2, 40.0)
    H = 600000
    counts, info = L.epipolar_score(p1, p2, base[np.arange(H) % 300], 40.0)
    assert info["workgroups"] > 2048
    np.testing.assert_array_equal(counts, want[np.arange(H) % 300])


def test_score_edges(L):
    """F of a pure x translation: e = (y2 - y1)^2 exactly on integer coordinates.  A match exactly on the threshold is an inlier,
    one past it is not; a NaN F, and an F whose lines vanish, count nothing."""
    F = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    p1 = np.array([[10, 20], [5, 7], [0, 0], [3, 3], [8, 1], [40, 40], [7, 70], [1, 2], [2, 1]], dtype=np.float64)
    dy = np.array([3, 0, -2, 2, -3, 1, 4, -1, 2], dtype=np.float64)
    p2 = p1 + np.stack([np.arange(9.0) * 11 - 30, dy], axis=1)
    counts, _ = L.epipolar_score(p1, p2, np.stack([F, NAN_F, 2.0 * F, np.zeros((3, 3)), -F]), 2.0)
    assert counts.tolist() == [6, 0, 6, 0, 6]
    mask, err = L.epipolar_mask(p1, p2, F, 2.0)
    np.testing.assert_array_equal(err, dy * dy)
    np.testing.assert_array_equal(mask, np.abs(dy) <= 2)
    assert not L.epipolar_mask(p1, p2, F, np.nextafter(2.0, 0.0))[0][np.abs(dy) == 2].any()
    assert L.epipolar_mask(p1, p2, F, 0.0)[0].tolist() == (dy == 0).tolist()
    mask, err = L.epipolar_mask(p1, p2, np.zeros((3, 3)), 1e300)
    assert np.isnan(err).all() and not mask.any()


# ------------------------------------------------------------------------------------------------------------ ransac
def assert_ransac_equal(got, want, what):
    info = got["info"]
    assert info["chosen"] == want["chosen"] and info["chosen_count"] == want["chosen_count"], what
    assert info["refit_counts"] == want["refit_counts"] and info["refits_run"] == len(want["refit_counts"]), what
    assert info["refits_kept"] == want["refits_kept"] and info["final_count"] == want["final_count"], what
    assert info["keep_all"] == want["keep_all"], what
    np.testing.assert_array_equal(got["mask"], want["mask"], err_msg=what)


@pytest.mark.parametrize("n,n_out,threshold,seed", ec.RANSAC_SCENES)
def test_ransac_equals_the_restatement(L, n, n_out, threshold, seed):
    """The same samples -> the same chosen hypothesis, the same count after each refit, the same mask.  No match lies within
    1 % of threshold^2 under the restatement's final F (checked on the CPU: none within 5 %), so none is excused.  Against the
    truth: every true inlier kept, at most 2 outliers kept, each within threshold of the true epipolar lines."""
    p1, p2, F_true, out = ec.scene(n, n_out, 0.5, seed)
    samples = ec.draw_samples(n, 2048, 1000 + seed)
    want = ec.ransac(p1, p2, samples, threshold)
    e = ec.errors(want["F"], p1, p2)
    assert not (np.abs(e - threshold ** 2) <= 0.01 * threshold ** 2).any()
    got = L.epipolar_ransac(p1, p2, threshold, samples=samples)
    assert_ransac_equal(got, want, f"scene({n}, {n_out})")
    # the final F itself: the last kept refit against the extended-precision refit on the set it summed over, or the chosen
    # sample's solve against the extended-precision solve, at the tolerance rule of linalg_cases
    ref, kappa, family = lg.whole_filter_reference(p1, p2, samples, want, threshold)
    d = ec.sign_distance(got["F"], ref["F"])[0]
    print("distance of the final F to the restatement's", ec.sign_distance(got["F"], want["F"])[0], "to the exact one", d,
          "allowed", lg.tolerance(family, kappa), family)
    assert d <= lg.tolerance(family, kappa)
    np.testing.assert_array_equal(got["mask"], ec.inliers(got["F"], p1, p2, threshold))
    assert got["mask"][~out].all()
    kept = out & got["mask"]
    assert kept.sum() <= 2 and (ec.errors(F_true, p1, p2)[kept] <= threshold ** 2).all()
    for refits in (0, 1):
        got = L.epipolar_ransac(p1, p2, threshold, samples=samples, refits=refits)
        assert_ransac_equal(got, ec.ransac(p1, p2, samples, threshold, refits=refits), f"scene({n}, {n_out}) refits {refits}")


def test_ransac_large_n(L):
    """70 001 matches: more than the 256 workgroups of the refit's reductions cover in one stride, 137 match tiles in splits"""
    n = 70001
    p1, p2, _, out = ec.scene(n, 20000, 0.5, 4)
    samples = ec.draw_samples(n, 256, 11)
    want = ec.ransac(p1, p2, samples, 3.0)
    e = ec.errors(want["F"], p1, p2)
    excused = np.abs(e - 9.0) <= 0.09
    got = L.epipolar_ransac(p1, p2, 3.0, samples=samples)
    assert got["info"]["reduce_blocks"] == 256 and got["info"]["splits"] > 1
    assert got["info"]["chosen"] == want["chosen"] and got["info"]["chosen_count"] == want["chosen_count"]
    assert not excused.any()
    assert_ransac_equal(got, want, "70 001 matches")
    assert got["mask"][~out].mean() > 0.999 and got["mask"][out].mean() < 0.02


def test_ransac_own_draws(L):
    """samples=None draws what alp_epipolar_samples draws, whatever the forced splits (1 500 matches: three match tiles)"""
    n, n_out, threshold = 1500, 600, 3.0
    p1, p2, _, out = ec.scene(n, n_out, 0.5, 2)
    samples = L.epipolar_samples(n, 4096, seed=9)
    want = L.epipolar_ransac(p1, p2, threshold, samples=samples)
    for splits in (0, 1, 2, 3):
        got = L.epipolar_ransac(p1, p2, threshold, hypotheses=4096, seed=9, splits=splits)
        assert got["info"]["chosen"] == want["info"]["chosen"] and got["info"]["refit_counts"] == want["info"]["refit_counts"]
        np.testing.assert_array_equal(got["mask"], want["mask"])
        np.testing.assert_array_equal(got["F"], want["F"])
    assert want["mask"][~out].mean() > 0.98 and want["mask"][out].mean() < 0.03
    other = L.epipolar_ransac(p1, p2, threshold, hypotheses=4096, seed=10)
    assert other["info"]["chosen"] != want["info"]["chosen"]


def test_ransac_keeps_everything_without_eight_inliers(L):
    rng = np.random.default_rng(12)
    p1, p2 = rng.uniform(0, 1000, (12, 2)), rng.uniform(0, 1000, (12, 2))
    got = L.epipolar_ransac(p1, p2, 0.01, hypotheses=512, seed=1)
    assert got["info"]["keep_all"] and got["mask"].all() and got["info"]["chosen_count"] < 8
    assert got["info"]["refits_run"] == 0 and got["info"]["refit_counts"] == []
    from alproj_amd import gcp
    mask, F, info = gcp.filter_geometric(p1, p2, threshold=0.01, hypotheses=512, return_model=True)
    assert mask.all() and mask.dtype == bool and info["keep_all"]


# ------------------------------------------------------------------------------------------------------------ thinning
def test_filter_spatial_equals_the_reference(L):
    from alproj_amd import gcp
    g = np.load(GOLDEN)
    seen = {"first": 0, "center": 0}
    for k in range(int(g["n_cases"])):
        sel = str(g[f"sel{k}"])
        if sel == "random":
            continue
        grid, w, h, _ = g[f"args{k}"]
        got = gcp.filter_spatial(g[f"pts{k}"], int(grid) if grid == int(grid) else float(grid), (int(w), int(h)), sel)
        np.testing.assert_array_equal(got, g[f"mask{k}"], err_msg=f"case {k}: {sel}, grid {grid}")
        assert got.dtype == bool
        seen[sel] += 1
    assert seen["first"] >= 12 and seen["center"] >= 14


def test_grid_thin_edges(L):
    cell = np.array([5, -3, 5, 2 ** 40, -3, 2 ** 40 + 7, 5], dtype=np.int64)
    with pytest.raises(L.AlprojHipError, match="2\\^26"):
        L.grid_thin(cell)
    cell = np.array([5, -3, 5, -3 + 2 ** 26 - 1, -3, 0, 5], dtype=np.int64)
    assert L.grid_thin(cell).tolist() == [True, True, False, True, False, True, False]
    dist = np.array([2.0, 1.0, 0.0, 9.0, 1.0, np.inf, -0.0])
    assert L.grid_thin(cell, dist).tolist() == [False, True, True, True, False, True, False]
    for bad in (np.nan, -1e-300):
        d = dist.copy()
        d[4] = bad
        with pytest.raises(L.AlprojHipError, match=r"dist\[4\]"):
            L.grid_thin(cell, d)
    assert L.grid_thin(np.zeros(0, dtype=np.int64)).shape == (0,)
    # many points, few cells, more than one workgroup: the lowest index of each cell, and the lowest of the minima
    rng = np.random.default_rng(0)
    cell = rng.integers(-50, 50, 100001)
    dist = rng.integers(0, 40, 100001).astype(np.float64)
    first = np.zeros(len(cell), dtype=bool)
    first[np.unique(cell, return_index=True)[1]] = True
    np.testing.assert_array_equal(L.grid_thin(cell), first)
    frame = pd.DataFrame({"cell": cell, "dist": dist})
    want = np.zeros(len(cell), dtype=bool)
    want[frame.groupby("cell")["dist"].idxmin().to_numpy()] = True
    np.testing.assert_array_equal(L.grid_thin(cell, dist), want)


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_filter_matches_reproduces_the_reference_lines(L):
    """image_match lines 507-544 restated with the two masks: int32 points as match_keypoints returns them"""
    from alproj_amd import gcp
    p1, p2, _, out = ec.scene(400, 150, 0.5, 21)
    q1, q2 = np.float32(p1).astype("int32"), np.float32(p2).astype("int32")
    samples = ec.draw_samples(400, 1024, 5)
    for grid, sel, state in ((None, "first", None), (100, "first", None), (64, "center", None), (150, "random", 4)):
        got = gcp.filter_matches(q1, q2, (ec.WIDTH, ec.HEIGHT), threshold=3.0, spatial_thin_grid=grid, spatial_thin_selection=sel,
                                 spatial_thin_random_state=state, samples=samples)
        mask = gcp.filter_geometric(q1, q2, threshold=3.0, samples=samples)
        np.testing.assert_array_equal(mask, L.epipolar_ransac(q1.astype(np.float64), q2.astype(np.float64), 3.0, samples=samples)["mask"])
        a, b = q1[mask], q2[mask]
        if grid is not None:
            thin = gcp.filter_spatial(a, grid, (ec.WIDTH, ec.HEIGHT), sel, state)
            a, b = a[thin], b[thin]
        want = pd.DataFrame(np.hstack((a, b)), columns=["u_org", "v_org", "u_sim", "v_sim"])
        pd.testing.assert_frame_equal(got, want)
        assert 0 < len(got) <= mask.sum() and mask[~out].mean() > 0.9 and mask[out].mean() < 0.05
    mask, F, info = gcp.filter_geometric(q1, q2, threshold=3.0, hypotheses=2048, seed=2, return_model=True)
    again = gcp.filter_geometric(q1, q2, threshold=3.0, hypotheses=2048, seed=2)
    np.testing.assert_array_equal(mask, again)
    assert F.shape == (3, 3) and info["final_count"] == mask.sum() and not info["keep_all"]
    np.testing.assert_array_equal(mask, ec.inliers(F, q1.astype(np.float64), q2.astype(np.float64), 3.0))


def test_entry_point_refusals(L):
    lib = L.lib()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    p = np.ascontiguousarray(np.random.default_rng(0).uniform(0, 100, (16, 2)))
    P = p.ctypes.data_as(dp)
    s = np.tile(np.arange(8, dtype=np.int32), (4, 1))
    S = s.ctypes.data_as(ip)
    F = np.zeros((4, 9))
    out_i = np.zeros(32, dtype=np.int32)
    out_u8 = np.zeros(16, dtype=np.uint8)
    U8 = out_u8.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    EINVAL = -1

    def refused(rc, text):
        assert rc == EINVAL, (rc, text)
        assert text in lib.alp_last_error().decode(), (lib.alp_last_error(), text)

    refused(lib.alp_epipolar_samples(7, 4, 0, out_i.ctypes.data_as(ip)), "n must be 8..2^20")
    refused(lib.alp_epipolar_samples(2 ** 20 + 1, 4, 0, out_i.ctypes.data_as(ip)), "n must be 8..2^20")
    refused(lib.alp_epipolar_samples(8, 0, 0, out_i.ctypes.data_as(ip)), "H must be 1..2^20")
    refused(lib.alp_epipolar_samples(8, 4, 0, None), "NULL")
    refused(lib.alp_epipolar_solve8(None, P, 16, S, 4, F.ctypes.data_as(dp)), "NULL")
    refused(lib.alp_epipolar_solve8(P, P, 16, None, 4, F.ctypes.data_as(dp)), "NULL")
    refused(lib.alp_epipolar_solve8(P, P, 7, S, 4, F.ctypes.data_as(dp)), "must be 8..2^20")
    for bad in (16, -1):
        t = s.copy()
        t[2, 5] = bad
        refused(lib.alp_epipolar_solve8(P, P, 16, t.ctypes.data_as(ip), 4, F.ctypes.data_as(dp)), "sample 5 of hypothesis 2")
        refused(lib.alp_epipolar_ransac(P, P, 16, t.ctypes.data_as(ip), 4, 0, 3.0, 4, 0, None, U8, None), "sample 5 of hypothesis 2")
    refused(lib.alp_epipolar_score(P, P, 16, None, 4, 3.0, 0, out_i.ctypes.data_as(ip), None), "NULL")
    refused(lib.alp_epipolar_score(P, P, 16, F.ctypes.data_as(dp), 4, float("nan"), 0, out_i.ctypes.data_as(ip), None), "threshold")
    refused(lib.alp_epipolar_score(P, P, 16, F.ctypes.data_as(dp), 4, 3.0, 2, out_i.ctypes.data_as(ip), None), "only 1 tiles")
    refused(lib.alp_epipolar_score(P, P, 16, F.ctypes.data_as(dp), 4, 3.0, -1, out_i.ctypes.data_as(ip), None), "splits is negative")
    refused(lib.alp_epipolar_score(P, P, 16, F.ctypes.data_as(dp), 2 ** 20 + 1, 3.0, 0, out_i.ctypes.data_as(ip), None), "H = 1048577")
    # H * n above 2^35: refused on the sizes alone, before any array is read
    refused(lib.alp_epipolar_score(P, P, 2 ** 15 + 1, F.ctypes.data_as(dp), 2 ** 20, 3.0, 0, out_i.ctypes.data_as(ip), None), "passes 2^35")
    refused(lib.alp_epipolar_ransac(P, P, 2 ** 20, None, 2 ** 16, 0, 3.0, 4, 0, None, U8, None), "passes 2^35")
    refused(lib.alp_epipolar_mask(P, P, 16, None, 3.0, U8, None), "NULL")
    refused(lib.alp_epipolar_mask(P, P, 16, F.ctypes.data_as(dp), -1.0, U8, None), "threshold")
    refused(lib.alp_epipolar_ransac(P, None, 16, None, 4, 0, 3.0, 4, 0, None, U8, None), "NULL")
    refused(lib.alp_epipolar_ransac(P, P, 16, None, 4, 0, 3.0, 9, 0, None, U8, None), "refits must be 0..8")
    refused(lib.alp_epipolar_ransac(P, P, 16, None, 4, 0, float("inf"), 4, 0, None, U8, None), "threshold")
    refused(lib.alp_epipolar_ransac(P, P, 16, None, 0, 0, 3.0, 4, 0, None, U8, None), "H = 0")
    cell = np.zeros(4, dtype=np.int64)
    refused(lib.alp_grid_thin(None, None, 4, U8), "NULL")
    refused(lib.alp_grid_thin(cell.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None, -1, U8), "n must be 0..2^30")
    # every output of the whole filter may be NULL
    assert lib.alp_epipolar_ransac(P, P, 16, None, 4, 0, 3.0, 4, 0, None, None, None) == 0


FILTER_ENTRY_POINTS = {          # name -> (minimal sample, the text of its H range)
    "alp_epipolar_ransac": (8, "2^20"),
    "alp_essential_ransac": (5, "2^20 / 10"),
    "alp_epipolar_lmeds": (8, "2^20"),
    "alp_essential_lmeds": (5, "2^20 / 10"),
}


@pytest.mark.parametrize("name", FILTER_ENTRY_POINTS)
def test_whole_filters_refuse_alike(L, name):
    """The four whole filters share one driver: each refuses the common bad arguments with ALP_EINVAL and the one message, under
    its own name, before anything is launched; and of several bad arguments it names the first in the order points, rank
    (LMedS), K (essential), the criterion's numbers, refits, splits, samples."""
    lib = L.lib()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    width, h_range = FILTER_ENTRY_POINTS[name]
    p = np.ascontiguousarray(np.random.default_rng(0).uniform(0, 100, (513, 2)))
    P = p.ctypes.data_as(dp)
    lmeds, essential = name.endswith("lmeds"), "essential" in name
    s = np.tile(np.arange(width, dtype=np.int32), (4, 1))
    s[2, 3] = 16
    bad_samples = s.ctypes.data_as(ip)

    def refused(text, p1=P, n=16, samples=None, H=4, refits=4, splits=0, rank=width + 1, focal=800.0, number=None):
        K = [np.array([focal, 50.0, 50.0]).ctypes.data_as(dp)] if essential else []
        # the criterion's numbers: (rank, scale2, floor2) or the threshold; `number` replaces scale2 or the threshold
        criterion = [rank, 14.0 if number is None else number, 1.0] if lmeds else [3.0 if number is None else number]
        rc = getattr(lib, name)(p1, P, n, samples, H, 0, *K, *criterion, refits, splits, None, None, None, *([None] if lmeds else []))
        assert rc == -1, (rc, text)
        assert lib.alp_last_error().decode() == f"{name}: {text}"

    refused(f"n = {width - 1}, must be {width}..2^20", n=width - 1)
    refused(f"H = 0, must be 1..{h_range}", H=0)
    refused("refits must be 0..8", refits=9)
    refused("splits = 3, but 513 matches are only 2 tiles of 512", n=513, splits=3)
    refused("sample 3 of hypothesis 2 is 16, outside 0..15", samples=bad_samples)
    refused("NULL input", p1=None)
    # the order: every argument after the one named is bad as well
    later = dict(samples=bad_samples)
    refused("splits = 3, but 16 matches are only 1 tiles of 512", splits=3, **later)
    later.update(splits=3)
    refused("refits must be 0..8", refits=9, **later)
    later.update(refits=9)
    refused(("scale2" if lmeds else "threshold") + " must be finite and not negative", number=float("nan"), **later)
    later.update(number=float("nan"))
    if essential:
        refused("the focal length must be finite and positive", focal=-1.0, **later)
        later.update(focal=-1.0)
    if lmeds:
        refused("rank = 0, must be 1..n = 16", rank=0, **later)
        later.update(rank=0)
    refused(f"n = {width - 1}, must be {width}..2^20", n=width - 1, **later)
