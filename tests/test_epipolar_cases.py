"""CPU: the numpy restatement of the geometric match filter (tests/epipolar_cases.py) against an independent triple loop and
against the truth on synthetic scenes, and every refusal and edge case of alproj_amd.gcp.filter_geometric / filter_spatial /
filter_matches that makes no device call.  tests/test_gpu_epipolar.py holds the device to the restatement."""
import math
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_filter_spatial.npz")


def error_by_loops(F, a, b):
    """e of one match: Python floats (IEEE double, no fused multiply-add), the products summed left to right in loops"""
    F = [[float(F[i][j]) for j in range(3)] for i in range(3)]
    x1, y1, x2, y2 = float(a[0]), float(a[1]), float(b[0]), float(b[1])
    l2 = []
    for i in range(3):
        acc = F[i][0] * x1
        acc = acc + F[i][1] * y1
        l2.append(acc + F[i][2])
    l1 = []
    for j in range(2):
        acc = F[0][j] * x2
        acc = acc + F[1][j] * y2
        l1.append(acc + F[2][j])
    s = x2 * l2[0]
    s = s + y2 * l2[1]
    s = s + l2[2]
    quotients = []
    for d in (l2[0] * l2[0] + l2[1] * l2[1], l1[0] * l1[0] + l1[1] * l1[1]):
        quotients.append(s * s / d if d != 0.0 else (math.nan if s * s == 0.0 else math.inf))
    return math.nan if any(q != q for q in quotients) else max(quotients)


def test_errors_equal_the_triple_loop():
    p1, p2, F, _ = ec.scene(120, 40, 0.5, 1)
    rng = np.random.default_rng(3)
    for G in (F, rng.standard_normal((3, 3)), ec.solve8(p1, p2, np.arange(8))):
        want = np.array([error_by_loops(G, a, b) for a, b in zip(p1, p2)])
        np.testing.assert_array_equal(ec.errors(G, p1, p2), want)


def test_error_is_the_squared_distance_to_the_epipolar_lines():
    """F = the x-translation pair: l2 = (0, -1, y1) -> e = (y2 - y1)^2 in both images"""
    F = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    p1 = np.array([[10.0, 20.0], [5.0, 7.0], [0.0, 0.0]])
    p2 = np.array([[90.0, 23.0], [1.0, 7.0], [4.0, -2.0]])
    np.testing.assert_array_equal(ec.errors(F, p1, p2), [9.0, 0.0, 4.0])
    np.testing.assert_array_equal(ec.inliers(F, p1, p2, 2.0), [False, True, True])           # exactly on the threshold: an inlier
    assert not ec.inliers(np.full((3, 3), np.nan), p1, p2, 1e300).any()
    assert ec.counts(np.stack([F, np.full((3, 3), np.nan)]), p1, p2, 3.0).tolist() == [3, 0]


def test_scene_is_what_it_says():
    p1, p2, F, out = ec.scene(300, 100, 0.0, 4)
    assert p1.shape == p2.shape == (300, 2) and out.sum() == 100 and not out[:200].any()
    assert abs(np.sqrt((F * F).sum()) - 1.0) < 1e-15 and abs(np.linalg.det(F)) < 1e-18
    assert ec.errors(F, p1, p2)[~out].max() < 1e-16 * 1504 ** 2          # noise-free matches lie on their lines
    assert (ec.errors(F, p1, p2)[out] > 9.0).mean() > 0.9
    q1, q2, _, _ = ec.scene(300, 0, 0.5, 4)
    r = np.sqrt(ec.errors(F, q1, q2))
    assert 0.3 < np.median(r) < 1.0 and r.max() < 4.0                     # sigma = 0.5 on both images
    for p in (p1, p2[~out]):
        assert p.min() > -1 and p[:, 0].max() < 1505 and p[:, 1].max() < 1001


def test_solve8_recovers_the_truth_without_noise():
    p1, p2, F, _ = ec.scene(200, 0, 0.0, 1)
    G = ec.solve8_all(p1, p2, ec.draw_samples(200, 300, 5))
    assert ec.sign_distance(G, F).max() <= 1e-11
    assert np.abs(np.linalg.det(G)).max() <= 1e-12
    np.testing.assert_allclose(np.sqrt((G * G).sum(axis=(1, 2))), 1.0, rtol=0, atol=1e-15)


def test_solve8_refuses_a_repeated_point():
    p1, p2, _, _ = ec.scene(50, 0, 0.5, 2)
    assert np.isnan(ec.solve8(p1, p2, np.array([0, 1, 2, 3, 4, 5, 6, 6]))).all()
    assert np.isfinite(ec.solve8(p1, p2, np.arange(8))).all()


def test_choose_takes_the_lowest_index_on_a_tie():
    assert ec.choose(np.array([3, 9, 9, 2])) == 1 and ec.choose(np.array([0, 0])) == 0


@pytest.mark.parametrize("n,n_out,threshold,seed", ec.RANSAC_SCENES)
def test_ransac_restatement_against_the_truth(n, n_out, threshold, seed):
    """The scenes of the device test: every true inlier kept, no outlier kept except at most 2 within threshold of the true
    epipolar lines, and no match within 1 % of threshold^2 (so that two numerical routes give one mask)."""
    p1, p2, F, out = ec.scene(n, n_out, 0.5, seed)
    r = ec.ransac(p1, p2, ec.draw_samples(n, 2048, 1000 + seed), threshold)
    e = ec.errors(r["F"], p1, p2)
    assert not (np.abs(e - threshold ** 2) <= 0.01 * threshold ** 2).any()
    assert not r["keep_all"] and r["mask"][~out].all()
    kept = out & r["mask"]
    assert kept.sum() <= 2 and (ec.errors(F, p1, p2)[kept] <= threshold ** 2).all()
    assert r["final_count"] == r["mask"].sum() >= r["chosen_count"] >= 8
    assert len(r["refit_counts"]) == min(r["refits_kept"] + 1, 4)


def test_ransac_keeps_everything_without_eight_inliers():
    rng = np.random.default_rng(12)
    p1, p2 = rng.uniform(0, 1000, (12, 2)), rng.uniform(0, 1000, (12, 2))
    r = ec.ransac(p1, p2, ec.draw_samples(12, 64, 1), 0.01)
    assert r["keep_all"] and r["mask"].all() and r["chosen_count"] < 8 and r["refit_counts"] == []


# ------------------------------------------------------------------------------------------------------------ the Python layer
def test_filter_geometric_edge_cases_of_the_reference():
    from alproj_amd import gcp
    empty = gcp.filter_geometric(np.zeros((0, 2)), np.zeros((0, 2)))
    assert empty.dtype == bool and empty.shape == (0,)
    assert gcp.filter_geometric([], [], method="no such method").shape == (0,)        # the reference looks at the length first
    p = np.arange(14.0).reshape(7, 2)
    for method in ("none", "NONE", "fundamental", "Fundamental"):
        m = gcp.filter_geometric(p, p, method=method)
        assert m.dtype == bool and m.all() and m.shape == (7,)
    mask, F, info = gcp.filter_geometric(p, p, return_model=True)
    assert mask.all() and F is None and info == {}
    with pytest.raises(ValueError, match=r"Unknown outlier_filter 'homography'\. Available: 'essential', 'fundamental', 'none'"):
        gcp.filter_geometric(p, p, method="homography")
    with pytest.raises(NotImplementedError, match="stays with the reference"):
        gcp.filter_geometric(p, p, method="essential")


def test_filter_geometric_refuses_before_the_device():
    from alproj_amd import gcp
    p = np.arange(40.0).reshape(20, 2)
    bad = p.copy()
    bad[3, 1] = np.nan
    for args, kw in (((p, p[:19]), {}), ((p.reshape(10, 4), p.reshape(10, 4)), {}), ((bad, p), {}), ((p, p), {"threshold": np.inf}),
                     ((p, p), {"threshold": -1.0}), ((p, p), {"hypotheses": 0}), ((p, p), {"refits": 9}), ((p, p), {"refits": -1})):
        with pytest.raises(ValueError):
            gcp.filter_geometric(*args, **kw)


def test_filter_spatial_validation_and_empty_case():
    from alproj_amd import gcp
    for grid in (0, -5):
        with pytest.raises(ValueError, match="grid_size must be positive"):
            gcp.filter_spatial(np.zeros((3, 2)), grid, (100, 100))
    empty = gcp.filter_spatial(np.zeros((0, 2)), 10, (100, 100), selection="no such selection")
    assert empty.dtype == bool and empty.shape == (0,)
    with pytest.raises(ValueError, match=r"Unknown selection 'nearest'\. Available: 'first', 'random', 'center'"):
        gcp.filter_spatial(np.zeros((3, 2)), 10, (100, 100), selection="nearest")


def test_filter_spatial_random_equals_the_reference():
    """selection="random" makes no device call: the reference's own draws, case by case of the golden file"""
    from alproj_amd import gcp
    g = np.load(GOLDEN)
    seen = 0
    for k in range(int(g["n_cases"])):
        if str(g[f"sel{k}"]) != "random":
            continue
        grid, w, h, seed = g[f"args{k}"]
        got = gcp.filter_spatial(g[f"pts{k}"], int(grid), (int(w), int(h)), "random", int(seed))
        np.testing.assert_array_equal(got, g[f"mask{k}"])
        seen += 1
    assert seen >= 10


def test_filter_matches_without_a_device_call():
    from alproj_amd import gcp
    none = gcp.filter_matches(np.zeros((0, 2), dtype="int32"), np.zeros((0, 2), dtype="int32"), (100, 100), spatial_thin_grid=10)
    assert list(none.columns) == ["u_org", "v_org", "u_sim", "v_sim"] and len(none) == 0
    p1 = np.array([[1, 2], [3, 4], [50, 60]], dtype="int32")
    p2 = p1 + 100
    frame = gcp.filter_matches(p1, p2, None, outlier_filter="none")
    pd.testing.assert_frame_equal(frame, pd.DataFrame(np.hstack((p1, p2)), columns=["u_org", "v_org", "u_sim", "v_sim"]))
    assert len(gcp.filter_matches(p1, p2, None)) == 3                     # fewer than 8 points: all kept
    with pytest.raises(ValueError, match="image_size could not be determined"):
        gcp.filter_matches(p1, p2, None, outlier_filter="none", spatial_thin_grid=10)
    thinned = gcp.filter_matches(p1, p2, (100, 100), outlier_filter="none", spatial_thin_grid=10, spatial_thin_selection="random",
                                 spatial_thin_random_state=1)
    assert thinned.to_numpy().tolist() == [[1, 2, 101, 102], [50, 60, 150, 160]] or thinned.to_numpy().tolist() == [[3, 4, 103, 104], [50, 60, 150, 160]]
    with pytest.raises(ValueError, match="Unknown outlier_filter"):
        gcp.filter_matches(p1, p2, None, outlier_filter="ransac")
    for name in ("filter_geometric", "filter_spatial", "filter_matches"):
        assert name in gcp.__all__


def test_plan_mode_prints_the_filter_plan():
    from alproj_amd import _build
    exe = _build.build_host("plain", "clang")
    out = subprocess.run([exe, "--plan", "epi,5000,16384,0,256", "epi,513,1,2,64", "epi,8,600000,0,256"], capture_output=True, text=True, check=True)
    rows = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    # hyp_tile match_tile splits hyp_tiles match_tiles workgroups solve_blocks reduce_blocks bytes
    assert rows[0][:8] == [256, 512, 10, 64, 10, 640, 256, 20]            # 4 * 256 CUs / 64 tiles = 16 splits, capped by 10 match tiles
    assert rows[1][:8] == [256, 512, 2, 1, 2, 2, 1, 3]
    assert rows[2][:8] == [256, 512, 1, 2344, 1, 2344, 9375, 1]
    assert subprocess.run([exe, "--plan", "epi,7,16,0,64"], capture_output=True).returncode == 2
    assert subprocess.run([exe, "--plan", "epi,512,16,2,64"], capture_output=True).returncode == 2       # more splits than match tiles
