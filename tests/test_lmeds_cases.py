"""CPU: the numpy restatement of the least-median-of-squares match filter (tests/lmeds_cases.py) against a full sort, its formulas,
and the truth of its scenes; the refusals and the all-True edge cases of the Python layer that make no device call.  The device
is held to the restatement in tests/test_gpu_lmeds.py."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
import essential_cases as es  # noqa: E402
import lmeds_cases as lc  # noqa: E402

K = es.K_TRUE


@pytest.fixture(scope="module")
def fundamental():
    """scene -> (p1, p2, outlier, Fs) with numpy's own 8-point solutions: computed once, shared, never changed"""
    out = {}
    for scene in lc.LMEDS_SCENES:
        p1, p2, outlier, samples = lc.fundamental_scene(*scene)
        out[scene] = (p1, p2, outlier, ec.solve8_all(p1, p2, samples))
    return out


@pytest.fixture(scope="module")
def essential():
    out = {}
    for scene in lc.LMEDS5_SCENES + (lc.LMEDS5_LOW_SHARE,):
        p1, p2, outlier, samples = lc.essential_scene(*scene[:4])
        out[scene] = (p1, p2, outlier, es.solve5_all(p1, p2, samples, K, judge=False)[0])
    return out


def test_values_agree_with_a_full_sort(fundamental):
    p1, p2, _, Fs = fundamental[lc.LMEDS_SCENES[1]]
    Fs = Fs[:200].copy()
    Fs[3] = np.nan
    Fs[7] = 0.0
    n = len(p1)
    for r in (1, 9, n // 2, n - 1, n):
        v = lc.values(Fs, p1, p2, r)
        for h, F in enumerate(Fs):
            e = ec.errors(F, p1, p2)
            e[np.isnan(e)] = np.inf
            assert v[h] == np.sort(e)[r - 1]
        assert np.isinf(v[3]) and np.isinf(v[7])


def test_rank_and_scale_formulas():
    for m in (8, 5):
        assert lc.rank_of(m + 1, m) == m + 1                                    # n = m + 1: the rank is n
        for q in (0.1, 0.5):
            assert lc.rank_of(2 * (m + 1), m, q) == m + 1                       # up to n = 2 (m + 1) the quantile changes nothing
            assert lc.rank_of(2 * (m + 1) - 1, m, q) == m + 1
        assert lc.rank_of(2 * (m + 1) + 1, m) == m + 2
        assert lc.rank_of(100000, m) == 50000 and lc.rank_of(100001, m) == 50001 and lc.rank_of(100000, m, 0.25) == 25000
        assert lc.rank_of(100, m, 1.0) == 100 and lc.rank_of(7 + m, m, 0.999) == 7 + m
        for n in (m + 1, 2 * (m + 1), 100000):
            want = 2.5 * 1.4826022 * (1.0 + 5.0 / (n - m))
            assert abs(math.sqrt(lc.scale2_of(n, m)) - want) <= 1e-7 * want
            assert lc.scale2_of(n, m) > 1.0
            # a lower quantile has a larger constant: 1 / Phi^-1(0.625) = 3.138
            assert abs(math.sqrt(lc.scale2_of(n, m, 0.25)) - 2.5 * 3.1382 * (1.0 + 5.0 / (n - m))) <= 1e-4 * want
        assert lc.scale2_of(100, m, 1.0) == 0.0
    from alproj_amd import _lib
    for n, m, q in ((9, 8, 0.5), (18, 8, 0.5), (500, 8, 0.5), (400, 5, 0.25), (100000, 5, 0.5), (77, 5, 1.0)):
        assert _lib.lmeds_rank(n, m, q) == lc.rank_of(n, m, q) and _lib.lmeds_scale2(n, m, q) == lc.scale2_of(n, m, q)


@pytest.mark.parametrize("scene", lc.LMEDS_SCENES)
def test_fundamental_scenes_against_the_truth(fundamental, scene):
    p1, p2, outlier, Fs = fundamental[scene]
    n = len(p1)
    for refits in (0, 1, 4):
        out = lc.lmeds(p1, p2, Fs, 8, refits=refits)
        lost, kept = lc.truth(out, outlier)
        ok, why = lc.decisions_decided(out, p1, p2)
        print(f"{scene} refits {refits}: bound {out['bound']:.3f} px, {lost} true inliers lost, {kept} outliers kept, refits kept {out['refits_kept']}")
        assert lost == 0 and kept <= lc.OUTLIER_CAP * n and ok, why
        assert out["mask"].sum() >= out["rank"] and out["bound"] >= 1.0
        assert out["values"][out["chosen"]] == out["values"].min() == out["value"] and out["chosen"] == np.flatnonzero(out["values"] == out["value"])[0]
        assert out["final_value"] <= out["value"] and out["refits_kept"] <= len(out["refit_values"]) <= refits


@pytest.mark.parametrize("scene", lc.LMEDS5_SCENES)
def test_essential_scenes_against_the_truth(essential, scene):
    p1, p2, outlier, Fs = essential[scene]
    for refits in (0, 1, 4):
        out = lc.lmeds(p1, p2, Fs, 5, refits=refits, K=K)
        lost, kept = lc.truth(out, outlier)
        ok, why = lc.decisions_decided(out, p1, p2)
        print(f"{scene} refits {refits}: bound {out['bound']:.3f} px, {lost} true inliers lost, {kept} outliers kept, refits kept {out['refits_kept']}")
        assert lost == 0 and kept <= lc.OUTLIER_CAP * len(p1) and ok, why


def test_a_quantile_below_the_inlier_share(essential):
    """280 of 400 matches are outliers.  At the median every hypothesis' value belongs to an outlier and the bound is useless; at
    quantile 0.25, below the inlier share 0.3, the filter keeps 120 / 120 true inliers and 5 outliers at a bound of 28.4 px."""
    scene = lc.LMEDS5_LOW_SHARE
    p1, p2, outlier, Fs = essential[scene]
    half = lc.lmeds(p1, p2, Fs, 5, K=K)
    low = lc.lmeds(p1, p2, Fs, 5, quantile=scene[4], K=K)
    for name, out in (("quantile 0.5", half), (f"quantile {scene[4]}", low)):
        lost, kept = lc.truth(out, outlier)
        print(f"{name}: rank {out['rank']}, bound {out['bound']:.3f} px, {lost} of 120 true inliers lost, {kept} of 280 outliers kept")
    assert low["rank"] == 100 and half["rank"] == 200
    assert lc.truth(low, outlier) == (0, 5) and 28.0 < low["bound"] < 29.0
    assert lc.decisions_decided(low, p1, p2)[0]
    assert half["bound"] > 3 * low["bound"] and lc.truth(half, outlier)[1] > 50


def test_self_distance_of_the_refit_value(fundamental, essential):
    """lmeds_cases.SELF_DISTANCE: two numpy routes to the value of the first refit's candidate, over every scene"""
    worst = 0.0
    for scenes, m, Kq in ((fundamental, 8, None), (essential, 5, K)):
        for scene, (p1, p2, _, Fs) in scenes.items():
            q = scene[4] if len(scene) > 4 else 0.5
            out = lc.lmeds(p1, p2, Fs, m, quantile=q, refits=1, K=Kq)
            a, b = lc.refit_value_routes(p1, p2, out["sets"][0], out["rank"], Kq)
            assert a == out["refit_values"][0]
            print(f"{scene}: eigh {a!r} svd {b!r} relative {abs(a - b) / max(a, b):.3e}")
            worst = max(worst, abs(a - b) / max(a, b))
    assert worst <= lc.SELF_DISTANCE and lc.VALUE_TOL == 100 * lc.SELF_DISTANCE


def test_large_scene_is_decided():
    p1, p2, outlier, samples = lc.large_scene()
    assert len(p1) == 70001 and samples.max() < 70001 and samples.max() >= 69500
    Fs = ec.solve8_all(p1, p2, samples)
    for refits in (0, 4):
        out = lc.lmeds(p1, p2, Fs, 8, refits=refits)
        ok, why = lc.decisions_decided(out, p1, p2)
        assert ok, why
        assert lc.truth(out, outlier)[0] == 0 and lc.truth(out, outlier)[1] <= lc.OUTLIER_CAP * len(p1)


def test_placed_keys_are_exact():
    y = np.array([0.0, 2.0 ** -30, 1.0 + 2.0 ** -26, 3.0, 2.0 ** 30 * (1.0 + 5 * 2.0 ** -26), 1e200, np.nan])
    p1, p2 = lc.placed(y)
    with np.errstate(over="ignore"):
        want = y * y
    want[-1] = np.inf
    assert lc.errors_inf(lc.F_ROWS, p1, p2).tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------------------ Python layer, no device call
def test_python_layer_refusals_and_edges():
    from alproj_amd import gcp
    p = np.random.default_rng(0).uniform(0.0, 1000.0, (40, 2))
    for name in ("USAC_MAGSAC", "usac_default"):
        with pytest.raises(NotImplementedError, match="'RANSAC', 'LMEDS'"):
            gcp.filter_geometric(p, p, ransac_method=name)
    for name in ("MAGSAC", "", "least median"):
        with pytest.raises(ValueError, match="Unknown ransac_method"):
            gcp.filter_geometric(p, p, ransac_method=name)
    for q in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="quantile"):
            gcp.filter_geometric(p, p, ransac_method="LMEDS", quantile=q)
    for t in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_threshold"):
            gcp.filter_geometric(p, p, ransac_method="LMEDS", min_threshold=t)
    with pytest.raises(ValueError):
        gcp.filter_matches(p, p, None, ransac_method="nonsense")
    with pytest.raises(TypeError):                                               # keyword only
        gcp.filter_geometric(p, p, "fundamental", 10.0, 16384, 0, 4, None, False, None, None, None, "LMEDS")
    # n <= m: all True before any device call (there is no device here), with the model None
    for n, method, kw in ((8, "fundamental", {}), (3, "fundamental", {}), (5, "essential", {"focal_length": 1200.0}), (2, "essential", {})):
        mask, F, info = gcp.filter_geometric(p[:n], p[:n], method=method, ransac_method="LMEDS", return_model=True, **kw)
        assert mask.dtype == bool and mask.all() and len(mask) == n and F is None and info == {}
    assert gcp.filter_geometric(p[:0], p[:0], ransac_method="LMEDS").shape == (0,)
    assert gcp.filter_geometric(p, p, method="none", ransac_method="LMEDS").all()
    df = gcp.filter_matches(p[:8], p[:8], None, ransac_method="LMEDS")
    assert len(df) == 8 and list(df.columns) == ["u_org", "v_org", "u_sim", "v_sim"]
    # the essential filter still wants its focal length
    with pytest.raises(NotImplementedError, match="focal"):
        gcp.filter_geometric(p, p, method="essential", ransac_method="LMEDS")
    assert "ransac_method" in gcp.filter_matches.__doc__ and "LMEDS" in gcp.__doc__
