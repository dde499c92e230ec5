"""GPU: the least-median-of-squares match filter (alp_epipolar_select / alp_epipolar_lmeds / alp_essential_lmeds) and the Python
layer over it (alproj_amd.gcp.filter_geometric(ransac_method="LMEDS") / filter_matches) against the numpy restatement of
tests/lmeds_cases.py and the truth of its synthetic scenes.

what can go wrong                                              where it is held
a tile seam of matches or hypotheses, a split, a rank          test_select_equals_the_restatement, test_select_beyond_one_wave_of_workgroups
a digit of the radix select, a tie across the rank, inf, NaN   test_select_of_placed_keys
choice, bound, refit loop and its stop, the final mask         test_lmeds_equals_the_restatement, test_essential_lmeds_equals_the_restatement
strided reductions, many splits                                test_lmeds_large_n
the device's own draws                                         test_lmeds_own_draws
the smallest n, no finite hypothesis, the floor of the bound   test_lmeds_edges
the Python layer                                               test_python_layer
refusals of the C entry points                                 test_entry_point_refusals

What makes no device call needs no GPU: tests/test_lmeds_cases.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
import essential_cases as es  # noqa: E402
import lmeds_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

K = es.K_TRUE
INF_BITS = 0x7FF0000000000000


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def seam():
    """scene(1025, 300, 0.5, 3), 257 hypotheses from numpy's solve with a NaN one and a zero one among them: computed once"""
    p1, p2, _, _ = ec.scene(1025, 300, 0.5, 3)
    Fs = ec.solve8_all(p1, p2, ec.draw_samples(1025, 257, 11))
    Fs[5] = np.nan
    Fs[200] = 0.0
    return p1, p2, Fs


# ------------------------------------------------------------------------------------------------------------ select
@pytest.mark.parametrize("n", [8, 9, 511, 512, 513, 1025])
def test_select_equals_the_restatement(L, seam, n):
    """Bit for bit at the seams of the 512-match tile and of the 256-hypothesis tile, every rank that the issue names, and one
    answer for every number of splits."""
    p1, p2, Fs = seam[0][:n], seam[1][:n], seam[2]
    tiles = (n + 511) // 512
    ranks = sorted({1, min(n, 9), (n + 1) // 2, n - 1, n})
    for r in ranks:
        want = lc.values(Fs, p1, p2, r)
        assert np.isinf(want[5]) and np.isinf(want[200])
        for H in (1, 255, 256, 257):
            got, info = L.epipolar_select(p1, p2, Fs[:H], r)
            assert got.shape == (H,) and info["passes"] == 16 and info["match_tiles"] == tiles
            np.testing.assert_array_equal(bits(got), bits(want[:H]), err_msg=f"n {n} rank {r} H {H}")
        for splits in sorted({1, 2, tiles} - {s for s in (2,) if s > tiles}):
            got, info = L.epipolar_select(p1, p2, Fs, r, splits=splits)
            assert info["splits"] == splits
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"n {n} rank {r} splits {splits}")


def test_select_beyond_one_wave_of_workgroups(L, seam):
    """more workgroups than the device holds at once: 468 hypothesis tiles x 3 splits = 1404, where 256 CUs hold 5 each"""
    p1, p2, Fs = seam
    rng = np.random.default_rng(5)
    big = Fs[rng.integers(0, 257, 256 * 467 + 3)]
    want = lc.values(Fs, p1, p2, 513)
    got, info = L.epipolar_select(p1, p2, big, 513, splits=3)
    assert info["workgroups"] == 468 * 3
    src = np.random.default_rng(5).integers(0, 257, 256 * 467 + 3)
    np.testing.assert_array_equal(bits(got), bits(want[src]))


def _expect(keys, r):
    """the r-th smallest of the placed errors, NaN as inf: built from the keys, not taken from the device"""
    e = np.where(np.isnan(keys), np.inf, keys)
    return np.sort(e)[r - 1]


def test_select_of_placed_keys(L):
    """F_ROWS makes the error of a match exactly y1^2 (y2 = 0), so the keys stand where the test puts them."""
    rng = np.random.default_rng(2)
    cases = {}
    # spread over 2^-60 .. 2^60 (y = 2^-30 .. 2^30, exact squares): every pass has work
    cases["spread"] = 2.0 ** rng.integers(-30, 31, 700) * (1.0 + rng.integers(0, 2 ** 20, 700) * 2.0 ** -26)
    # runs that agree in every digit but the last: y = 2^k (1 + j 2^-26), whose square 2^2k (1 + j 2^-25 + j^2 2^-52) is exact
    cases["last digit"] = np.concatenate([2.0 ** k * (1.0 + np.arange(1, 9) * 2.0 ** -26) for k in (-3, 0, 7)] * 25)
    # many exact zeros and ties across the rank
    cases["zeros and ties"] = np.concatenate([np.zeros(300), np.full(200, 3.0), np.full(150, 5.0), rng.permutation(np.arange(1, 51) * 0.5)])
    # +inf (the square overflows) and NaN errors among finite ones
    y = rng.permutation(np.concatenate([np.full(120, 1e200), np.full(130, np.nan), np.arange(1, 400) * 0.25]))
    cases["inf and nan"] = y
    for name, y in cases.items():
        y = rng.permutation(y)
        p1, p2 = lc.placed(y)
        with np.errstate(over="ignore"):
            keys = y * y
        np.testing.assert_array_equal(bits(lc.errors_inf(lc.F_ROWS, p1, p2)), bits(np.where(np.isnan(keys), np.inf, keys)), err_msg=name)
        n = len(y)
        Fs = np.stack([lc.F_ROWS, np.full((3, 3), np.nan), np.zeros((3, 3)), lc.F_ROWS])
        for r in sorted({1, 2, 9, n // 3, (n + 1) // 2, 300, 301, 500, 501, 650, 651, n - 1, n} & set(range(1, n + 1))):
            want = _expect(keys, r)
            for splits in (0, 1, 2):
                got, _ = L.epipolar_select(p1, p2, Fs, r, splits=splits)
                assert bits(got)[0] == bits(want) and bits(got)[3] == bits(want), f"{name}: rank {r}: {got[0]!r}, not {want!r}"
                assert bits(got)[1] == INF_BITS and bits(got)[2] == INF_BITS, f"{name}: a NaN F and a zero F have the value inf"


# ------------------------------------------------------------------------------------------------------------ whole filter
def _compare(dev, ref, p1, p2, outlier, n):
    ok, why = lc.decisions_decided(ref, p1, p2)
    assert ok, why                                       # the scene was chosen so: nothing is excused silently
    info = dev["info"]
    assert info["chosen"] == ref["chosen"]
    assert bits(dev["value"]) == bits(ref["value"])
    assert info["keep_all"] == ref["keep_all"] and info["refits_kept"] == ref["refits_kept"]
    assert info["refits_run"] == len(ref["refit_values"]) == len(dev["refit_values"])
    for a, b in zip(dev["refit_values"], ref["refit_values"]):
        print(f"refit value: device {a!r} numpy {b!r} relative {abs(a - b) / b:.3e} (tolerance {lc.VALUE_TOL:.1e})")
        assert abs(a - b) <= lc.VALUE_TOL * b
    assert abs(dev["final_value"] - ref["final_value"]) <= lc.VALUE_TOL * ref["final_value"]
    assert abs(dev["bound"] - ref["bound"]) <= lc.VALUE_TOL * ref["bound"]
    np.testing.assert_array_equal(dev["mask"], ref["mask"])
    assert info["final_count"] == int(ref["mask"].sum())
    lost, kept = lc.truth(ref, outlier)
    assert lost == 0 and kept <= lc.OUTLIER_CAP * n


@pytest.mark.parametrize("scene", lc.LMEDS_SCENES)
def test_lmeds_equals_the_restatement(L, scene):
    n, n_out, seed = scene
    p1, p2, outlier, samples = lc.fundamental_scene(n, n_out, seed)
    Fs = L.epipolar_solve8(p1, p2, samples)               # the device's own hypotheses: a value cannot be compared across solvers
    r, s2 = lc.rank_of(n, 8), lc.scale2_of(n, 8)
    for refits in (0, 1, 4):
        ref = lc.lmeds(p1, p2, Fs, 8, refits=refits)
        dev = L.epipolar_lmeds(p1, p2, r, s2, 1.0, refits=refits, samples=samples)
        _compare(dev, ref, p1, p2, outlier, n)
        if refits == 0:
            assert bits(dev["bound"] ** 2) == bits(ref["bound"] ** 2) and bits(dev["F"]).tolist() == bits(Fs[ref["chosen"]]).tolist()


@pytest.mark.parametrize("scene", lc.LMEDS5_SCENES + (lc.LMEDS5_LOW_SHARE,))
def test_essential_lmeds_equals_the_restatement(L, scene):
    n, n_out, seed, planar = scene[:4]
    quantile = scene[4] if len(scene) > 4 else 0.5
    p1, p2, outlier, samples = lc.essential_scene(n, n_out, seed, planar)
    Fs, _ = L.epipolar_solve5(p1, p2, samples, K[0], K[1:])
    r, s2 = lc.rank_of(n, 5, quantile), lc.scale2_of(n, 5, quantile)
    for refits in (0, 1, 4):
        ref = lc.lmeds(p1, p2, Fs, 5, quantile=quantile, refits=refits, K=K)
        dev = L.essential_lmeds(p1, p2, K[0], K[1:], r, s2, 1.0, refits=refits, samples=samples)
        _compare(dev, ref, p1, p2, outlier, n)


def test_lmeds_large_n(L):
    """70 001 matches, 256 hypotheses: the refit's reductions stride and the select runs on many splits"""
    p1, p2, outlier, samples = lc.large_scene()
    n = len(p1)
    assert n == 70001
    Fs = L.epipolar_solve8(p1, p2, samples)
    r, s2 = lc.rank_of(n, 8), lc.scale2_of(n, 8)
    want = lc.values(Fs, p1, p2, r)
    got, info = L.epipolar_select(p1, p2, Fs, r)
    assert info["splits"] > 1
    np.testing.assert_array_equal(bits(got), bits(want))
    for refits in (0, 4):
        ref = lc.lmeds(p1, p2, Fs, 8, refits=refits)
        dev = L.epipolar_lmeds(p1, p2, r, s2, 1.0, refits=refits, samples=samples)
        assert dev["info"]["splits"] > 1 and dev["info"]["reduce_blocks"] * 256 < n
        _compare(dev, ref, p1, p2, outlier, n)


def test_lmeds_own_draws(L):
    n, n_out, seed = lc.LMEDS_SCENES[0]
    p1, p2, outlier, _ = lc.fundamental_scene(n, n_out, seed)
    r, s2 = lc.rank_of(n, 8), lc.scale2_of(n, 8)
    a = L.epipolar_lmeds(p1, p2, r, s2, 1.0, hypotheses=2048, seed=3)
    b = L.epipolar_lmeds(p1, p2, r, s2, 1.0, hypotheses=2048, seed=3)
    c = L.epipolar_lmeds(p1, p2, r, s2, 1.0, hypotheses=2048, seed=4)
    np.testing.assert_array_equal(a["mask"], b["mask"])
    assert a["info"] == b["info"] and bits(a["F"]).tolist() == bits(b["F"]).tolist() and a["value"] == b["value"]
    assert a["info"]["chosen"] != c["info"]["chosen"]
    # the draws are alp_epipolar_samples' own
    d = L.epipolar_lmeds(p1, p2, r, s2, 1.0, samples=L.epipolar_samples(n, 2048, seed=3))
    assert d["info"]["chosen"] == a["info"]["chosen"] and d["value"] == a["value"]
    np.testing.assert_array_equal(a["mask"], d["mask"])
    e = L.essential_lmeds(p1, p2, K[0], K[1:], lc.rank_of(n, 5), lc.scale2_of(n, 5), 1.0, hypotheses=512, seed=3)
    f = L.essential_lmeds(p1, p2, K[0], K[1:], lc.rank_of(n, 5), lc.scale2_of(n, 5), 1.0, samples=L.epipolar_samples5(n, 512, seed=3))
    assert e["info"]["chosen"] == f["info"]["chosen"] and e["value"] == f["value"]
    np.testing.assert_array_equal(e["mask"], f["mask"])


def test_lmeds_edges(L):
    # n = m + 1 and n = 2 (m + 1): the rank is m + 1
    for n in (9, 18):
        p1, p2, _, _ = ec.scene(n, 0, 0.5, 2)
        samples = ec.draw_samples(n, 64, 3)
        Fs = L.epipolar_solve8(p1, p2, samples)
        assert lc.rank_of(n, 8) == 9
        ref = lc.lmeds(p1, p2, Fs, 8, refits=0)
        dev = L.epipolar_lmeds(p1, p2, 9, lc.scale2_of(n, 8), 1.0, refits=0, samples=samples)
        assert dev["info"]["chosen"] == ref["chosen"] and bits(dev["value"]) == bits(ref["value"])
        assert dev["bound"] == ref["bound"]             # without a refit nothing but bit-equal numbers enters
        np.testing.assert_array_equal(dev["mask"], ref["mask"])
        assert dev["mask"].sum() >= 9
    for n in (6, 12):
        p1, p2, _, _ = ec.scene(n, 0, 0.5, 2)
        samples = es.draw_samples5(n, 64, 3)
        Fs, _ = L.epipolar_solve5(p1, p2, samples, K[0], K[1:])
        ref = lc.lmeds(p1, p2, Fs, 5, refits=0, K=K)
        dev = L.essential_lmeds(p1, p2, K[0], K[1:], 6, lc.scale2_of(n, 5), 1.0, refits=0, samples=samples)
        assert dev["info"]["chosen"] == ref["chosen"] and bits(dev["value"]) == bits(ref["value"]) and dev["bound"] == ref["bound"]
        np.testing.assert_array_equal(dev["mask"], ref["mask"])
        assert dev["mask"].sum() >= 6
    # every hypothesis NaN: samples of one repeated match have rank below 8
    p1, p2, _, _ = ec.scene(40, 0, 0.5, 2)
    dev = L.epipolar_lmeds(p1, p2, 20, lc.scale2_of(40, 8), 1.0, samples=np.zeros((70, 8), dtype=np.int32))
    assert dev["info"]["keep_all"] and dev["mask"].all() and np.isinf(dev["value"]) and dev["info"]["refits_run"] == 0
    # a noise-free scene: the values are rounding noise, the bound is the floor exactly, every true inlier is kept
    p1, p2, _, outlier = ec.scene(200, 60, 0.0, 3)
    samples = ec.draw_samples(200, 1024, 4)
    r, s2 = lc.rank_of(200, 8), lc.scale2_of(200, 8)
    dev = L.epipolar_lmeds(p1, p2, r, s2, 1.0, samples=samples)
    assert dev["bound"] == 1.0 and dev["mask"][~outlier].all() and dev["value"] < 1e-12
    dev = L.epipolar_lmeds(p1, p2, r, s2, 0.25 * 0.25, samples=samples)
    assert dev["bound"] == 0.25 and dev["mask"][~outlier].all()
    # min_threshold = 0: the bound is scale^2 * value alone, and by scale > 1 at least `rank` matches are inliers
    dev = L.epipolar_lmeds(p1, p2, r, s2, 0.0, refits=0, samples=samples)
    assert dev["bound"] == np.sqrt(s2 * dev["value"])
    assert dev["mask"].sum() >= r
    Fs = L.epipolar_solve8(p1, p2, samples)
    ref = lc.lmeds(p1, p2, Fs, 8, min_threshold=0.0, refits=0)
    assert dev["info"]["chosen"] == ref["chosen"] and bits(dev["value"]) == bits(ref["value"])
    np.testing.assert_array_equal(dev["mask"], ref["mask"])


# ------------------------------------------------------------------------------------------------------------ Python layer
def test_python_layer(L):
    from alproj_amd import gcp
    n, n_out, seed = lc.LMEDS_SCENES[0]
    p1, p2, outlier, samples = lc.fundamental_scene(n, n_out, seed)
    r, s2 = lc.rank_of(n, 8), lc.scale2_of(n, 8)
    assert L.lmeds_rank(n, 8) == r and L.lmeds_scale2(n, 8) == s2
    low = L.epipolar_lmeds(p1, p2, r, s2, 1.0, samples=samples)
    mask, F, info = gcp.filter_geometric(p1, p2, samples=samples, ransac_method="lmeds", return_model=True)
    np.testing.assert_array_equal(mask, low["mask"])
    assert bits(F).tolist() == bits(low["F"]).tolist()
    assert info["method"] == "LMEDS" and info["rank"] == r and info["value"] == low["value"] and info["final_value"] == low["final_value"]
    assert info["bound"] == low["bound"] and info["refit_values"] == low["refit_values"] and info["chosen"] == low["info"]["chosen"]
    np.testing.assert_array_equal(gcp.filter_geometric(p1, p2, samples=samples, ransac_method="LMEDS", threshold=0.01), low["mask"])
    # other parameters reach the device
    q = gcp.filter_geometric(p1, p2, samples=samples, ransac_method="LMEDS", quantile=0.4, min_threshold=2.0, return_model=True)[2]
    assert q["rank"] == 200 and q["bound"] >= 2.0
    # the essential filter through filter_matches and params
    params = {"fov": np.degrees(2 * np.arctan(ec.WIDTH / 2 / ec.FOCAL)), "w": ec.WIDTH, "h": ec.HEIGHT}
    s5 = es.draw_samples5(n, 512, 9)
    low5 = L.essential_lmeds(p1, p2, (ec.WIDTH / 2) / np.tan(params["fov"] * np.pi / 180 / 2), (ec.WIDTH / 2, ec.HEIGHT / 2),
                             lc.rank_of(n, 5), lc.scale2_of(n, 5), 1.0, samples=s5)
    df = gcp.filter_matches(p1, p2, (ec.WIDTH, ec.HEIGHT), outlier_filter="essential", params=params, samples=s5, ransac_method="LMEDS")
    assert list(df.columns) == ["u_org", "v_org", "u_sim", "v_sim"]
    np.testing.assert_array_equal(df.to_numpy(), np.hstack([p1[low5["mask"]], p2[low5["mask"]]]))
    df8 = gcp.filter_matches(p1, p2, (ec.WIDTH, ec.HEIGHT), samples=samples, ransac_method="LMEDS")
    np.testing.assert_array_equal(df8.to_numpy(), np.hstack([p1[low["mask"]], p2[low["mask"]]]))
    # "RANSAC" is the call without the argument, bit for bit
    a = gcp.filter_geometric(p1, p2, threshold=3.0, samples=samples, return_model=True)
    b = gcp.filter_geometric(p1, p2, threshold=3.0, samples=samples, return_model=True, ransac_method="ransac")
    c = L.epipolar_ransac(p1, p2, 3.0, samples=samples)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[0], c["mask"])
    assert bits(a[1]).tolist() == bits(b[1]).tolist() == bits(c["F"]).tolist() and a[2] == b[2] == c["info"]


# ------------------------------------------------------------------------------------------------------------ refusals
def test_entry_point_refusals(L):
    lib = L.lib()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    p = np.ascontiguousarray(np.random.default_rng(0).uniform(0, 1000, (600, 2)))
    P = p.ctypes.data_as(dp)
    Fm = np.zeros((4, 9))
    Fp = Fm.ctypes.data_as(dp)
    val = np.zeros(4)
    V = val.ctypes.data_as(dp)
    Kv = np.array(K)
    Kp = Kv.ctypes.data_as(dp)
    bad = np.full((2, 8), 600, dtype=np.int32)
    EINVAL = -1

    def select(n=600, H=4, rank=300, splits=0, p1=P, F=Fp, out=V):
        return lib.alp_epipolar_select(p1, P, n, F, H, rank, splits, out, None)

    assert select() == 0
    for kw in (dict(p1=None), dict(F=None), dict(out=None), dict(n=7), dict(n=(1 << 20) + 1), dict(H=0), dict(H=(1 << 20) + 1), dict(rank=0),
               dict(rank=601), dict(splits=-1), dict(splits=3)):
        assert select(**kw) == EINVAL, kw
    # 16 passes * H * n above 2^35, which H * n alone is not
    assert lib.alp_epipolar_select(P, P, 1 << 16, Fp, (1 << 15) + 1, 1, 0, V, None) == EINVAL
    assert "2^35" in lib.alp_last_error().decode()

    def lmeds(n=600, H=4, rank=300, scale2=14.0, floor2=1.0, refits=4, splits=0, p1=P, samples=None, essential=False, Kq=Kp):
        if essential:
            return lib.alp_essential_lmeds(p1, P, n, samples, H, 0, Kq, rank, scale2, floor2, refits, splits, None, None, None, None)
        return lib.alp_epipolar_lmeds(p1, P, n, samples, H, 0, rank, scale2, floor2, refits, splits, None, None, None, None)

    for essential in (False, True):
        assert lmeds(essential=essential) == 0
        for kw in (dict(p1=None), dict(n=4), dict(n=(1 << 20) + 1), dict(H=0), dict(H=(1 << 20) + 1), dict(rank=0), dict(rank=601),
                   dict(scale2=-1.0), dict(scale2=float("nan")), dict(scale2=float("inf")), dict(floor2=-1.0), dict(floor2=float("nan")),
                   dict(refits=-1), dict(refits=9), dict(splits=-1), dict(splits=3), dict(samples=bad.ctypes.data_as(ip), H=2)):
            assert lmeds(essential=essential, **kw) == EINVAL, (essential, kw)
    assert lmeds(n=7) == EINVAL and lmeds(n=7, rank=5, essential=True) == 0
    assert lmeds(essential=True, Kq=None) == EINVAL
    assert lmeds(essential=True, H=(1 << 20) // 10 + 1) == EINVAL
    # the work cap of the passes, named in the message
    assert lib.alp_epipolar_lmeds(P, P, 1 << 16, None, (1 << 15) + 1, 0, 1, 14.0, 1.0, 0, 0, None, None, None, None) == EINVAL
    assert "2^35" in lib.alp_last_error().decode()
