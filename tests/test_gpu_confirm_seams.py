"""The argmin confirmation of a float32 point set (alp_eval_population_wait; alp_points.hip: confirm_losses) at its own launch
seams.  The scenes, the populations and the restated rules: tests/confirm_cases.py.

The identity: the losses eval_population(..., want_argmin=True) returns for the confirmed candidates of a float32 set are, bit for
bit, the losses of a float64 set that stores the same values -- the same arithmetic on the same numbers, added in the same order
whenever the two launches cut the points into the same stripes.  Up to four rows of 256 points both launch rules give one
stripe per row on any device; above that the float64 set is evaluated on the confirmation's grid (ALP_POP_GRID, read at call
time).  Every case asserts that the band it meant to build is the band the library saw.  The weighted sets carry integer
weights with a zero on the last point, except the set of one point: weights that sum to 0 are refused, so its point weighs 2."""
import numpy as np
import pytest

from alproj_amd import _lib
from tests import confirm_cases as cc

pytestmark = pytest.mark.gpu

N_NAMES = ("1", "255", "256", "257", "1000", "two_row_stripes")


@pytest.fixture(scope="module")
def L():
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def scenes(L):
    """{(point count's name, weighted): (xyz, uv, weights)}, built once"""
    counts = cc.point_counts(L.device_info()["cu_count"])
    return {(name, weighted): cc.scene(counts[name], weighted) for name in N_NAMES for weighted in (False, True)}


def _points(L, xyz, uv, w, prec):
    pts = L.Points(xyz, cc.ORIGIN, prec)
    pts.set_observed(uv)
    if w is not None:
        pts.set_weights(w)
    return pts


@pytest.mark.parametrize("loss", list(cc.LOSSES))
@pytest.mark.parametrize("band", cc.BANDS)
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("n_name", N_NAMES)
def test_confirmed_losses_are_the_float64_sets(L, scenes, monkeypatch, n_name, weighted, band, loss):
    kind, fs = cc.LOSSES[loss]
    xyz, uv, w = scenes[(n_name, weighted)]
    n = len(xyz)
    cu = L.device_info()["cu_count"]
    assert xyz.dtype == uv.dtype == np.float32 and (w is None or (w.dtype == np.float32 and w[-1] == (0.0 if n > 1 else 2.0)))
    cand, near = cc.population(band)
    confirmed = near[:cc.CONFIRM_MAX]
    rest = np.setdiff1d(np.arange(len(cand)), confirmed)

    monkeypatch.delenv("ALP_POP_GRID", raising=False)
    with _points(L, xyz, uv, w, "f32") as p32:
        plain, _ = p32.eval_population(cand, kind, fs, want_argmin=False)
        got, amin = p32.eval_population(cand, kind, fs)
        assert p32.eval_population_info()[0] == "general"
    # the float64 set of the same stored values, on the confirmation's stripes
    stripes = cc.confirm_grid(n, cu)
    if n > 4 * 256:
        monkeypatch.setenv("ALP_POP_GRID", f"{stripes},1")
    with _points(L, xyz.astype(np.float64), uv.astype(np.float64), None if w is None else w.astype(np.float64), "f64") as p64:
        want, _ = p64.eval_population(cand, kind, fs, want_argmin=False)
        assert p64.eval_population_info() == ("general", stripes, 1)
    monkeypatch.delenv("ALP_POP_GRID", raising=False)

    # the guard: the band the library saw is the one meant, and it confirmed the first CONFIRM_MAX of it
    in_band, which = cc.confirm_band(plain)
    differ = int(np.count_nonzero(got != plain))
    print(f"n {n} band {band}: {len(in_band)} in the band, {len(which)} confirmed, {differ} losses replaced; float64 losses "
          f"{len(np.unique(want[near]))} distinct of {band}; largest |got / want - 1| of the confirmed "
          f"{np.abs(got[confirmed] / want[confirmed] - 1).max():.3e}")
    assert in_band == list(near) and which == list(confirmed), (in_band, which)
    assert len(np.unique(want[near])) == band, "every near-tied candidate has its own float64 value"
    assert np.isfinite(plain).all() and np.isfinite(want).all()

    np.testing.assert_array_equal(got[confirmed], want[confirmed])
    np.testing.assert_array_equal(got[rest], plain[rest])
    assert amin == confirmed[int(np.argmin(want[confirmed]))]
