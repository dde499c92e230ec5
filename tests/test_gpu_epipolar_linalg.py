"""GPU: the linear algebra under the four match filters (epi_solve_kernel and rank2_denorm in alproj_amd/csrc/epi_hypotheses.h,
epi_accum_kernel and epi_refit_kernel in alproj_amd/csrc/alp_epipolar.hip) against the extended-precision references of
tests/linalg_cases.py, case by case at the tolerance rule stated there: d <= max(64 eps, 8 RHO[family] eps kappa), kappa from the
exact spectra of the case and RHO from what float64 delivers on the CPU (tests/test_linalg_cases.py).

what can go wrong                                             where it is held
a pivot lost, a wrong tie, a wrong back substitution          test_solve_families (every free unknown, a row and a column swap
                                                              at every step: asserted on the CPU)
the record of the columns when swaps chain                    test_solve_families (some 170 samples with a displaced swap; the
                                                              planted swap fails the rule on every one on the CPU)
the dropped column of rank 2, near-equal column norms         test_solve_families (each column dropped; motions with s1 ~ s2)
exact zeros in F, an epipole at infinity, another scale       test_solve_families (the motion families)
large, offset and integer coordinates, exact pivot ties       test_solve_families (scaled, offset, integer)
the rank decision and its threshold                           test_solve_ladder (finite above 1e-11, NaN below 1e-15)
one of the 45 packed sums, the order of 256 partial sums      test_refit_families (sizes 8 .. 1025), test_refit_of_70001_matches
a rotation pair missed, a sweep ended early                   test_refit_families (lambda1 at rounding level: 8 matches, noise-free;
                                                              a gap of 1e-6 lambda9: shallow)
the eigenvector chosen when lambda1 rounds negative           test_refit_families (8 matches, noise-free)
the projection to (s, s, 0), K for Hartley's normalisation    test_refit_families (essential: s1 and s2 10 % apart; the constraints)
the refit under LMedS' own bound                              test_refit_families (lmeds)

Every reference is mpmath on the test's own inputs, computed once per module (some 200 solves and 17 refits: seconds).  Each
test prints the device's worst d / (eps kappa) per family next to the allowed figure."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
import essential_cases as es  # noqa: E402
import linalg_cases as lg  # noqa: E402
import lmeds_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def solved(L):
    """Every solve case with its reference and the device's F: one alp_epipolar_solve8 call per scene"""
    cases = lg.solve_references()
    start = 0
    while start < len(cases):
        stop = start
        while stop < len(cases) and cases[stop]["scene"] == cases[start]["scene"]:
            stop += 1
        samples = np.stack([c["sample"] for c in cases[start:stop]]).astype(np.int32)
        assert len(samples) <= 64
        for c, F in zip(cases[start:stop], L.epipolar_solve8(cases[start]["p1"], cases[start]["p2"], samples)):
            c["device"] = F
        start = stop
    return cases


@pytest.fixture(scope="module")
def refitted():
    return lg.refit_references()


def report(rows):
    """rows of (family, d, kappa) -> prints the worst ratio per family; the list of those outside the rule"""
    worst = {}
    for family, d, kappa in rows:
        used, allowed = d / (lg.EPS * kappa), lg.tolerance(family, kappa) / (lg.EPS * kappa)
        if family not in worst or used / allowed > worst[family][0] / worst[family][1]:
            worst[family] = (used, allowed, d, kappa)
    for family, (used, allowed, d, kappa) in worst.items():
        print(f"device {family:22s} d {d:9.3g}  kappa {kappa:9.3g}  d / (eps kappa) {used:9.3g}  allowed {allowed:9.3g}")
    return [(family, d, kappa) for family, d, kappa in rows if not d <= lg.tolerance(family, kappa)]


def unit_norm(F):
    return abs(np.sqrt((F * F).sum()) - 1.0) <= 1e-14


# ------------------------------------------------------------------------------------------------------------ the 8-point solve
def test_solve_families(solved):
    rows = []
    for c in solved:
        if c["family"] == "ladder":
            continue
        assert c["share"] > lg.DECIDED, (c["scene"], c["row"])          # decided: a finite F is owed
        F = c["device"]
        assert np.isfinite(F).all() and unit_norm(F), (c["scene"], c["row"])
        rows.append((c["family"], float(ec.sign_distance(F, c["ref"]["F"])[0]), c["kappa"]))
    assert len(rows) >= 190
    assert report(rows) == []


def test_solve_ladder(solved):
    rows, between = [], 0
    for c in solved:
        if c["family"] != "ladder":
            continue
        F = c["device"]
        if c["share"] > lg.DECIDED:
            assert np.isfinite(F).all() and unit_norm(F), c["row"]
            rows.append((c["family"], float(ec.sign_distance(F, c["ref"]["F"])[0]), c["kappa"]))
        elif c["share"] < lg.UNDECIDED:
            assert np.isnan(F).all(), c["row"]
        else:                     # no accuracy is claimed here, but what is returned is NaN or a fundamental matrix
            between += 1
            assert np.isnan(F).all() or (np.isfinite(F).all() and unit_norm(F) and abs(np.linalg.det(F)) <= 1e-12), c["row"]
    assert len(rows) >= 6 and between <= 4
    assert report(rows) == []


# ------------------------------------------------------------------------------------------------------------ the refit
def device_hypotheses(L, case):
    if case["K"] is None:
        return L.epipolar_solve8(case["p1"], case["p2"], case["samples"])
    f, cx, cy = case["K"]
    return L.epipolar_solve5(case["p1"], case["p2"], case["samples"], f, (cx, cy))[0].reshape(-1, 3, 3)


def device_filter(L, case, cpu):
    p1, p2, samples = case["p1"], case["p2"], case["samples"]
    K = () if case["K"] is None else (case["K"][0], case["K"][1:])
    if case["kind"] == "ransac":
        call = L.epipolar_ransac if case["K"] is None else L.essential_ransac
        return call(p1, p2, *K, case["threshold"], samples=samples, refits=1)
    call = L.epipolar_lmeds if case["K"] is None else L.essential_lmeds
    return call(p1, p2, *K, cpu["rank"], cpu["scale2"], cpu["floor2"], samples=samples, refits=1)


def check_refit(L, r):
    """One refit case on the device -> (family, d, kappa), after the assertions that do not depend on the rule"""
    case, cpu = r["case"], r["cpu"]
    p1, p2 = case["p1"], case["p2"]
    what = f"{case['family']} / {case['name']}"
    # the set the refit sums over, from the DEVICE's F0 with the error expression that the suite holds bit equal to the device's
    dev = lg.restate(case, device_hypotheses(L, case))
    assert dev["chosen"] == cpu["chosen"], what
    np.testing.assert_array_equal(dev["set"], cpu["set"], err_msg=what)          # the reference's inlier set is the device's
    got = device_filter(L, case, cpu)
    info = got["info"]
    assert info["chosen"] == cpu["chosen"] and not info["keep_all"], what
    assert info["refits_run"] == 1 and info["refit_counts"] == cpu["counts"], what
    assert info["refits_kept"] == 1, what                                        # the final F is the refit
    F = got["F"]
    assert np.isfinite(F).all() and unit_norm(F), what
    if case["kind"] == "ransac":
        np.testing.assert_array_equal(got["mask"], ec.inliers(F, p1, p2, case["threshold"]), err_msg=what)
    else:
        bound2 = lc.bound2_of(got["final_value"], cpu["scale2"], cpu["floor2"])
        np.testing.assert_array_equal(got["mask"], lc.errors_inf(F, p1, p2) <= bound2, err_msg=what)
    assert info["final_count"] == int(got["mask"].sum()), what
    if case["K"] is not None:
        res = es.essential_residuals(es.to_essential(F, case["K"]))
        print(what, "essential residuals", res, "allowed", lg.tolerance(case["family"], r["kappa"]))
        assert max(res) <= lg.tolerance(case["family"], r["kappa"]), what
    return case["family"], float(ec.sign_distance(F, r["ref"]["F"])[0]), r["kappa"]


def test_refit_families(L, refitted):
    rows = []
    for r in refitted:
        assert len(r["case"]["samples"]) == 1 and len(r["case"]["p1"]) <= 1400
        rows.append(check_refit(L, r))
    assert {family for family, _, _ in rows} == {f for f in lg.RHO if f.startswith("refit ")} - {"refit large"}
    assert report(rows) == []


def test_refit_of_70001_matches(L):
    """One call: 256 reduce blocks stride over 70 001 matches, 35 001 of them in the sum"""
    (r,) = lg.refit_references(large=True)
    assert len(r["case"]["p1"]) == 70001
    assert report([check_refit(L, r)]) == []
