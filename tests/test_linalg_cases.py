"""CPU: the cases and the yardsticks of tests/linalg_cases.py.  The float64 routes (numpy's and the kernels' algorithms restated)
stay within RHO of the extended-precision references; the solve cases reach every free unknown, a row and a column swap at every
elimination step, displaced column swaps and each dropped column; the ladder's rungs fall where the GPU test expects them; every
refit case meets its preconditions; and the rule has teeth: a wrong column record, a rotation pair never visited and a Jacobi
stopped after one sweep each fail it on these inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
import essential_cases as es  # noqa: E402
import linalg_cases as lg  # noqa: E402

# What this module's own assertion on the routes allows above RHO: another BLAS build moves the last bits of numpy's SVD and eigh
# and of the A^T A that both routes start from.  It does not enter lg.tolerance(): the device is held to RHO itself.
BLAS_HEADROOM = 1.25
# RHO is the figure measured here rounded UP to two digits (at most a tenth above it), so with the headroom the other way a
# constant more than this above what is measured is not the measured one
RHO_GUARD = 1.1 * BLAS_HEADROOM


@pytest.fixture(scope="module")
def solved():
    return lg.solve_references()


@pytest.fixture(scope="module")
def refitted():
    out = lg.refit_references() + lg.refit_references(large=True)
    for r in out:
        r["d_numpy"], r["d_route"] = lg.route_distances(r["case"], r["cpu"]["set"], r["ref"])
    return out


def dist(F, ref):
    return float(ec.sign_distance(F, ref["F"])[0])


def test_routes_stay_within_rho(solved, refitted):
    """The worst d / (EPS kappa) of both float64 routes per family: printed (RHO is these figures rounded up to two digits) and
    held, with BLAS_HEADROOM for another build of the libraries under numpy"""
    worst = {}
    for c in solved:
        if c["share"] > lg.DECIDED:
            assert np.isfinite(c["numpy"]).all() and np.isfinite(c["route"]).all(), (c["scene"], c["row"])
            rho = max(dist(c["numpy"], c["ref"]), dist(c["route"], c["ref"])) / (lg.EPS * c["kappa"])
            worst[c["family"]] = max(worst.get(c["family"], 0.0), rho)
    for r in refitted:
        rho = max(r["d_numpy"], r["d_route"]) / (lg.EPS * r["kappa"])
        worst[r["case"]["family"]] = max(worst.get(r["case"]["family"], 0.0), rho)
    for family, rho in worst.items():
        print(f"rho {family:24s} {rho:10.3g}   RHO {lg.RHO[family]:10.3g}")
    assert set(worst) == set(lg.RHO)
    for family, rho in worst.items():
        assert rho <= BLAS_HEADROOM * lg.RHO[family], family
        assert lg.RHO[family] <= RHO_GUARD * rho, f"RHO of {family} is above the measured figure"


def test_exact_solve_is_a_solution(solved):
    """The reference against its own definition, in float64: unit norm, rank 2, and the sample on its lines as far as rank 2
    allows: the null vector f meets every row of the design matrix, and rank 2 takes s3 u3 v3^T from it, so in normalised
    coordinates |b^T G a| <= s3 |a| |b| for G at the norm sqrt(s1^2 + s2^2) that the truncation leaves of a unit f."""
    for c in solved:
        if c["share"] <= lg.DECIDED:
            continue
        F, (s1, s2, s3) = c["ref"]["F"], c["ref"]["s"]
        assert abs(np.sqrt((F * F).sum()) - 1.0) <= 4 * lg.EPS and abs(np.linalg.det(F)) <= 1e-15
        T1, T2 = (ec._transform(*norm) for norm in c["norms"])
        G = np.linalg.inv(T2).T @ F @ np.linalg.inv(T1)
        G *= np.sqrt(s1 * s1 + s2 * s2) / np.sqrt((G * G).sum())
        a = (T1 @ np.c_[c["p1"][c["sample"]], np.ones(8)].T).T
        b = (T2 @ np.c_[c["p2"][c["sample"]], np.ones(8)].T).T
        residual = np.abs(np.einsum("ij,jk,ik->i", b, G, a))
        bound = s3 * np.sqrt((a * a).sum(axis=1) * (b * b).sum(axis=1))
        assert (residual <= bound * (1.0 + 1e-9) + 1e-11).all(), (c["scene"], c["row"], residual, bound)


def test_coverage_of_the_elimination(solved):
    """What the solve families reach, so that no coverage family is needed on top of them"""
    full = [c["info"] for c in solved if "free" in c["info"]]
    assert {i["free"] for i in full} == set(range(9))
    assert {i["drop"] for i in full} == {0, 1, 2}
    rows = {k for i in full for k, (r, _) in enumerate(i["pivots"]) if r != k}
    cols = {k for i in full for k, (_, c) in enumerate(i["pivots"]) if c != k}
    assert rows == set(range(7))          # (step 7 has one row left: no swap can happen there)
    assert cols == set(range(8))
    assert sum(i["displaced"] for i in full) >= 64 and sum(not i["displaced"] for i in full) >= 8
    ties = [c for c in solved if c["family"] == "integer"]
    assert ties and all(np.array_equal(c["p1"], np.trunc(c["p1"])) for c in ties)


def test_ladder_rungs(solved):
    share = np.array([c["share"] for c in solved if c["family"] == "ladder"])
    assert len(share) == 14 and (np.diff(share) < 0).all()
    assert (share > lg.DECIDED).sum() >= 6 and (share < lg.UNDECIDED).sum() >= 2 and share[-1] < 1e-40
    assert ((share <= lg.DECIDED) & (share >= lg.UNDECIDED)).sum() <= 4
    for c in solved:          # the kernel's route decides as the GPU test will ask the device to
        if c["family"] == "ladder" and c["share"] < lg.UNDECIDED:
            assert np.isnan(c["route"]).all()


def test_refit_preconditions(refitted):
    """Every case: the refit kept, every decision decided, kappa within the cap, and what the case itself requires"""
    sizes, totals, kinds = set(), set(), set()
    for r in refitted:
        case, cpu, ref = r["case"], r["cpu"], r["ref"]
        what, require, lam, s = f"{case['family']} / {case['name']}", case["require"], ref["lam"], ref["s"]
        assert cpu["kept"] and cpu["decided"] and lg.usable(case), what
        assert r["kappa"] <= lg.KAPPA_CAP, what
        assert len(case["samples"]) == 1 and len(case["p1"]) <= require.get("n", 1025), what
        assert set(require) <= {"n", "set", "null", "gap", "s12"}, what
        if "set" in require:
            assert int(cpu["set"].sum()) == require["set"], what
        if "null" in require:          # lambda1 at rounding level and a wide gap
            assert abs(lam[0]) <= require["null"] * lam[8] and lam[1] > 1e-9 * lam[8], what
        if "gap" in require:
            assert require["gap"][0] <= (lam[1] - lam[0]) / lam[8] <= require["gap"][1], what
        if "s12" in require:
            assert (s[0] - s[1]) / s[0] > require["s12"], what
        sizes.add(require.get("set")), totals.add(require.get("n", 1025)), kinds.update(require)
    # the sizes of the issue, the two cases beyond 1025 matches, and each special requirement somewhere
    assert sizes >= {8, 9, 64, 257, 513, 1025, 35001}
    assert totals == {1025, 1400, 70001}
    assert {"null", "gap", "s12"} <= kinds


def test_essential_refits_meet_the_constraints(refitted):
    for r in refitted:
        case = r["case"]
        if case["K"] is not None:
            n1, n2 = lg.norms_of(case)
            tol = lg.tolerance(case["family"], r["kappa"])
            for F in (r["ref"]["F"], lg.refit_route(case["p1"], case["p2"], r["cpu"]["set"], n1, n2, True)):
                res = es.essential_residuals(es.to_essential(F, case["K"]))
                print(case["name"], "residuals", res, "allowed", tol)
                assert max(res) <= tol


def test_a_wrong_column_record_fails_the_rule(solved):
    """swap_unchained in place of the swap: bit equal on every sample without a displaced swap, outside the rule on every sample
    with one.  The x translation alone is left out of the second half: its F has exact zeros, and two unknowns that are both
    zero can change places."""
    displaced = failed = 0
    for c in solved:
        if "free" not in c["info"] or c["share"] <= lg.DECIDED:
            continue
        F, _ = lg.solve8_route(c["p1"], c["p2"], c["sample"], *c["norms"], swap=lg.swap_unchained)
        if not c["info"]["displaced"]:
            np.testing.assert_array_equal(F, c["route"])
        elif c["family"] != "motion x translation":
            displaced += 1
            failed += not dist(F, c["ref"]) <= lg.tolerance(c["family"], c["kappa"])
    print("displaced", displaced, "outside the rule with the planted swap", failed)
    assert failed == displaced >= 64


@pytest.mark.parametrize("plant", [dict(skip=(2, 5)), dict(sweeps=1)])
def test_a_crippled_jacobi_fails_the_rule(refitted, plant):
    """One of the 36 pairs never rotated (the other rotations carry most of its entry away: few cases notice), or one sweep"""
    failed = []
    for r in refitted:
        case = r["case"]
        if case["name"] == "70 001":
            continue
        n1, n2 = lg.norms_of(case)
        F = lg.refit_route(case["p1"], case["p2"], r["cpu"]["set"], n1, n2, case["K"] is not None, **plant)
        if not dist(F, r["ref"]) <= lg.tolerance(case["family"], r["kappa"]):
            failed.append(case["name"])
    print(plant, "outside the rule:", failed)
    assert len(failed) >= 1


@pytest.mark.parametrize("essential", [False, True])
def test_whole_filter_fits_stay_within_their_family(essential):
    """The final F of every scene of tests/test_gpu_epipolar.py::test_ransac_equals_the_restatement and
    tests/test_gpu_essential.py::test_ransac5_equals_the_restatement, which hold the device's to the rule with a family's RHO
    borrowed from the cases above: the restatement's own lies within that RHO.  (An essential scene without a kept refit has no
    reference here: its F is the five-point solver's, held elsewhere.)"""
    families = []
    for scene in (es.RANSAC5_SCENES if essential else ec.RANSAC_SCENES):
        n, n_out, threshold, seed = scene[:4]
        if essential:
            p1, p2, _, _ = es.make_scene(n, n_out, 0.5, seed, scene[4])
            samples = es.draw_samples5(n, es.RANSAC5_SAMPLES, 1000 + seed)
            want = es.ransac5(p1, p2, samples, es.K_TRUE, threshold)
        else:
            p1, p2, _, _ = ec.scene(n, n_out, 0.5, seed)
            samples = ec.draw_samples(n, 2048, 1000 + seed)
            want = ec.ransac(p1, p2, samples, threshold)
        exact = lg.whole_filter_reference(p1, p2, samples, want, threshold, es.K_TRUE if essential else None)
        families.append(None if exact is None else exact[2])
        if exact is not None:
            ref, kappa, family = exact
            rho = dist(want["F"], ref) / (lg.EPS * kappa)
            print(scene, family, "kappa", kappa, "rho", rho)
            assert rho <= BLAS_HEADROOM * lg.RHO[family], scene
    assert families == (["refit essential", None, None, None] if essential else ["refit sizes", "general", "general", "general"])
