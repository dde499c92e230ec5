"""The numpy restatement of the least-median-of-squares match filter (alp_epipolar_select / alp_epipolar_lmeds /
alp_essential_lmeds in alproj_amd/csrc/alp_epipolar.hip; ``ransac_method="LMEDS"`` of alproj_amd.gcp.filter_geometric) and the
scenes its tests use.  Not a test module: tests/test_lmeds_cases.py holds it to a full sort, to its formulas and to the truth on the
CPU, tests/test_gpu_lmeds.py holds the device to it.

The hypotheses, the error of a match and the refit are those of epipolar_cases and essential_cases, which this module imports and
does not change.  m is the size of a minimal sample: 8 for the fundamental filter, 5 for the essential one."""
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
import essential_cases as es  # noqa: E402

# (n, n_out, scene seed) of the whole-filter tests of the fundamental filter: sigma = 0.5, 2048 samples from
# ec.draw_samples(n, 2048, 1000 + seed).  They are three of epipolar_cases.RANSAC_SCENES' own scenes, kept after checking on the
# restatement alone that for refits 0, 1 and 4 every true inlier is kept, at most 2 % of n outliers are kept (2, 1 and 0 of them,
# at bounds of 3.57, 4.67 and 3.90 px), and every decision is decided (decisions_decided: a device whose refit differs in the last
# bits must go the same way).  The planar essential scene and the large scene were searched the same way over the seeds 1..15.
LMEDS_SCENES = ((500, 200, 7), (64, 24, 4), (300, 120, 74))
LMEDS_SAMPLES = 2048
# (n, n_out, scene seed, planar) of the essential filter: 1024 samples from es.draw_samples5(n, 1024, 1000 + seed)
LMEDS5_SCENES = ((64, 24, 7, False), (110, 10, 1, True))
LMEDS5_SAMPLES = 1024
# more than half outliers: (n, n_out, scene seed, planar, quantile).  The median of the errors then belongs to an outlier under
# every hypothesis; a quantile below the inlier share (0.3 here) is what the parameter is for.
LMEDS5_LOW_SHARE = (400, 280, 5, False, 0.25)

# the large scene: ec.scene(500, 100, 0.5, seed) repeated 140 times and its first match once more, 70 001 matches (a scene of
# that many distinct matches always has an error within 1 % of its bound, and nothing would be decided), with 256 samples of 8
LARGE_SCENE = (500, 100, 15, 140, 256)
OUTLIER_CAP = 0.02            # of n: the outliers a filter may keep on these scenes (a cap, not a measurement)
MARGIN = 0.01                 # relative: what two numerical routes to one refit may not come closer to than this is decided

# The tolerance of a refit's value on the device.  Measured on the CPU (tests/test_lmeds_cases.py prints and asserts it): the
# relative distance between two numpy routes to the value of the first refit's candidate, the eigenvector of the smallest eigenvalue
# of A^T A by numpy.linalg.eigh against the last right singular vector of A by numpy.linalg.svd, is at most 1.5e-10 over the scenes
# above (1.44e-10 on the planar essential scene, 4.0e-11 on the other essential one, 3.2e-12 and less on the fundamental ones).  The device, with another summation order and Jacobi rotations, gets 100 times that.
SELF_DISTANCE = 1.5e-10
VALUE_TOL = 100 * SELF_DISTANCE


def rank_of(n, m, quantile=0.5):
    """The 1-based rank of the order statistic that is a hypothesis' value; m + 1 whatever the quantile below n = 2 (m + 1)."""
    return int(min(n, max(m + 1, math.ceil(quantile * n))))


def scale2_of(n, m, quantile=0.5):
    """(2.5 * (1 / Phi^-1((1 + quantile) / 2)) * (1 + 5 / (n - m)))^2; quantile = 1: 0.0"""
    if quantile >= 1.0:
        return 0.0
    scale = 2.5 * (1.0 / statistics.NormalDist().inv_cdf((1.0 + quantile) / 2.0)) * (1.0 + 5.0 / (n - m))
    return scale * scale


def errors_inf(F, p1, p2):
    """ec.errors with a NaN error (and every error of a NaN F) as +inf"""
    e = ec.errors(F, p1, p2)
    return np.where(np.isnan(e), np.inf, e)


def values(Fs, p1, p2, r):
    """The r-th smallest error (1-based) of every F, by numpy.partition"""
    return np.array([np.partition(errors_inf(F, p1, p2), r - 1)[r - 1] for F in np.asarray(Fs).reshape(-1, 3, 3)])


def bound2_of(v, scale2, floor2):
    return max(scale2 * v, floor2)


def lmeds(p1, p2, Fs, m, quantile=0.5, min_threshold=1.0, refits=4, K=None, refit=None):
    """The whole filter on given hypotheses ``Fs`` (any shape (..., 3, 3); the essential filter's (H, 10, 3, 3) flatten to the slot
    index h * 10 + slot) -> dict chosen, values (of every hypothesis), value (the chosen one), final_value, bound (pixels),
    bound2, refit_values (of every refit run, the rejected last one included), refits_kept, mask, keep_all, F, and for the tests'
    margins path (the chosen F and every candidate), path_values, sets (the inlier set every refit was fitted to).
    ``refit``: mask -> F; by default ec.refit with Hartley's normalisation of all points, or es.refit5 with ``K``."""
    n = len(p1)
    if refit is None:
        if K is None:
            n1, n2 = ec.hartley(p1), ec.hartley(p2)
            refit = lambda mask: ec.refit(p1, p2, mask, n1, n2)  # noqa: E731
        else:
            refit = lambda mask: es.refit5(p1, p2, mask, K)  # noqa: E731
    r, scale2, floor2 = rank_of(n, m, quantile), scale2_of(n, m, quantile), float(min_threshold) * float(min_threshold)
    Fs = np.asarray(Fs).reshape(-1, 3, 3)
    v = values(Fs, p1, p2, r)
    k = int(np.argmin(v))                       # the lowest index on a tie
    F, value = Fs[k], float(v[k])
    out = {"chosen": k, "values": v, "value": value, "refit_values": [], "refits_kept": 0, "keep_all": not np.isfinite(value),
           "rank": r, "scale2": scale2, "floor2": floor2, "path": [F], "path_values": [value], "sets": []}
    b2 = bound2_of(value, scale2, floor2)
    if not out["keep_all"]:
        for _ in range(refits):
            inl = errors_inf(F, p1, p2) <= b2
            G = refit(inl)
            vg = float(values(G, p1, p2, r)[0])
            out["sets"].append(inl), out["path"].append(G), out["path_values"].append(vg), out["refit_values"].append(vg)
            if not vg < value:
                break
            F, value, b2 = G, vg, bound2_of(vg, scale2, floor2)
            out["refits_kept"] += 1
    out["F"], out["final_value"], out["bound2"], out["bound"] = F, value, b2, math.sqrt(b2) if np.isfinite(b2) else math.inf
    out["mask"] = np.ones(n, dtype=bool) if out["keep_all"] else errors_inf(F, p1, p2) <= b2
    return out


def decisions_decided(out, p1, p2):
    """(ok, why): True when a device whose refit candidates differ from the restatement's in the last bits must take the same
    decisions and return the same mask.  A refit decision is decided when the candidate was fitted to the same inlier set as the
    round before (bit-equal inputs give the bit-equal candidate on either side, so the value is equal and the loop stops), or
    when its value and the current one differ by more than MARGIN (1 %) relative.  An inlier set, the final mask included, is
    decided when under its F no error lies within MARGIN of that F's b2."""
    if out["keep_all"]:
        return True, ""
    value = out["path_values"][0]
    for k, vg in enumerate(out["refit_values"]):
        same_set = k > 0 and np.array_equal(out["sets"][k], out["sets"][k - 1])
        if not same_set and not abs(vg - value) > MARGIN * max(vg, value):
            return False, f"refit {k}: value {vg!r} against {value!r}"
        if vg < value:
            value = vg
    # the matrices whose inlier sets were used: the chosen one, every kept candidate (the last of them gives the mask)
    used, value = [(out["path"][0], out["path_values"][0])], out["path_values"][0]
    for G, vg in zip(out["path"][1:], out["refit_values"]):
        if vg < value:
            used.append((G, vg))
            value = vg
    for F, v in used:
        b2 = bound2_of(v, out["scale2"], out["floor2"])
        e = errors_inf(F, p1, p2)
        if (np.abs(e - b2) <= MARGIN * b2).any():
            return False, f"an error within {MARGIN} of b2 = {b2!r}"
    return True, ""


def truth(out, is_outlier):
    """(true inliers lost, outliers kept) of a result"""
    return int((~out["mask"] & ~is_outlier).sum()), int((out["mask"] & is_outlier).sum())


def refit_value_routes(p1, p2, inl, r, K=None):
    """The value of the refit on the inlier set ``inl`` by two numpy routes to the null vector of the design matrix A: eigh of
    A^T A (what ec.refit and es.refit5 do) and svd of A -> (value by eigh, value by svd)"""
    if K is None:
        n1, n2 = ec.hartley(p1), ec.hartley(p2)
        A = ec._design((p1[inl] - n1[0]) * n1[1], (p2[inl] - n2[0]) * n2[1])
        finish = lambda f: ec._rank2_denorm(f, n1, n2)  # noqa: E731
    else:
        A = es._design(es.normalise(p1[inl], K), es.normalise(p2[inl], K))
        finish = lambda f: es.denormalise(es.project_essential(f.reshape(3, 3)), K)  # noqa: E731
    _, V = np.linalg.eigh(A.T @ A)
    _, _, Vt = np.linalg.svd(A, full_matrices=False)
    return float(values(finish(V[:, 0]), p1, p2, r)[0]), float(values(finish(Vt[8]), p1, p2, r)[0])


def fundamental_scene(n, n_out, seed, sigma=0.5):
    """-> (p1, p2, is_outlier, samples (2048, 8)) of an LMEDS_SCENES row"""
    p1, p2, _, outlier = ec.scene(n, n_out, sigma, seed)
    return p1, p2, outlier, ec.draw_samples(n, LMEDS_SAMPLES, 1000 + seed)


def essential_scene(n, n_out, seed, planar, sigma=0.5):
    """-> (p1, p2, is_outlier, samples (1024, 5)) of an LMEDS5_SCENES row"""
    p1, p2, _, outlier = es.make_scene(n, n_out, sigma, seed, planar)
    return p1, p2, outlier, es.draw_samples5(n, LMEDS5_SAMPLES, 1000 + seed)


# F with e = (y1 - y2)^2 exactly: l2 = (0, -1, y1), l1 = (0, 1), s = y1 - y2, both denominators 1
F_ROWS = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])


def placed(errors_sqrt, rng=None):
    """Matches whose error under F_ROWS is exactly errors_sqrt^2 (where that square is exact): y1 = errors_sqrt, y2 = 0, x free"""
    y = np.asarray(errors_sqrt, dtype=np.float64)
    x = np.arange(len(y), dtype=np.float64) if rng is None else rng.uniform(0.0, 1000.0, len(y))
    p1 = np.stack([x, y], axis=1)
    p2 = np.stack([x[::-1].copy(), np.zeros(len(y))], axis=1)
    return np.ascontiguousarray(p1), np.ascontiguousarray(p2)


def large_scene():
    """-> (p1, p2, is_outlier, samples (256, 8)) of LARGE_SCENE: the samples are drawn in the first copy and moved to copy
    h mod 140, so that they reach over all match tiles"""
    n0, n_out, seed, copies, H = LARGE_SCENE
    q1, q2, _, outlier = ec.scene(n0, n_out, 0.5, seed)
    idx = np.r_[np.tile(np.arange(n0), copies), 0]
    samples = (ec.draw_samples(n0, H, 1000 + seed) + n0 * (np.arange(H) % copies)[:, None]).astype(np.int32)
    return np.ascontiguousarray(q1[idx]), np.ascontiguousarray(q2[idx]), outlier[idx], samples
