"""Extended-precision references for the linear algebra of the match filters (alproj_amd/csrc/epi_hypotheses.h: epi_solve_kernel
and rank2_denorm; alproj_amd/csrc/alp_epipolar.hip: epi_accum_kernel and epi_refit_kernel), two float64 restatements of the kernels'
own routes, the condition number of every case and the case families.  Not a test module: tests/test_linalg_cases.py holds the
float64 routes to the references on the CPU and asserts what the cases cover, tests/test_gpu_epipolar_linalg.py holds the device to
the references.

The references run in mpmath at DPS digits on the float64 inputs as they are given: nothing is rounded before the last step.
F is (3, 3) float64 at unit Frobenius norm with b^T F a = 0, as in epipolar_cases; a norm is (centre (2,), scale), Hartley's of all
points or, for the essential filter, ((cx, cy), 1 / f).

The tolerance rule.  A result may lie d = sign_distance(F, F_exact) <= max(FLOOR, MARGIN * RHO[family] * EPS * kappa) from the
reference, kappa being the case's own condition number from the exact spectra:
    solve   sigma1 / sigma8 of the 8 x 9 matrix  +  s1 / (s2 - s3) of its 3 x 3 null vector
    refit   lambda9 / (lambda2 - lambda1) of the 9 x 9 sum  +  s1 / (s2 - s3) of its eigenvector
RHO[family] is the worst d / (EPS * kappa) of the float64 routes on the CPU (numpy's SVD / eigh and the kernels' algorithms
restated below) over the family, measured and rounded up to two digits; tests/test_linalg_cases.py asserts that the routes stay
within RHO itself (with a stated headroom of its own for another BLAS build, which does not enter the device's tolerance).
MARGIN = 8 is what the device gets on top: it differs from a float64 run of the same algorithm by fused
multiply-adds and the order of the partial sums, which change rounding and not conditioning, while a lost pivot, a missed
rotation pair or an early stop cost orders of magnitude (test_linalg_cases.py plants each and sees it fail the rule)."""
import math
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
import essential_cases as es  # noqa: E402
import lmeds_cases as lc  # noqa: E402

DPS = 50
EPS = 2.0 ** -52
MARGIN = 8.0
FLOOR = 64 * EPS
PIVOT_SHARE = 1e-13           # the kernel's EPI_RANK_TOL
DECIDED, UNDECIDED = 1e-11, 1e-15     # sigma8 / sigma1 above DECIDED: a finite F is owed; below UNDECIDED: NaN is owed

# The worst d / (EPS * kappa) of the float64 routes per family (numpy's route and the kernel's route against the exact
# reference), measured by tests/test_linalg_cases.py::test_routes_stay_within_rho, which prints them; each constant is the measured
# figure rounded up to two digits.  The offset and the scaled coordinates, and each motion, amplify the denormalisation by a
# constant of their own, hence a figure per family (the x translation's exact F has zeros where T2^T f T1 cancels).
RHO = {
    "general": 0.35,                # measured 0.35
    "motion x translation": 31,     # measured 30.1
    "motion forward": 2.2,          # measured 2.16
    "motion roll 90": 0.0038,       # measured 0.00374
    "motion zoom 2": 0.013,         # measured 0.0121
    "scaled": 0.036,                # measured 0.035
    "offset": 0.036,                # measured 0.035
    "integer": 0.097,               # measured 0.096
    "ladder": 0.0019,               # measured 0.00188
    "outliers": 0.75,               # measured 0.75
    "refit sizes": 0.0054,          # measured 0.0053
    "refit noise-free": 0.0028,     # measured 0.00276
    "refit scaled": 0.002,          # measured 0.00194
    "refit offset": 0.0077,         # measured 0.00767
    "refit integer": 2.4,           # measured 2.35
    "refit shallow": 0.0052,        # measured 0.00518
    "refit essential": 0.015,       # measured 0.0141
    "refit lmeds": 0.0011,          # measured 0.00108
    "refit large": 0.005,           # measured 0.00491
}
KAPPA_CAP = 1e8               # no refit case is worse conditioned than this


def tolerance(family, kappa):
    return max(FLOOR, MARGIN * RHO[family] * EPS * kappa)


def hartley_norms(p1, p2):
    return ec.hartley(p1), ec.hartley(p2)


def essential_norm(K=es.K_TRUE):
    f, cx, cy = K
    return (np.array([cx, cy]), 1.0 / f)


# ------------------------------------------------------------------------------------------------------------ exact references
def _mp_transform(norm):
    c, s = norm
    c0, c1, s = mp.mpf(float(c[0])), mp.mpf(float(c[1])), mp.mpf(float(s))
    return mp.matrix([[s, 0, -s * c0], [0, s, -s * c1], [0, 0, 1]])


def _mp_finish(f, norm1, norm2, essential):
    """f: 9 mp numbers, a 3 x 3 matrix in normalised coordinates -> (F float64, (s1, s2, s3) float64)"""
    U, S, V = mp.svd_r(mp.matrix([f[0:3], f[3:6], f[6:9]]))
    s = [S[0], S[1], S[2]]
    kept = [(s[0] + s[1]) / 2] * 2 + [0] if essential else [s[0], s[1], 0]
    G = U * mp.diag(kept) * V
    F = _mp_transform(norm2).T * G * _mp_transform(norm1)
    fro = mp.sqrt(sum(F[i, j] ** 2 for i in range(3) for j in range(3)))
    F = np.array([[float(F[i, j] / fro) for j in range(3)] for i in range(3)])
    return F, np.array([float(x) for x in s])


def solve8_exact(p1, p2, sample, norm1, norm2):
    """The 8-point solve of one sample -> dict F, sigma (8,): the singular values of the 8 x 9 matrix, s (3,): those of the null
    vector.  The null vector is the last right singular vector by mp.svd_r; rank 2 by mp.svd_r again."""
    with mp.workdps(DPS):
        rows = []
        for i in sample:
            x1, y1 = ((mp.mpf(float(p1[i, k])) - mp.mpf(float(norm1[0][k]))) * mp.mpf(float(norm1[1])) for k in range(2))
            x2, y2 = ((mp.mpf(float(p2[i, k])) - mp.mpf(float(norm2[0][k]))) * mp.mpf(float(norm2[1])) for k in range(2))
            rows.append([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, mp.mpf(1)])
        rows.append([mp.mpf(0)] * 9)                  # a square matrix: all nine right singular vectors
        _, S, V = mp.svd_r(mp.matrix(rows))
        sigma = np.array([float(S[i]) for i in range(8)])
        F, s = _mp_finish([V[8, j] for j in range(9)], norm1, norm2, False)
    return {"F": F, "sigma": sigma, "s": s}


def _dyadic(x):
    """float64 values -> (Python ints, shift) with x = ints * 2^-shift exactly"""
    x = np.asarray(x, dtype=np.float64).ravel()
    m, e = np.frexp(x)
    mi = (m * 2.0 ** 53).astype(np.int64)
    e = e.astype(np.int64) - 53
    lo = int(e.min())
    return [int(a) << int(b - lo) for a, b in zip(mi, e)], -lo


def _exact_coordinates(p, norm):
    """(x - c) * s of every row of p as exact integers at one shift -> (xs, ys, shift)"""
    ints, sh = _dyadic(np.r_[p.ravel(), norm[0]])
    (s,), ss = _dyadic([norm[1]])
    cx, cy = ints[-2], ints[-1]
    return [(v - cx) * s for v in ints[0:-2:2]], [(v - cy) * s for v in ints[1:-2:2]], sh + ss


def sum9_exact(p1, p2, mask, norm1, norm2):
    """The 9 x 9 sum of the design rows' outer products over ``mask``: every entry exact (integer arithmetic on the dyadic
    inputs), then one rounding to DPS digits -> mp.matrix.  Call inside mp.workdps."""
    x1, y1, sh1 = _exact_coordinates(p1[mask], norm1)
    x2, y2, sh2 = _exact_coordinates(p2[mask], norm2)
    sh = max(sh1, sh2)
    x1, y1 = (np.array([v << (sh - sh1) for v in c], dtype=object) for c in (x1, y1))
    x2, y2 = (np.array([v << (sh - sh2) for v in c], dtype=object) for c in (x2, y2))
    one = 1 << sh
    cols = [x2 * x1, x2 * y1, x2 * one, y2 * x1, y2 * y1, y2 * one, x1 * one, y1 * one, np.array([one * one] * len(x1), dtype=object)]
    M = mp.matrix(9, 9)
    for i in range(9):
        for j in range(i, 9):
            M[i, j] = M[j, i] = mp.ldexp(mp.mpf(int((cols[i] * cols[j]).sum())), -4 * sh)
    return M


def refit_exact(p1, p2, mask, norm1, norm2, essential=False):
    """The refit on the matches of ``mask`` -> dict F, lam (9,) ascending, s (3,): the eigenvector of the smallest eigenvalue of
    the 9 x 9 sum by mp.eigsy, projected to rank 2 (essential: to (s, s, 0)) and denormalised."""
    with mp.workdps(DPS):
        E, Q = mp.eigsy(sum9_exact(p1, p2, mask, norm1, norm2))
        order = sorted(range(9), key=lambda k: E[k])
        lam = np.array([float(E[k]) for k in order])
        F, s = _mp_finish([Q[j, order[0]] for j in range(9)], norm1, norm2, essential)
    return {"F": F, "lam": lam, "s": s}


def kappa_solve(ref):
    with np.errstate(divide="ignore"):
        return float(ref["sigma"][0] / ref["sigma"][7] + ref["s"][0] / (ref["s"][1] - ref["s"][2]))


def kappa_refit(ref):
    with np.errstate(divide="ignore"):
        return float(ref["lam"][8] / (ref["lam"][1] - ref["lam"][0]) + ref["s"][0] / (ref["s"][1] - ref["s"][2]))


# ------------------------------------------------------------------------------------------------------------ the kernels' routes
def _transform(norm):
    return ec._transform(*norm)


def normalised_design(p1, p2, idx, norm1, norm2):
    return ec._design((p1[idx] - norm1[0]) * norm1[1], (p2[idx] - norm2[0]) * norm2[1])


def _rotation(app, aqq, apq):
    """(cos, sin) of the angle theta in [-pi / 4, pi / 4] with tan 2 theta = 2 a_pq / (a_qq - a_pp): the plane rotation
    [[c, s], [-s, c]] of the columns p, q that zeroes a_pq"""
    d = float(aqq - app)
    theta = 0.5 * math.atan2(2.0 * apq, d) if d >= 0.0 else 0.5 * math.atan2(-2.0 * apq, -d)
    return math.cos(theta), math.sin(theta)


def rank2_route(f, norm1, norm2, essential=False):
    """A one-sided Jacobi on the three columns of f: pairs (0, 1), (0, 2), (1, 2) are rotated until orthogonal (16 sweeps at
    most), the column of the smallest norm is dropped (the first on a tie), the essential projection scales the two others to
    the mean of their norms; then T2^T . T1 and unit norm -> (F, the dropped column)."""
    g, v = np.array(f, dtype=np.float64).reshape(3, 3), np.eye(3)
    for _ in range(16):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            gram = g[:, [p, q]].T @ g[:, [p, q]]          # the columns are orthogonal when its off-diagonal entry vanishes
            if gram[0, 1] != 0.0 and abs(gram[0, 1]) > 1e-17 * math.sqrt(gram[0, 0] * gram[1, 1]):
                rotated = True
                c, sn = _rotation(gram[0, 0], gram[1, 1], gram[0, 1])
                rot = np.array([[c, sn], [-sn, c]])
                g[:, [p, q]] = g[:, [p, q]] @ rot
                v[:, [p, q]] = v[:, [p, q]] @ rot
        if not rotated:
            break
    norms = np.sqrt((g * g).sum(axis=0))
    drop = int(np.argmin(norms))
    scale = np.ones(3)
    if essential:
        with np.errstate(all="ignore"):
            scale = 0.5 * (norms.sum() - norms[drop]) / norms
    scale[drop] = 0.0
    with np.errstate(all="ignore"):
        F = _transform(norm2).T @ ((g * scale) @ v.T) @ _transform(norm1)
        fro = np.sqrt((F * F).sum())
    if not (np.isfinite(fro) and fro > 0.0):
        return np.full((3, 3), np.nan), drop
    return F / fro, drop


def swap_entries(perm, k, j):
    perm[k], perm[j] = perm[j], perm[k]


def solve8_route(p1, p2, sample, norm1, norm2, swap=swap_entries):
    """The kernel's route in float64: Gaussian elimination of the 8 x 9 matrix with complete pivoting (the first largest entry
    in row-major order of what is left), a rank below 8 when a pivot is not above PIVOT_SHARE of the first, the null vector by
    back substitution from 1 in the last column, rank 2 by rank2_route -> (F, info): info holds pivots (the (row, column) of
    every step's pivot), free (the unknown left in the last column), drop (rank2_route's) and displaced (a swap fetched a
    column whose unknown was not at home: an earlier swap had put another there), or only pivots when the rank is below 8.
    ``swap`` updates the record of which unknown stands in which column (the tests plant a wrong one)."""
    A = normalised_design(p1, p2, np.asarray(sample), norm1, norm2)
    perm, home, pivots, displaced = list(range(9)), list(range(9)), [], False
    for k in range(8):
        rest = np.abs(A[k:, k:])
        i, j = np.unravel_index(int(np.argmax(rest)), rest.shape)
        if k == 0:
            first = rest[i, j]
        if not rest[i, j] > first * PIVOT_SHARE or not np.isfinite(rest[i, j]):
            return np.full((3, 3), np.nan), {"pivots": pivots}
        i, j = int(i) + k, int(j) + k
        pivots.append((i, j))
        A[[k, i]] = A[[i, k]]
        if j != k:
            A[:, [k, j]] = A[:, [j, k]]
            displaced = displaced or home[j] != j
            swap(perm, k, j)
            swap_entries(home, k, j)
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k] / A[k, k], A[k, k + 1:])
    y = np.zeros(9)
    y[8] = 1.0
    for k in range(7, -1, -1):
        y[k] = -(A[k, k + 1:] @ y[k + 1:]) / A[k, k]
    f = np.zeros(9)
    f[perm] = y
    F, drop = rank2_route(f, norm1, norm2)
    return F, {"pivots": pivots, "free": perm[8], "drop": drop, "displaced": displaced}


def jacobi_smallest(M, skip=None, sweeps=40):
    """The eigenvector of the smallest eigenvalue of a symmetric matrix by the cyclic two-sided Jacobi method: every pair (p, q)
    with p < q in row order, a rotation wherever |a_pq| > 1e-17 sqrt(|a_pp| |a_qq|), until a sweep rotates nothing (``sweeps`` at
    most); the column whose diagonal entry is smallest.  ``skip``: a pair that is never rotated (the tests plant it)."""
    M = np.array(M, dtype=np.float64)
    n = len(M)
    V = np.eye(n)
    for _ in range(sweeps):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = M[p, q]
                if (p, q) == skip or apq == 0.0 or not abs(apq) > 1e-17 * math.sqrt(abs(M[p, p]) * abs(M[q, q])):
                    continue
                rotated = True
                c, sn = _rotation(M[p, p], M[q, q], apq)
                rot = np.array([[c, sn], [-sn, c]])
                M[:, [p, q]] = M[:, [p, q]] @ rot
                M[[p, q], :] = rot.T @ M[[p, q], :]
                V[:, [p, q]] = V[:, [p, q]] @ rot
                M[p, q] = M[q, p] = 0.0
        if not rotated:
            break
    return V[:, int(np.argmin(np.diag(M)))]


def refit_route(p1, p2, mask, norm1, norm2, essential=False, skip=None, sweeps=40):
    """The kernel's route in float64: the 9 x 9 sum in float64, jacobi_smallest, rank2_route -> F"""
    A = normalised_design(p1, p2, mask, norm1, norm2)
    return rank2_route(jacobi_smallest(A.T @ A, skip, sweeps), norm1, norm2, essential)[0]


def refit_numpy(p1, p2, mask, norm1, norm2, K=None):
    """numpy's route: ec.refit, or es.refit5 with ``K`` for the essential filters"""
    return ec.refit(p1, p2, mask, norm1, norm2) if K is None else es.refit5(p1, p2, mask, K)


# ------------------------------------------------------------------------------------------------------------ scenes
def two_views(n, n_out, sigma, seed, R, t, zoom=1.0, depth=(6.0, 30.0)):
    """epipolar_cases.scene with a motion of one's own: the same camera and 3-D point model (uniform in the first image, depths
    6 to 30), the second view rotated by R, translated by t and, with ``zoom``, at that multiple of the focal length
    -> (p1, p2, is_outlier)"""
    rng = np.random.default_rng(seed)
    K = np.array([[ec.FOCAL, 0.0, ec.WIDTH / 2.0], [0.0, ec.FOCAL, ec.HEIGHT / 2.0], [0.0, 0.0, 1.0]])
    K2 = K.copy()
    K2[0, 0] = K2[1, 1] = zoom * ec.FOCAL
    p1, p2 = np.empty((0, 2)), np.empty((0, 2))
    while len(p1) < n:
        m = 2 * n + 16
        uv = np.stack([rng.uniform(0.0, ec.WIDTH, m), rng.uniform(0.0, ec.HEIGHT, m), np.ones(m)], axis=1)
        X = (np.linalg.inv(K) @ uv.T).T * rng.uniform(depth[0], depth[1], m)[:, None]
        Y = (R @ X.T).T + t
        q = (K2 @ Y.T).T
        q = q[:, :2] / q[:, 2:3]
        ok = (Y[:, 2] > 0) & (q[:, 0] >= 0) & (q[:, 0] < ec.WIDTH) & (q[:, 1] >= 0) & (q[:, 1] < ec.HEIGHT)
        p1, p2 = np.vstack([p1, uv[ok, :2]]), np.vstack([p2, q[ok]])
    p1, p2 = p1[:n] + sigma * rng.standard_normal((n, 2)), p2[:n] + sigma * rng.standard_normal((n, 2))
    is_outlier = np.zeros(n, dtype=bool)
    if n_out:
        is_outlier[n - n_out:] = True
        p2[n - n_out:] = np.stack([rng.uniform(0.0, ec.WIDTH, n_out), rng.uniform(0.0, ec.HEIGHT, n_out)], axis=1)
    return np.ascontiguousarray(p1), np.ascontiguousarray(p2), is_outlier


def _roll(angle):
    return np.array([[math.cos(angle), -math.sin(angle), 0.0], [math.sin(angle), math.cos(angle), 0.0], [0.0, 0.0, 1.0]])


GENERAL = (500, 200, 0.5, 7)
MOTIONS = {          # name -> (R, t, zoom, sigma)
    "x translation": (np.eye(3), np.array([0.9, 0.0, 0.0]), 1.0, 0.0),       # the epipole at infinity, F with exact zeros
    "forward": (np.eye(3), np.array([0.0, 0.0, 1.5]), 1.0, 0.5),
    "roll 90": (_roll(math.pi / 2.0), np.array([0.9, 0.15, 0.3]), 1.0, 0.5),
    "zoom 2": (_roll(0.0), np.array([0.9, 0.15, 0.3]), 2.0, 0.5),
}


def scaled(p):
    return np.ascontiguousarray(p * np.array([5616.0 / ec.WIDTH, 3744.0 / ec.HEIGHT]))


def offset(p):
    return np.ascontiguousarray(p + np.array([1e5, -3e4]))


def integer(p):
    return np.ascontiguousarray(np.trunc(p))


COORDINATES = {"scaled": scaled, "offset": offset, "integer": integer}


def inlier_samples(n_in, H, seed):
    """H rows of 8 distinct indices below n_in"""
    return ec.draw_samples(n_in, H, seed)


# ------------------------------------------------------------------------------------------------------------ solve families
LADDER_SAMPLE_SEED, LADDER_K = 3, tuple(range(13))


def ladder_scene():
    """The general scene's 300 inliers and 14 more matches: match b of one sample moved to 10^-k px from match a of the same
    sample, in both images, for k = 0..12, and an exact repeat of a.  Row r of the samples is the sample with b replaced by
    the r-th of them -> (p1, p2, samples (14, 8))"""
    p1, p2, _, _ = ec.scene(*GENERAL)
    p1, p2 = p1[:300], p2[:300]
    base = inlier_samples(300, 1, LADDER_SAMPLE_SEED)[0]
    a, b = base[0], base[1]
    moved = []
    for p in (p1, p2):
        u = (p[b] - p[a]) / np.sqrt(((p[b] - p[a]) ** 2).sum())
        moved.append(np.array([p[a] + 10.0 ** -k * u for k in LADDER_K] + [p[a]]))
    samples = np.tile(base, (len(LADDER_K) + 1, 1))
    samples[:, 1] = 300 + np.arange(len(samples))
    return np.ascontiguousarray(np.vstack([p1, moved[0]])), np.ascontiguousarray(np.vstack([p2, moved[1]])), samples.astype(np.int32)


def solve_scenes():
    """Every solve family as scenes -> list of dict family, name, p1, p2, samples (H <= 64, 8): each goes through one
    alp_epipolar_solve8 call, and the device forms Hartley's normalisation from all points of the scene."""
    g1, g2, _, _ = ec.scene(*GENERAL)
    general = ec.draw_samples(500, 64, 1007)
    scenes = [dict(family="general", name="general", p1=g1, p2=g2, samples=general)]
    for k, (name, (R, t, zoom, sigma)) in enumerate(MOTIONS.items()):
        p1, p2, _ = two_views(200, 0, sigma, 11 + k, R, t, zoom)
        scenes.append(dict(family="motion " + name, name=name, p1=p1, p2=p2, samples=ec.draw_samples(200, 16, 21 + k)))
    for name, change in COORDINATES.items():
        scenes.append(dict(family=name, name=name, p1=change(g1), p2=change(g2), samples=general[:16]))
    l1, l2, rungs = ladder_scene()
    scenes.append(dict(family="ladder", name="ladder", p1=l1, p2=l2, samples=rungs))
    scenes.append(dict(family="outliers", name="outliers", p1=g1, p2=g2, samples=(300 + ec.draw_samples(200, 16, 31)).astype(np.int32)))
    # (no coverage family: tests/test_linalg_cases.py asserts that these already reach every free unknown, a swap at every step,
    # displaced swaps and each dropped column)
    return scenes


# ------------------------------------------------------------------------------------------------------------ refit families
# There is no entry point for the refit alone: a case is a whole-filter call with ONE given sample and refits = 1, built so that
# the refit is kept (the final F is then the refit) and so that no decision on the way hangs on rounding: no match within 1 %
# of the bound under the sample's F0 or under the refit.  The seeds below were chosen on the CPU restatement alone;
# tests/test_linalg_cases.py asserts the preconditions for every case.
PATH_MARGIN = 0.01
GENERAL_T = np.array([0.9, 0.15, 0.3])          # the motion of epipolar_cases.scene, with the rotation below


def _general_rotation():
    ay, ax = 0.08, 0.05
    Ry = np.array([[np.cos(ay), 0.0, np.sin(ay)], [0.0, 1.0, 0.0], [-np.sin(ay), 0.0, np.cos(ay)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(ax), -np.sin(ax)], [0.0, np.sin(ax), np.cos(ax)]])
    return Ry @ Rx


GENERAL_R = _general_rotation()


def sized_threshold(e, m):
    """The threshold that exactly m of the errors ``e`` meet: its square is the geometric middle of the m-th smallest error and
    the next one; None when those two lie within 2.1 % of each other (one would lie within 1 % of the bound)."""
    srt = np.sort(e)
    lo, hi = srt[m - 1], srt[m]
    if not (lo > 0.0 and hi > 1.021 * lo):
        return None
    return math.sqrt(math.sqrt(lo * hi))


def first_F0(case):
    """The restatement's hypotheses of the case's one sample: (1, 3, 3), or (10, 3, 3) for the essential filters"""
    if case["K"] is None:
        return ec.solve8_all(case["p1"], case["p2"], case["samples"])
    return es.solve5_all(case["p1"], case["p2"], case["samples"], case["K"], judge=False)[0].reshape(-1, 3, 3)


def norms_of(case):
    if case["K"] is None:
        return hartley_norms(case["p1"], case["p2"])
    return essential_norm(case["K"]), essential_norm(case["K"])


def restate(case, Fs=None):
    """The whole filter of the case on the CPU, refits = 1, from the hypotheses ``Fs`` (by default the restatement's own)
    -> dict chosen, F0, bound2 (of the inlier set the refit sums over), set (that inlier set), counts (refit_counts as the
    device reports them), kept, decided (no match within PATH_MARGIN of a bound that is used, and for LMedS the value
    decision by more than that), G (the restatement's refit)."""
    p1, p2, K = case["p1"], case["p2"], case["K"]
    Fs = first_F0(case) if Fs is None else np.asarray(Fs).reshape(-1, 3, 3)
    n1, n2 = norms_of(case)
    if case["kind"] == "ransac":
        t2 = case["threshold"] ** 2
        c = ec.counts(Fs, p1, p2, case["threshold"])
        k = ec.choose(c)
        inl = ec.inliers(Fs[k], p1, p2, case["threshold"])
        G = refit_numpy(p1, p2, inl, n1, n2, K)
        cg = int(ec.inliers(G, p1, p2, case["threshold"]).sum())
        decided = es.path_is_decided([Fs[k], G], p1, p2, case["threshold"])
        # another slot of a five-point sample must not reach the chosen one's count
        decided = decided and all(c[j] < c[k] - 2 for j in range(len(c)) if j != k)
        return {"chosen": k, "F0": Fs[k], "bound2": t2, "set": inl, "counts": [cg], "kept": cg > int(c[k]), "decided": decided, "G": G}
    m = 8 if K is None else 5
    out = lc.lmeds(p1, p2, Fs, m, case["quantile"], case["min_threshold"], refits=1, K=K)
    decided = lc.decisions_decided(out, p1, p2)[0]
    v = np.sort(out["values"])
    decided = decided and (len(v) == 1 or v[1] > (1.0 + PATH_MARGIN) * v[0])
    b2 = lc.bound2_of(out["path_values"][0], out["scale2"], out["floor2"])
    bg = lc.bound2_of(out["path_values"][1], out["scale2"], out["floor2"])
    cg = int((lc.errors_inf(out["path"][1], p1, p2) <= bg).sum())
    return {"chosen": out["chosen"], "F0": out["path"][0], "bound2": b2, "set": out["sets"][0], "counts": [cg],
            "kept": out["refits_kept"] == 1,
            "decided": decided, "G": out["path"][1], "rank": out["rank"], "scale2": out["scale2"], "floor2": out["floor2"]}


def _case(family, name, p1, p2, sample, kind="ransac", K=None, threshold=None, size=None, quantile=0.5, min_threshold=1.0, **require):
    """A refit case.  ``require``: what the case is there for, which tests/test_linalg_cases.py asserts of its exact reference on
    top of what every case must meet (the refit kept, every decision decided, kappa <= KAPPA_CAP, at most ``n`` = 1025 matches):
    set (the number of matches summed over), null (lambda1 / lambda9 at most this), gap ((lambda2 - lambda1) / lambda9 within this
    pair), s12 ((s1 - s2) / s1 of the eigenvector above this)."""
    case = dict(family=family, name=name, p1=p1, p2=p2, samples=np.asarray(sample, dtype=np.int32).reshape(1, -1), kind=kind, K=K,
                threshold=threshold, quantile=quantile, min_threshold=min_threshold, require=require)
    if size is not None:          # the threshold that gives the refit exactly ``size`` matches to sum over (a five-point sample: under
                                  # the slot below; the filter may then choose another slot and sum over a few more)
        Fs = first_F0(case)
        best = int(np.argmax(ec.counts(Fs, p1, p2, 3.0)))          # the slot that 3 px would choose
        case["threshold"] = sized_threshold(ec.errors(Fs[best], p1, p2), size)
    return case


def sizes_case(size, n, n_out, scene_seed, sample_seed):
    p1, p2, _, _ = ec.scene(n, n_out, 0.5, scene_seed)
    require = dict(set=size, n=max(n, 1025))
    if size == 8:
        require["null"] = 1e-25          # a sum of rank 8: lambda1 is zero
    return _case("refit sizes", f"{size} of {n}", p1, p2, inlier_samples(n - n_out, 1, sample_seed), size=size, **require)


def large_case(scene_seed, sample_seed, size=250, copies=140):
    """ec.scene(500, 100, 0.5) repeated 140 times and its first match once more: 70 001 matches, whose errors are those of the 500
    (70 001 distinct matches always hold one within 1 % of the threshold)"""
    q1, q2, _, _ = ec.scene(500, 100, 0.5, scene_seed)
    case = _case("refit large", "70 001", q1, q2, inlier_samples(400, 1, sample_seed), size=size, set=size * copies + 1, n=500 * copies + 1)
    idx = np.r_[np.tile(np.arange(500), copies), 0]
    case["p1"], case["p2"] = np.ascontiguousarray(q1[idx]), np.ascontiguousarray(q2[idx])
    return case


def worst_sample(p1, p2, n_in, draws, seed):
    """Of ``draws`` samples among the first n_in matches, the one whose 8 x 9 matrix has the smallest sigma8 / sigma1"""
    n1, n2 = hartley_norms(p1, p2)
    samples = inlier_samples(n_in, draws, seed)
    share = [np.linalg.svd(normalised_design(p1, p2, s, n1, n2), compute_uv=False) for s in samples]
    return samples[int(np.argmin([sv[7] / sv[0] for sv in share]))]


def noise_free_case(scene_seed, sample_seed, n=200, n_out=60):
    """Exact inliers and 30 % outliers.  An F0 from exact matches already holds every inlier, so a counting filter never keeps
    the refit; LMedS does, when the refit's median error is smaller, and its bound stays at the floor of 1 px.  F0 comes from
    the worst conditioned of 2000 samples, so that its errors are well above the refit's."""
    p1, p2, _, _ = ec.scene(n, n_out, 0.0, scene_seed)
    return _case("refit noise-free", "noise-free", p1, p2, worst_sample(p1, p2, n - n_out, 2000, sample_seed), kind="lmeds",
                 set=n - n_out, null=1e-25)


def coordinates_case(name, sample_seed, size=200):
    p1, p2, _, _ = ec.scene(*GENERAL)
    return _case("refit " + name, name, COORDINATES[name](p1), COORDINATES[name](p2), inlier_samples(300, 1, sample_seed), size=size)


def shallow_case(spread, scene_seed, sample_seed, sigma=0.1, size=150):
    p1, p2, _ = two_views(300, 90, sigma, scene_seed, GENERAL_R, GENERAL_T, depth=(12.0, 12.0 + spread))
    # the narrowest spread brings the gap to about 1e-6 lambda9, and no further
    require = dict(gap=(5e-7, 2e-6)) if spread <= 1.0 else {}
    sample = inlier_samples(210, 1, sample_seed)
    return _case("refit shallow", f"depths 12 to {12.0 + spread}", p1, p2, sample, size=size, set=size, **require)


def essential_case(short, scene_seed, sample_seed, size=150):
    """The general scene; or sigma = 2 and a tenth of the baseline, with a threshold that takes some thirty of the 90 random
    matches into the sum: the unconstrained eigenvector is then no essential matrix (s1 and s2 differ by more than 10 %)"""
    if short:
        p1, p2, _ = two_views(300, 90, 2.0, scene_seed, GENERAL_R, 0.1 * GENERAL_T)
    else:
        p1, p2, _, _ = ec.scene(300, 90, 0.5, scene_seed)
    sample = es.draw_samples5(210, 1, sample_seed)
    require = dict(s12=0.1) if short else {}
    return _case("refit essential", "short baseline" if short else "general", p1, p2, sample, K=es.K_TRUE, size=size, **require)


def lmeds_case(essential, scene_seed, sample_seed):
    p1, p2, _, _ = ec.scene(300, 90, 0.5, scene_seed)
    sample = es.draw_samples5(210, 1, sample_seed) if essential else inlier_samples(210, 1, sample_seed)
    name, K = ("essential", es.K_TRUE) if essential else ("fundamental", None)
    return _case("refit lmeds", name, p1, p2, sample, kind="lmeds", K=K)


def usable(case):
    """What the seeds below were searched for, on the restatement alone: each sample seed is the first from 1 upwards for which
    this holds together with the case's own ``require``"""
    if case["kind"] == "ransac" and case["threshold"] is None:
        return False
    cpu = restate(case)
    return bool(cpu["kept"] and cpu["decided"])


REFIT_CASES = (          # (builder, arguments): the seeds that the search on the restatement kept
    (sizes_case, (8, 64, 24, 3, 2)), (sizes_case, (9, 64, 24, 3, 7)), (sizes_case, (64, 257, 90, 3, 1)),
    (sizes_case, (257, 513, 150, 3, 23)), (sizes_case, (513, 1025, 525, 3, 2)),
    # 1025 matches to sum over and a refit that is kept need more than 1025 matches in all: 1000 inliers, 400 outliers
    (sizes_case, (1025, 1400, 400, 3, 2)),
    (noise_free_case, (1, 1)),
    (coordinates_case, ("scaled", 39)), (coordinates_case, ("offset", 39)), (coordinates_case, ("integer", 25)),
    (shallow_case, (4.0, 5, 4)), (shallow_case, (1.0, 5, 2)),
    (essential_case, (False, 2, 4)), (essential_case, (True, 4, 22, 240)),
    (lmeds_case, (False, 2, 2)), (lmeds_case, (True, 2, 1)),
)
LARGE_CASE = (large_case, (15, 1))


def refit_cases():
    return [make(*args) for make, args in REFIT_CASES]


def reference_of(case, inlier_set):
    """refit_exact of the case on ``inlier_set`` with the case's own normalisation -> (reference, kappa)"""
    n1, n2 = norms_of(case)
    ref = refit_exact(case["p1"], case["p2"], inlier_set, n1, n2, case["K"] is not None)
    return ref, kappa_refit(ref)


def route_distances(case, inlier_set, ref):
    """(d of numpy's route, d of the kernel's route) to the reference on ``inlier_set``"""
    n1, n2 = norms_of(case)
    a = refit_numpy(case["p1"], case["p2"], inlier_set, n1, n2, case["K"])
    b = refit_route(case["p1"], case["p2"], inlier_set, n1, n2, case["K"] is not None)
    return float(ec.sign_distance(a, ref["F"])[0]), float(ec.sign_distance(b, ref["F"])[0])


def swap_unchained(perm, k, j):
    """A planted error: right as long as the unknown in column j is unknown j, that is, on every sample but the displaced"""
    perm[k], perm[j] = j, perm[k]


def solve_references():
    """Every solve case, computed once per module (some 220 mpmath solves: seconds) -> list of dict family, scene, row, p1, p2,
    sample, norms, ref (solve8_exact), kappa, share (sigma8 / sigma1), numpy (ec.solve8's F), route and info (solve8_route's)"""
    out = []
    for sc in solve_scenes():
        n1, n2 = hartley_norms(sc["p1"], sc["p2"])
        for row, sample in enumerate(sc["samples"]):
            ref = solve8_exact(sc["p1"], sc["p2"], sample, n1, n2)
            route, info = solve8_route(sc["p1"], sc["p2"], sample, n1, n2)
            out.append(dict(family=sc["family"], scene=sc["name"], row=row, p1=sc["p1"], p2=sc["p2"], sample=sample, norms=(n1, n2),
                            ref=ref, kappa=kappa_solve(ref), share=float(ref["sigma"][7] / ref["sigma"][0]),
                            numpy=ec.solve8(sc["p1"], sc["p2"], sample, n1, n2), route=route, info=info))
    return out


def refit_references(large=False):
    """Every refit case (or the one of 70 001 matches) on the restatement's own F0 -> list of dict case, cpu (restate), ref, kappa"""
    out = []
    for case in ([LARGE_CASE[0](*LARGE_CASE[1])] if large else refit_cases()):
        cpu = restate(case)
        ref, kappa = reference_of(case, cpu["set"])
        out.append(dict(case=case, cpu=cpu, ref=ref, kappa=kappa))
    return out


# ------------------------------------------------------------------------------------------------------------ the whole filters' final F
def last_kept_fit(p1, p2, F, threshold, refits, refit):
    """The counting filter's refit loop from the chosen ``F`` (``refit``: inlier set -> candidate) -> (the inlier set that the
    final F was fitted to, or None when no refit was kept; the final F)"""
    count, fitted_to = int(ec.inliers(F, p1, p2, threshold).sum()), None
    for _ in range(refits):
        inl = ec.inliers(F, p1, p2, threshold)
        G = refit(inl)
        cg = int(ec.inliers(G, p1, p2, threshold).sum())
        if cg <= count:
            break
        F, count, fitted_to = G, cg, inl
    return fitted_to, F


def whole_filter_reference(p1, p2, samples, want, threshold, K=None, refits=4):
    """What the final F of ec.ransac / es.ransac5 (``want``) is held to -> (reference, kappa, family), or None: refit_exact on the
    set its last kept refit summed over; without a kept refit the 8-point solve of the chosen sample; the five-point solver's
    own matrices are held elsewhere (essential_cases.DEVICE_TOL)."""
    if K is None:
        n1, n2 = hartley_norms(p1, p2)
        F0 = ec.solve8(p1, p2, samples[want["chosen"]], n1, n2)
        refit = lambda inl: ec.refit(p1, p2, inl, n1, n2)  # noqa: E731
    else:
        n1 = n2 = essential_norm(K)
        F0 = want["path"][0]
        refit = lambda inl: es.refit5(p1, p2, inl, K)  # noqa: E731
    fitted_to, F = last_kept_fit(p1, p2, F0, threshold, refits, refit)
    assert np.array_equal(F, want["F"], equal_nan=True)
    if fitted_to is not None:
        ref = refit_exact(p1, p2, fitted_to, n1, n2, K is not None)
        return ref, kappa_refit(ref), "refit essential" if K is not None else "refit sizes"
    if K is not None:
        return None
    ref = solve8_exact(p1, p2, samples[want["chosen"]], n1, n2)
    return ref, kappa_solve(ref), "general"
