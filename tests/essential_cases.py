"""The numpy restatement of the essential-matrix match filter (alp_epipolar_samples5 / _solve5 / alp_essential_ransac in
alproj_amd/csrc/alp_epipolar.hip) and the scenes its tests use.  Not a test module: tests/test_essential_cases.py holds it to the
constraints, to the truth and to an independent root count on the CPU, tests/test_gpu_essential.py holds the device to it.

The formulation is Nister's five-point solver with Stewenius' Gauss-Jordan step, as in the kernel.  What the restatement shares
with the kernel, operation for operation, is the null-space basis of the sample's 5 x 9 matrix (``null_basis``: elimination with
complete pivoting needs only + - * /, so numpy repeats it bit for bit): the unknowns (x, y, z) of E = x N0 + y N1 + z N2 + N3,
and with them the ascending order of the roots z, mean something only with respect to that basis.  Everything after it goes
another way: the ten cubics by convolution of coefficient tensors, the 10 x 10 part by numpy.linalg.solve, the roots as the
eigenvalues of the companion matrix, the essential projection by numpy.linalg.svd and the refit by numpy.linalg.eigh.

F is the pixel-space matrix K^-T E K^-1 at unit Frobenius norm, with b^T F a = 0 for a = (x1, y1, 1), b = (x2, y2, 1); K is
(f, cx, cy), one for both images."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epipolar_cases as ec  # noqa: E402
from epipolar_cases import FOCAL, HEIGHT, WIDTH, choose, counts, errors, inliers, scene, sign_distance  # noqa: E402,F401

K_TRUE = (FOCAL, WIDTH / 2.0, HEIGHT / 2.0)
RANK_TOL = 1e-13          # the kernel's: a pivot below this share of the first one, and the sample's matrix has rank below 5
IMAG_TOL = 1e-8           # a companion eigenvalue is a real root when |imag| <= IMAG_TOL * max(1, |real|)

# A sample may be left out of the device comparison when two roots of its polynomial lie closer than ROOT_DELTA (relative to
# max(1, |z|)), or when a real root has |p'(z)| below SLOPE_FLOOR * sum |a_k z^k|: there the number of real roots is decided by
# rounding.  "Two roots" are counted in the complex plane: a conjugate pair with |imag| <= ROOT_DELTA is two roots 2 |imag|
# apart that rounding may bring onto the real axis, so it counts like two real roots that close.  Nothing else excuses a sample.
ROOT_DELTA = 1e-5
SLOPE_FLOOR = 1e-8
POLISH_TOL = 5e-14       # the kernel's SOLVE5_POLISH_TOL

# The tolerance of the device comparison, ||F_dev - F_ref|| up to sign.  Measured on the CPU (test_essential_cases.py prints and
# asserts it): on the noise-free scene(200, 0, 0.0, 1) with draw_samples5(200, 257, 5), the restatement's solution nearest the
# truth lies 1.2e-14 from it at the worst over all 257 samples (1.154e-14; 3.6e-14 and 1.7e-14 on the scene seeds 2 and 3).  The
# device gets 100 times the measured figure, 1.2e-12: another elimination order in the 10 x 10 part, bisection in place of the
# eigenvalues, and its own Gauss-Newton steps.
SELF_DISTANCE = 1.2e-14
DEVICE_TOL = 100 * SELF_DISTANCE

# (n, n_out, threshold, scene seed, planar) of the whole-filter tests, sigma = 0.5, 1024 samples from draw_samples5(n, 1024,
# 1000 + seed).  The seeds are chosen on the restatement alone, as epipolar_cases.RANSAC_SCENES was, so that the truth checks can
# be strict: every true inlier kept, at most 2 outliers kept and each of those within threshold of the TRUE lines, no match
# within 1 % of threshold^2 under the final F (none within 5 % when the seeds were chosen).  Of the seeds 1..30 these hold for 4
# at (400, 280), for 15 at (64, 24), for 12 of 15 at (9, 1).  (400, 280): the low inlier share, w = 0.3, where 1024 five-point
# samples hold an all-inlier one with probability 0.92 and 1024 eight-point samples with 0.07; seed 5 is also one whose refit is
# kept twice (92 -> 118 -> 120).  The planar scene has few outliers: an essential matrix fitted to noisy points of one plane
# has an uncertain epipole, and of (200, 80) it keeps 1 to 4 outliers that lie within threshold of ITS lines but 4 to 10 pixels
# from the true ones, for every seed tried; with 10 outliers, seed 6 of 1..15 keeps none.  (9, 1): 8 inliers are the fewest on
# which the refit's 9 x 9 matrix has one null vector, so that two eigenvalue routines give one candidate.
RANSAC5_SCENES = ((400, 280, 3.0, 5, False), (64, 24, 3.0, 7, False), (110, 10, 3.0, 6, True), (9, 1, 3.0, 1, False))
RANSAC5_SAMPLES = 1024

# monomials of the cubics as exponents of (x, y, z), in the kernel's column order: the first ten are eliminated
MONOMIALS = ((3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
             (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0))


def normalise(p, K):
    """x' = (x - cx) * (1 / f): the kernel multiplies by the reciprocal, formed once."""
    f, cx, cy = K
    return (p - np.array([cx, cy])) * (1.0 / f)


def _design(a, b):
    return np.stack([b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0], b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1],
                     a[:, 0], a[:, 1], np.ones(len(a))], axis=1)


def null_basis(A):
    """(4, 9): the null space of a 5 x 9 matrix as the kernel forms it, or None when its rank is below 5.  Gaussian elimination
    with complete pivoting (the first largest entry in row-major order), then for each of the four free columns the vector with
    1 there and 0 at the other three, by back substitution with the sum taken from the left."""
    A = np.array(A, dtype=np.float64)
    perm = list(range(9))
    first = 0.0
    for k in range(5):
        sub = np.abs(A[k:, k:])
        pi, pj = np.unravel_index(int(np.argmax(sub)), sub.shape)
        pv = sub[pi, pj]
        pi, pj = pi + k, pj + k
        if k == 0:
            first = pv
        if not (pv > first * RANK_TOL) or not np.isfinite(pv):
            return None
        if pi != k:
            A[[k, pi], k:] = A[[pi, k], k:]
        if pj != k:
            A[:, [k, pj]] = A[:, [pj, k]]
            perm[k], perm[pj] = perm[pj], perm[k]
        for i in range(k + 1, 5):
            mlt = A[i, k] / A[k, k]
            A[i, k + 1:] = A[i, k + 1:] - mlt * A[k, k + 1:]
    N = np.zeros((4, 9))
    for c in range(4):
        Y = np.zeros(9)
        Y[5 + c] = 1.0
        for k in range(4, -1, -1):
            s = 0.0
            for j in range(k + 1, 9):
                s += A[k, j] * Y[j]
            Y[k] = -s / A[k, k]
        N[c, perm] = Y
    return N


def _pmul(a, b):
    """The product of two polynomials in (x, y, z) held as (..., 4, 4, 4) coefficient tensors; the degrees add up to 3 at most."""
    out = np.zeros(np.broadcast_shapes(a.shape, b.shape))
    for i in range(4):
        for j in range(4 - i):
            for k in range(4 - i - j):
                out[..., i:, j:, k:] += a[..., i, j, k, None, None, None] * b[..., :4 - i, :4 - j, :4 - k]
    return out


def cubics(N):
    """(..., 10, 20): det E = 0 and the nine entries of 2 E E^T E - tr(E E^T) E = 0 for E = x N[0] + y N[1] + z N[2] + N[3], in
    MONOMIALS; N is (..., 4, 9), any number of samples at once."""
    N = np.asarray(N)
    E = np.zeros((3, 3) + N.shape[:-2] + (4, 4, 4))
    for r in range(3):
        for c in range(3):
            for k, at in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))):
                E[(r, c, Ellipsis) + at] = N[..., k, 3 * r + c]
    det = (_pmul(_pmul(E[0, 1], E[1, 2]) - _pmul(E[0, 2], E[1, 1]), E[2, 0])
           + _pmul(_pmul(E[0, 2], E[1, 0]) - _pmul(E[0, 0], E[1, 2]), E[2, 1])
           + _pmul(_pmul(E[0, 0], E[1, 1]) - _pmul(E[0, 1], E[1, 0]), E[2, 2]))
    EEt = [[sum(_pmul(E[i, k], E[j, k]) for k in range(3)) for j in range(3)] for i in range(3)]
    trace = EEt[0][0] + EEt[1][1] + EEt[2][2]
    rows = [det]
    for i in range(3):
        for j in range(3):
            rows.append(2.0 * sum(_pmul(EEt[i][k], E[k, j]) for k in range(3)) - _pmul(trace, E[i, j]))
    return np.stack([np.stack([row[(Ellipsis,) + m] for m in MONOMIALS], axis=-1) for row in rows], axis=-2)


def _polymul(a, b):
    return np.convolve(a, b)


def z_polynomial(M):
    """-> (B, p): after the first ten columns of the cubics are eliminated, the rows of x^2 z, x^2, y^2 z, y^2, x y z and x y give
    three equations B(z) (x, y, 1)^T = 0 with entries of degree 3, 3, 4 in z (highest power first), and p = det B, degree 10.
    None when the 10 x 10 part is singular."""
    lead = M[:, :10]
    if not np.isfinite(M).all() or np.linalg.cond(lead) > 1e14:
        return None
    return _z_polynomial(np.linalg.solve(lead, M[:, 10:]))


def _z_polynomial(T):
    B = []
    for hi, lo in ((4, 5), (6, 7), (8, 9)):          # row(hi) - z * row(lo)
        e, f = T[hi], T[lo]
        B.append([np.array([-f[0], e[0] - f[1], e[1] - f[2], e[2]]), np.array([-f[3], e[3] - f[4], e[4] - f[5], e[5]]),
                  np.array([-f[6], e[6] - f[7], e[7] - f[8], e[8] - f[9], e[9]])])
    p = (_polymul(_polymul(B[0][0], B[1][1]) - _polymul(B[0][1], B[1][0]), B[2][2])
         + _polymul(_polymul(B[0][1], B[1][2]) - _polymul(B[0][2], B[1][1]), B[2][0])
         + _polymul(_polymul(B[0][2], B[1][0]) - _polymul(B[0][0], B[1][2]), B[2][1]))
    return B, p


def real_roots(p):
    """(roots ascending, all companion eigenvalues): the real roots of p (highest power first) by numpy.linalg.eigvals, each
    polished by two Newton steps."""
    companion = np.diag(np.ones(len(p) - 2), -1)
    companion[0] = -p[1:] / p[0]
    ev = np.linalg.eigvals(companion)
    z = np.sort(ev.real[np.abs(ev.imag) <= IMAG_TOL * np.maximum(1.0, np.abs(ev.real))])
    dp = np.polyder(p)
    for _ in range(2):
        z = z - np.polyval(p, z) / np.polyval(dp, z)
    return np.sort(z), ev


def ill_conditioned(p, z, ev):
    """True when the number of real roots of p hangs on rounding (ROOT_DELTA, SLOPE_FLOOR above)."""
    near_real = ev[np.abs(ev.imag) <= ROOT_DELTA * np.maximum(1.0, np.abs(ev.real))]
    if len(near_real) != len(z):
        return True
    re = np.sort(near_real.real)
    if len(re) > 1 and (np.diff(re) <= ROOT_DELTA * np.maximum(1.0, np.abs(re[1:]))).any():
        return True
    if len(z):
        size = np.array([np.abs(p * zz ** np.arange(len(p) - 1, -1, -1)).sum() for zz in z])
        if (np.abs(np.polyval(np.polyder(p), z)) * np.maximum(1.0, np.abs(z)) <= SLOPE_FLOOR * size).any():
            return True
    return False


def polish(M, u, steps=3):
    """Gauss-Newton steps on the ten cubics M (before their elimination) at the rows (x, y, z) of ``u``; a step that does not
    shrink a row's residual ends that row's steps.  The kernel takes the same steps with the cubics evaluated on the entries
    of E."""
    ex = np.array(MONOMIALS, dtype=np.float64)
    u = np.array(u, dtype=np.float64)
    live = np.ones(len(u), dtype=bool)

    def residual(u):
        return np.prod(u[:, None, :] ** ex, axis=2) @ M.T

    g = residual(u)
    for _ in range(steps):
        J = np.empty((len(u), 10, 3))
        for k in range(3):
            lower = ex.copy()
            lower[:, k] = np.maximum(lower[:, k] - 1.0, 0.0)
            J[:, :, k] = (ex[:, k] * np.prod(u[:, None, :] ** lower, axis=2)) @ M.T
        with np.errstate(all="ignore"):
            w = u - (np.linalg.pinv(J) @ g[:, :, None])[:, :, 0]
            g2 = residual(w)
            live &= (g2 * g2).sum(axis=1) < (g * g).sum(axis=1)
        u[live], g[live] = w[live], g2[live]
    return u, g


def denormalise(E, K):
    """K^-T E K^-1 at unit Frobenius norm (NaN when that is not finite): E K^-1 first, then K^-T times it."""
    f, cx, cy = K
    s = 1.0 / f
    a = np.stack([s * E[:, 0], s * E[:, 1], E[:, 2] - s * (cx * E[:, 0] + cy * E[:, 1])], axis=1)
    F = np.stack([s * a[0], s * a[1], a[2] - s * (cx * a[0] + cy * a[1])])
    fro = np.sqrt((F * F).sum())
    if not (np.isfinite(fro) and fro > 0.0):
        return np.full((3, 3), np.nan)
    return F / fro


def solve5_details(p1, p2, samples, K, judge=True):
    """One dict per sample: F (nsol, 3, 3), E (nsol, 3, 3) at unit norm, z (nsol,) ascending: the roots whose solution the
    Gauss-Newton steps brought onto the cubics (POLISH_TOL), roots: all real roots, p (11,) or None, skip (bool:
    ill_conditioned, when ``judge``).  The cubics and the 10 x 10 solve run over all samples at once."""
    out = [{"F": np.zeros((0, 3, 3)), "E": np.zeros((0, 3, 3)), "z": np.zeros(0), "roots": np.zeros(0), "p": None, "skip": False} for _ in samples]
    a, b = normalise(p1, K), normalise(p2, K)
    bases = [null_basis(_design(a[s], b[s])) for s in samples]
    good = [h for h, N in enumerate(bases) if N is not None]
    if not good:
        return out
    M = cubics(np.stack([bases[h] for h in good]))
    with np.errstate(all="ignore"):
        fine = np.isfinite(M).all(axis=(1, 2))
        fine[fine] = np.linalg.cond(M[fine, :, :10]) <= 1e14
    T = np.zeros((len(good), 10, 10))
    T[fine] = np.linalg.solve(M[fine, :, :10], M[fine, :, 10:])
    for h, t, ok, m in zip(good, T, fine, M):
        if not ok:
            continue
        N = bases[h]
        B, p = _z_polynomial(t)
        if not np.isfinite(p).all() or p[0] == 0.0:
            continue
        z, ev = real_roots(p)
        if len(z) == 0:
            out[h]["p"], out[h]["roots"], out[h]["skip"] = p, z, bool(judge and ill_conditioned(p, z, ev))
            continue
        rows = np.array([[np.polyval(B[r][c], z) for c in range(3)] for r in range(3)])          # (3, 3, roots)
        cross = np.stack([np.cross(rows[i].T, rows[j].T) for i, j in ((0, 1), (0, 2), (1, 2))])      # (3, roots, 3)
        v = cross[np.argmax(np.abs(cross[:, :, 2]), axis=0), np.arange(len(z))]
        with np.errstate(all="ignore"):
            u, g = polish(m, np.stack([v[:, 0] / v[:, 2], v[:, 1] / v[:, 2], z], axis=1))
            Es = (u[:, :1] * N[0] + u[:, 1:2] * N[1] + u[:, 2:] * N[2] + N[3]).reshape(-1, 3, 3)
            # a solution that the steps did not bring onto the cubics is none: the residual of E at unit norm, as the kernel forms it
            kept = (g * g).sum(axis=1) <= POLISH_TOL ** 2 * (Es * Es).sum(axis=(1, 2)) ** 3
        Es = Es[kept]
        Fs = np.array([denormalise(E, K) for E in Es]).reshape(-1, 3, 3)
        if not np.isfinite(Fs).all():
            continue
        out[h] = {"F": Fs, "E": Es / np.sqrt((Es * Es).sum(axis=(1, 2)))[:, None, None], "z": z[kept], "roots": z, "p": p,
                  "skip": bool(judge and ill_conditioned(p, z, ev))}
    return out


def solve5(p1, p2, sample, K):
    """The pixel-space matrices of one sample of five matches, (nsol, 3, 3) with nsol <= 10, in ascending order of the root."""
    return solve5_details(p1, p2, [np.asarray(sample)], K)[0]["F"]


def solve5_all(p1, p2, samples, K, judge=True):
    """-> (F (H, 10, 3, 3) with NaN in the unused slots, nsol (H,), skip (H,) bool) as alp_epipolar_solve5 lays them out"""
    F = np.full((len(samples), 10, 3, 3), np.nan)
    nsol = np.zeros(len(samples), dtype=np.int32)
    skip = np.zeros(len(samples), dtype=bool)
    for h, d in enumerate(solve5_details(p1, p2, samples, K, judge)):
        nsol[h], skip[h] = len(d["F"]), d["skip"]
        F[h, :nsol[h]] = d["F"]
    return F, nsol, skip


def to_essential(F, K):
    """K^T F K"""
    f, cx, cy = K
    Km = np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])
    return Km.T @ np.asarray(F).reshape(3, 3) @ Km


def project_essential(E):
    """The nearest essential matrix in Frobenius norm: singular values (s, s, 0), s = (s1 + s2) / 2."""
    U, S, Vt = np.linalg.svd(E)
    s = (S[0] + S[1]) / 2.0
    return U @ np.diag([s, s, 0.0]) @ Vt


def essential_residuals(E):
    """(|det E|, the largest |entry| of 2 E E^T E - tr(E E^T) E) of E scaled to unit Frobenius norm"""
    E = np.asarray(E).reshape(3, 3)
    E = E / np.sqrt((E * E).sum())
    return abs(np.linalg.det(E)), np.abs(2.0 * E @ E.T @ E - np.trace(E @ E.T) * E).max()


def refit5(p1, p2, mask, K):
    """The 8-point solution on all matches of ``mask`` in K-normalised coordinates (the eigenvector of the smallest eigenvalue of
    the 9 x 9 sum: that matrix is K^T F K of the pixel-space fit), projected onto the essential matrices, back in pixels."""
    A = _design(normalise(p1[mask], K), normalise(p2[mask], K))
    _, V = np.linalg.eigh(A.T @ A)
    return denormalise(project_essential(V[:, 0].reshape(3, 3)), K)


def ransac5(p1, p2, samples, K, threshold, refits=4, Fs=None):
    """The whole filter on a given (H, 5) sample list -> dict F, mask, chosen (h * 10 + slot), chosen_count, final_count,
    refit_counts, refits_kept, keep_all, path (the chosen matrix and every refit candidate): epipolar_cases.ransac with ten slots per sample, the essential refit and 5 for 8."""
    Fs = solve5_all(p1, p2, samples, K, judge=False)[0] if Fs is None else Fs
    Fs = Fs.reshape(-1, 3, 3)
    c = counts(Fs, p1, p2, threshold)
    k = choose(c)
    F, count = Fs[k], int(c[k])
    out = {"chosen": k, "chosen_count": count, "refit_counts": [], "refits_kept": 0, "keep_all": count < 5, "path": [F]}
    if count >= 5:
        for _ in range(refits):
            G = refit5(p1, p2, inliers(F, p1, p2, threshold), K)
            out["path"].append(G)
            cg = int(inliers(G, p1, p2, threshold).sum())
            out["refit_counts"].append(cg)
            if cg <= count:
                break
            F, count = G, cg
            out["refits_kept"] += 1
    out["F"], out["final_count"] = F, count
    out["mask"] = np.ones(len(p1), dtype=bool) if out["keep_all"] else inliers(F, p1, p2, threshold)
    return out


SLOT_MARGIN, PATH_MARGIN = 1e-4, 0.01


def choice_is_decided(Fs, p1, p2, threshold):
    """True when two numerical routes to the slots ``Fs`` must choose the same one with the same count: no match of the chosen
    slot lies within SLOT_MARGIN of threshold^2 (relative), and no other slot could reach its count, or pass it, if all its
    matches that close to the threshold fell the other way.  SLOT_MARGIN: a slot within DEVICE_TOL of the restatement's moves
    s = b^T F a, with coordinates up to 1.5e3, by some 1e-6 of a 3-pixel error; 1e-4 is a hundred times that."""
    t2 = threshold * threshold
    with np.errstate(invalid="ignore"):
        e = np.array([errors(F, p1, p2) for F in np.asarray(Fs).reshape(-1, 3, 3)])
        c = (e <= t2).sum(axis=1)
        m = (np.abs(e - t2) <= SLOT_MARGIN * t2).sum(axis=1)
    k = choose(c)
    return bool(m[k] == 0 and (c[:k] + m[:k] < c[k]).all() and (c[k + 1:] + m[k + 1:] <= c[k]).all())


def path_is_decided(path, p1, p2, threshold):
    """True when no match lies within PATH_MARGIN (1 %) of threshold^2 under the chosen matrix or any refit candidate."""
    t2 = threshold * threshold
    with np.errstate(invalid="ignore"):
        return not any((np.abs(errors(F, p1, p2) - t2) <= PATH_MARGIN * t2).any() for F in path if np.isfinite(F).all())


# (scene seed, sample seed) of tests/test_gpu_essential.py::test_ransac5_launch_seams for n = 5, 6, 64, 513: scene(n, n // 3, 0.5,
# scene seed) and draw_samples5(n, 257, sample seed), chosen on the restatement alone so that choice_is_decided holds at H = 1, 26
# and 257 and path_is_decided at refits 0 and 4 (tests/test_essential_cases.py asserts it)
SEAM_SEEDS = {5: (1, 1), 6: (1, 1), 64: (1, 1), 513: (1, 1)}
SEAM_H = (1, 26, 257)


def seam_case(n):
    """-> (p1, p2, samples (257, 5), Fs (257, 10, 3, 3)) of a launch-seam size"""
    scene_seed, sample_seed = SEAM_SEEDS[n]
    p1, p2, _, _ = scene(n, n // 3, 0.5, scene_seed)
    samples = draw_samples5(n, 257, sample_seed)
    return p1, p2, samples, solve5_all(p1, p2, samples, K_TRUE, judge=False)[0]


def count_real_roots(p):
    """The number of real roots of p (highest power first) counted another way: p is monotone between two neighbouring real
    roots of p', so it has one root wherever its sign changes from one of them (or from the Cauchy bound) to the next."""
    p = np.asarray(p, dtype=np.float64)
    bound = 1.0 + np.abs(p[1:] / p[0]).max()
    crit = np.roots(np.polyder(p))
    crit = np.sort(crit.real[np.abs(crit.imag) <= IMAG_TOL * np.maximum(1.0, np.abs(crit.real))])
    signs = np.sign(np.polyval(p, np.r_[-bound, crit, bound]))
    signs = signs[signs != 0]
    return int((signs[1:] != signs[:-1]).sum())


def scene_planar(n, n_out, sigma, seed):
    """epipolar_cases.scene with every 3-D point on the plane 0.25 X - 0.15 Y + Z = 14 (depths from about 9 to 22): the same
    cameras, the same noise and outliers -> (p1, p2, F_true, is_outlier)."""
    rng = np.random.default_rng(seed)
    K = np.array([[FOCAL, 0.0, WIDTH / 2.0], [0.0, FOCAL, HEIGHT / 2.0], [0.0, 0.0, 1.0]])
    ay, ax = 0.08, 0.05
    Ry = np.array([[np.cos(ay), 0.0, np.sin(ay)], [0.0, 1.0, 0.0], [-np.sin(ay), 0.0, np.cos(ay)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(ax), -np.sin(ax)], [0.0, np.sin(ax), np.cos(ax)]])
    R, t = Ry @ Rx, np.array([0.9, 0.15, 0.3])
    normal, offset = np.array([0.25, -0.15, 1.0]), 14.0
    p1 = np.empty((0, 2))
    p2 = np.empty((0, 2))
    while len(p1) < n:
        m = 2 * n + 16
        uv = np.stack([rng.uniform(0.0, WIDTH, m), rng.uniform(0.0, HEIGHT, m), np.ones(m)], axis=1)
        ray = (np.linalg.inv(K) @ uv.T).T
        X = ray * (offset / (ray @ normal))[:, None]
        Y = (R @ X.T).T + t
        q = (K @ Y.T).T
        q = q[:, :2] / q[:, 2:3]
        ok = (Y[:, 2] > 0) & (q[:, 0] >= 0) & (q[:, 0] < WIDTH) & (q[:, 1] >= 0) & (q[:, 1] < HEIGHT)
        p1, p2 = np.vstack([p1, uv[ok, :2]]), np.vstack([p2, q[ok]])
    p1, p2 = p1[:n].copy(), p2[:n].copy()
    p1 += sigma * rng.standard_normal((n, 2))
    p2 += sigma * rng.standard_normal((n, 2))
    is_outlier = np.zeros(n, dtype=bool)
    if n_out:
        is_outlier[n - n_out:] = True
        p2[n - n_out:] = np.stack([rng.uniform(0.0, WIDTH, n_out), rng.uniform(0.0, HEIGHT, n_out)], axis=1)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    F = np.linalg.inv(K).T @ tx @ R @ np.linalg.inv(K)
    return np.ascontiguousarray(p1), np.ascontiguousarray(p2), F / np.sqrt((F * F).sum()), is_outlier


def make_scene(n, n_out, sigma, seed, planar=False):
    return (scene_planar if planar else scene)(n, n_out, sigma, seed)


EPI_STREAM, EPI_STREAM5 = 0x45504950, 0x45504935          # the third counter word of the 8-wide and of the 5-wide rows


def device_samples(n, H, seed, width):
    """What alp_epipolar_samples (width 8) and alp_epipolar_samples5 (width 5) draw: for hypothesis h the Philox blocks of the
    counters (attempt, h, stream, 0) under the key (seed low, seed high), attempt = 0, 1, ...; each of a block's four words w
    offers the index (w * n) >> 32, and an index the row already holds is passed over."""
    import cma_cases as cc
    k0, k1 = cc.key_of(seed)
    stream = np.uint64(EPI_STREAM if width == 8 else EPI_STREAM5)
    rows = np.empty((H, width), dtype=np.int32)
    attempts = np.arange(64, dtype=np.uint64)
    for h in range(H):
        w = np.stack(cc.philox4x32_10(attempts, np.uint64(h), stream, np.uint64(0), k0, k1), axis=1).ravel()
        row = []
        for c in (w * np.uint64(n)) >> np.uint64(32):
            if int(c) not in row:
                row.append(int(c))
                if len(row) == width:
                    break
        assert len(row) == width, "more than 64 blocks for one row: not in these tests"
        rows[h] = row
    return rows


def draw_samples5(n, H, seed):
    """H rows of 5 distinct indices, numpy's own draw (the tests that compare on the same samples)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(n, 5, replace=False) for _ in range(H)]).astype(np.int32)
