"""Seeded inputs shared by tests/test_gpu_popeval_grid.py and tests/test_gpu_points.py: the point sets, observations and candidate
populations of the population kernel's launch-grid tests, their float64 oracle losses, and the construction of a candidate that
sits exactly on a pole of one lens denominator."""
import numpy as np

from alproj_amd import synthetic as syn
from oracle import ref_numpy as orc

# a ragged point set of 67 rows of 256 points (the last one 37 short)
N_ROWS = 67
N = N_ROWS * 256 - 37
# forced stripe counts: rows_per = ceil(67 / stripes) = 67, 34, 23, 17, 14, 12, 10, 8, 7, 6, 5, 4, 3, 2, 1 and 1 (1000 is clamped
# to the 67 rows) -- every remainder of rows_per modulo any group width up to 9, so the sweep stays meaningful if the widths are
# retuned.  30 and 60 stripes: rows_per 3 and 2 with 7 and 26 EMPTY trailing stripes.
STRIPES = (1, 2, 3, 4, 5, 6, 7, 9, 10, 12, 14, 17, 23, 34, 67, 1000)
EMPTY_STRIPES = (30, 60)
TC = 128                              # candidates per tile (POP_TC, POP_TCD)
# rows of one unmasked group of pop_walk_stripe (alproj_amd/csrc/alp_point_kernels.h: POP_V, POP_VD, POP_V_LF, POP_VD_LF); the
# tests only use them to place marked points on group boundaries
GROUP_ROWS = {("general", "f32"): 6, ("shared_pose", "f32"): 6, ("lens_free", "f32"): 8,
              ("general", "f64"): 5, ("shared_pose", "f64"): 5, ("lens_free", "f64"): 6}
VARIANTS = ("general", "shared_pose", "lens_free")
LENS_KEYS = ("k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2", "s1", "s2", "s3", "s4")
LOSSES = {"mean_dist": (orc.LOSS_MEAN_DIST, 0.0), "huber": (orc.LOSS_HUBER, 10.0)}


def rows_per(stripes, rows=N_ROWS):
    s = min(stripes, rows)
    return -(-rows // s)


def stripe_bounds(stripes, n=N):
    """[beg, end) of every non-empty stripe, as popeval_kernel cuts them"""
    rows = -(-n // 256)
    rp = rows_per(stripes, rows)
    out = []
    for b in range(min(stripes, rows)):
        beg = b * rp * 256
        if beg < n:
            out.append((beg, min(beg + rp * 256, n)))
    return out


def mark_positions(stripes, V, n=N):
    """points on the boundaries the grid creates: first and last point of every stripe, lanes 0 and 255 of the last row of every
    V-group, the first and the last point of every 2-wide group, n - 256 and n - 1 (walked as pop_walk_stripe walks)"""
    idx = {n - 1, n - 256}
    for beg, end in stripe_bounds(stripes, n):
        idx |= {beg, end - 1}
        base = beg
        while base + 256 * V <= end:
            idx |= {base + 256 * (V - 1), base + 256 * V - 1}
            base += 256 * V
        while base + 512 <= end:
            idx |= {base, base + 511}
            base += 512
    return sorted(idx)


def mark_counts(total, n_marks, unit=1.0):
    """how often each of n_marks marked points was counted in a mean-distance sum `total` (loss * n) whose marks are off by
    unit * 4^k pixels and every other point by (almost) nothing: the base-4 digits of total / unit, or None when that is not
    within 0.25 of an integer below 4^n_marks"""
    q = total / unit
    code = int(round(q))
    if not (abs(q - code) < 0.25 and 0 <= code < 4 ** n_marks):
        return None
    return [(code >> (2 * k)) & 3 for k in range(n_marks)]


def truth(variant):
    """the pose that produced the observations: a lens for the general and shared-pose variants, k = p = s = 0 (a1, a2 kept)
    for the lens-free one"""
    t = syn.truth_params(316)
    if variant == "lens_free":
        t.update({k: 0.0 for k in LENS_KEYS})
    return t


def origin():
    t = syn.truth_params(316)
    return np.array([t["x"], t["y"], t["z"]])


def point_set(n=N, seed=67):
    """well-conditioned GCP-like points and their observations (the truth with a lens, 1 px noise)"""
    t = truth("general")
    xyz = syn.gcp_points(n, t, seed=seed)
    uv = orc.project_points(xyz, t) + np.random.default_rng(seed).normal(0, 1.0, (n, 2))
    return xyz, uv


def population(variant, P, seed=5):
    """P candidates (25-vectors) of one variant: general = D21 around the truth, shared_pose = only a1..s4 move, lens_free = D9
    around the truth without a lens"""
    from alproj_amd import _lib as L
    rng = np.random.default_rng(seed + VARIANTS.index(variant))
    t = truth(variant)
    base = np.tile(L.params_vector(t), (P, 1))
    if variant == "shared_pose":
        base[:, 7:21] += rng.uniform(-0.01, 0.01, (P, 14))
        return base
    tgt = syn.TARGETS_D21 if variant == "general" else syn.TARGETS_D9
    bounds = orc.bounds_to_array(t, tgt)
    X = rng.uniform(0.45, 0.55, (P, len(tgt)))
    cols = [L.PARAM_KEYS.index(k) for k in tgt]
    base[:, cols] = X * (bounds[:, 1] - bounds[:, 0]) + bounds[:, 0]
    return base


def local_inputs_f32(xyz, uv, o):
    """what a float32 point set stores: coordinates relative to the origin and observations, each rounded to float32"""
    xyz_l = (np.asarray(xyz, np.float64) - o).astype(np.float32).astype(np.float64)
    return xyz_l, np.asarray(uv).astype(np.float32).astype(np.float64)


def oracle_losses(xyz, uv, cand, o=None):
    """float64 oracle {loss name: (P,) losses}: one projection per candidate for both losses.  o: the inputs are relative to
    this origin (the candidates' camera positions are moved with them)"""
    out = {k: np.empty(len(cand)) for k in LOSSES}
    with np.errstate(all="ignore"):
        for i, c in enumerate(cand):
            p = orc.vector_to_params(c)
            if o is not None:
                p.update(x=p["x"] - o[0], y=p["y"] - o[1], z=p["z"] - o[2])
            proj = orc.project_points(xyz, p)
            out["mean_dist"][i] = orc.mean_distance(uv, proj)
            out["huber"][i] = orc.huber(uv, proj, LOSSES["huber"][1])
    return out


# ------------------------------------------------------------------ exact pole of one lens denominator
def oracle_r2(xyz, p):
    """r2 of optimize.py:105-108 for every point, formed operation by operation as oracle.ref_numpy.project_points /
    distort_points form it (so that a denominator built from it is zero in the ORACLE's arithmetic)"""
    hom = np.vstack((np.asarray(xyz, dtype=np.float64).T, np.ones((1, len(xyz)))))
    kmat = orc.intrinsic_mat(p["fov"], p["w"], p["h"], p["cx"], p["cy"])
    emat = orc.extrinsic_mat(p["pan"], p["tilt"], p["roll"], p["x"], p["y"], p["z"])
    img = np.dot(kmat, np.dot(emat, hom)[:3, :])
    uv = np.array([p["w"] - img[0, :] / img[2, :], img[1, :] / img[2, :]]).T
    c = np.array([(p["w"] - 1) / 2, (p["h"] - 1) / 2], dtype="float32")
    x = (uv[:, 0] - c[0]) / c[0]
    y = (uv[:, 1] - c[1]) / c[1]
    return ((x ** 2 + y ** 2) ** 0.5) ** 2


def pole_a2_steps(r2, k4, prec, W=None):
    """a2 values for which 1 + a2 steps ulp by ulp (in the precision of the point set) through -k4 r2, the zero of
    den_y = (1 + a2) + k4 r2 when k5 = k6 = 0 and k4 is minus a power of two (the product k4 r2 is exact).  r2 of a vertex is
    known to the device's arithmetic within a few ulps only (its own folding of the pose and, for float32, its rounded
    coordinates), so one of these candidates sits exactly on the device's pole; the oracle's own pole is at a2 = -k4 r2 - 1.
    W: float64 -- the oracle and the device fold the pose differently (R.(p - cam) against E.[p;1] with |t| ~ 4e6: ~1e-12
    relative = thousands of ulps); float32 -- the stored coordinates are rounded (~1e-6 = some ten ulps).  A caller that forms r2
    in the point set's local frame, as the device does, may pass a smaller W."""
    T, I, W0 = (np.float64, np.int64, 1 << 17) if prec == "f64" else (np.float32, np.int32, 400)
    W = W0 if W is None else W
    centre = np.array([-k4 * r2], dtype=T)
    targets = (centre.view(I)[0] + np.arange(-W, W + 1, dtype=I)).view(T)   # positive floats: consecutive bit patterns
    assert np.all(np.diff(targets) > 0) and 0.5 < targets[0] and targets[-1] < 2
    a2 = targets.astype(np.float64) - 1.0                               # 1 + a2 == t exactly (Sterbenz: t in [0.5, 2])
    assert np.array_equal((1.0 + a2).astype(T), targets)
    return a2
