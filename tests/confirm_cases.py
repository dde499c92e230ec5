"""The scenes, the populations and the restated rules of tests/test_gpu_confirm_seams.py (the argmin confirmation of a float32
point set: alp_points.hip: confirm_losses), in NumPy.

The scene is local: the camera of synthetic.truth_params at the origin, n ground-control-like points relative to it and their
observations (the truth's lens, 1 px of noise), ALL rounded to float32 -- and the origin of both point sets is (0, 0, 0).  The
planes hold float(double(in) - origin), so a float32 set given the float32 arrays and a float64 set given the same arrays
as float64 store the same numbers: the float64 set's losses are what float64 arithmetic gives on the float32 set's points.

A population for a band of B near-tied candidates has 2 B + 1 rows.  The odd rows 1, 3, ... are the near-tied ones: the
truth panned by 0.02 degrees plus j * 1e-9 degrees for the j-th of them, which float32 cannot order (its records of them are
equal or an ulp apart) and float64 tells apart.  The even rows are clearly worse: panned by 0.05 .. 0.5 degrees more, some
pixels of mean distance.  Every candidate carries the truth's lens (k1, k2, p1, p2 non-zero) and its own pan: the general
variant on either set."""
import numpy as np

from alproj_amd import synthetic as syn
from oracle import ref_numpy as orc

CONFIRM_MAX = 16                      # alproj_amd/csrc/host/alp_host.h
CONFIRM_GAP = 5e-5
NUDGE_DEG = 1e-9
K_PAN = 4
LOSSES = {"mean_dist": (orc.LOSS_MEAN_DIST, 0.0), "huber": (orc.LOSS_HUBER, 10.0)}
BANDS = (2, CONFIRM_MAX, 20)
ORIGIN = np.zeros(3)


def point_counts(cu):
    """one masked row, one full row, a second ragged row, four stripes of one row; and rows = 4 CUs + 2, which the
    confirmation cuts into stripes of two rows, the last of them a full row and a row of one point"""
    return {"1": 1, "255": 255, "256": 256, "257": 257, "1000": 1000, "two_row_stripes": 256 * 4 * cu + 257}


def confirm_grid(n, cu):
    """host::confirm_grid (alproj_amd/csrc/host/alp_plan.h), as tests/test_launch_plan.py reads it off the C++"""
    return min(max(-(-n // 256), 1), 4 * cu)


def local_truth():
    t = syn.truth_params(316)
    return dict(t, x=0.0, y=0.0, z=0.0)


def scene(n, weighted, seed=41):
    """(xyz float32 (n, 3), uv float32 (n, 2), weights float32 (n,) or None).  The weights are integers 0 .. 3 with a zero on the
    last point; a set of one point keeps a weight of 2 (weights that sum to 0 are refused: Points.set_weights)."""
    t = syn.truth_params(316)
    xyz = syn.gcp_points(n, t, seed=seed)
    uv = orc.project_points(xyz, t) + np.random.default_rng(seed).normal(0, 1.0, (n, 2))
    local = (xyz - np.array([t["x"], t["y"], t["z"]])).astype(np.float32)
    w = None
    if weighted:
        w = np.random.default_rng(seed + 1).integers(0, 4, n).astype(np.float32)
        w[0] = 3.0
        w[-1] = 0.0 if n > 1 else 2.0
    return local, uv.astype(np.float32), w


def population(band, seed=43):
    """(candidates (2 band + 1, 25), the indices of the near-tied ones)"""
    from alproj_amd import _lib as L
    t = local_truth()
    base = L.params_vector(dict(t, pan=t["pan"] + 0.02))
    cand = np.tile(base, (2 * band + 1, 1))
    near = np.arange(1, 2 * band, 2)
    cand[near, K_PAN] += NUDGE_DEG * np.arange(band)
    worse = np.setdiff1d(np.arange(len(cand)), near)
    cand[worse, K_PAN] += np.random.default_rng(seed).uniform(0.05, 0.5, len(worse))
    return cand, near


def confirm_band(loss):
    """host::confirm_band restated (alproj_amd/csrc/host/alp_host.h): (the candidates whose loss lies within CONFIRM_GAP of the
    smallest one, the up to CONFIRM_MAX of them that are confirmed, in ascending order)"""
    best = np.nanmin(loss)
    band = [int(i) for i in np.flatnonzero(loss <= best + CONFIRM_GAP * abs(best))]
    which = []
    for i in band:
        if len(which) < CONFIRM_MAX:
            which.append(i)
        else:
            worst = 0
            for k in range(1, CONFIRM_MAX):
                a, b = which[k], which[worst]
                if loss[a] > loss[b] or (loss[a] == loss[b] and a > b):
                    worst = k
            if loss[i] < loss[which[worst]]:
                which[worst] = i
    return band, sorted(which)
