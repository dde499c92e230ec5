"""The scene and the populations of tests/test_gpu_mend.py (the mend pass of a float32 point set: alp_points_set_mend), in NumPy.

The scene: g5's camera moved to the origin, g5's points minus the original camera position, and two planted vertices a
centimetre or two from the camera plane -- camera-frame (1000, 300, -0.01) m and (-800, 200, -0.02) m -- all rounded to
float32, with g5's observations plus the rows (100, 100) and (5000, 3000).  It is local on purpose: the oracle's own noise from
the choice of frame is 1e-11 relative with the camera at the origin (and with the whole scene shifted by (512, -256, 128)),
8.5e-9 at g5's UTM position.  The oracle runs on the STORED inputs, the float32-rounded values as float64: a mended loss is
float64 arithmetic on exactly those.

Two kinds of candidate, per kernel variant:
  wild  keeps the pose and carries g5's lens (perturbed): the planted vertex's squared pixel distance is 1.6e43, above FLT_MAX
        by a factor of 10^4.7 -- float32 overflows (inf - inf = NaN), float64 holds it: mean distance around 4e18, Huber ten times
        that;
  tame  stays finite in float32.  General variant (fov varies): pan + 20 degrees, which takes the planted vertices a few hundred
        metres from the camera plane (mean distance ~1.6e3).  Shared-pose variant (lens only -- every candidate has the scene's pose, so
        the pose cannot decide): no lens term that grows with r^4 (k2.. = p = s = 0, a1 / a2 free, a k1 of 1e-13 that keeps the
        population out of the lens-free variant); the planted vertices then sit ~4e8 px out and their squares fit float32.
A flagged set S gives candidate i its wild row when i is in S and its tame row otherwise; the oracle's losses of both rows
are computed once.

Float32 knows a vertex 1 cm from the camera plane to about a per cent (the fold's float32 rows against coordinates of 1000 m),
so where the tame losses are dominated by the planted vertices (shared pose) the oracle's argmin is given a margin float32
cannot blur: candidate BEST has a vertical scale (1 + a1) / (1 + a2) of 0.05, every other tame one a scale of 2 .. 3 (a loss
12 % and more above).  In the general variant BEST is panned by 19 degrees and every other tame candidate by 20 .. 20.5.
`argmin_margin` states the margin of a flagged set and MARGIN what the GPU test asks of it before it compares: a hundred
times the tolerance of the arithmetic that decides (float32 on a well-conditioned candidate 1e-5, a mended loss 1e-7), and 0.1
where the planted vertices decide in float32."""
import os

import numpy as np

from oracle import ref_numpy as orc

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P = 300                                 # three candidate tiles: 128 / 128 / 44
BEST = 150                              # the tame candidate with the smallest loss (never in a partial flagged set): best()
F_SCALE = 10.0
LOSSES = {"mean_dist": (orc.LOSS_MEAN_DIST, 0.0), "huber": (orc.LOSS_HUBER, F_SCALE)}
VARIANTS = ("general", "shared_pose")
PLANTED_CAM = np.array([[1000.0, 300.0, -0.01], [-800.0, 200.0, -0.02]])
PLANTED_UV = np.array([[100.0, 100.0], [5000.0, 3000.0]])
ORIGIN = np.zeros(3)
K_FOV, K_PAN, K_A1, K_A2, K_K1 = 3, 4, 7, 8, 9


def best(n=P):
    """the index of the tame candidate with the smallest loss in a population of n"""
    return BEST if n > BEST else n // 2


def g5():
    return np.load(os.path.join(G, "g5_population.npz"))


def base_params():
    """g5's params_init with the camera at the origin"""
    p = orc.vector_to_params(g5()["params_init"])
    p.update(x=0.0, y=0.0, z=0.0)
    return p


def f32(a):
    """what a float32 point set stores, as float64"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def scene(copies=1, head=None, extra=0):
    """(xyz, uv), float32-rounded float64 arrays: `copies` copies of g5's local points (copy c moved by c x (0.37, -0.21, 0.11) m;
    `head`: only the first `head` points of the first copy; `extra`: that many more points of one further copy), then the two
    planted vertices"""
    g = g5()
    p0 = orc.vector_to_params(g["params_init"])
    local = g["xyz"] - np.array([p0["x"], p0["y"], p0["z"]])
    p = base_params()
    rot = orc.extrinsic_mat(p["pan"], p["tilt"], p["roll"], 0.0, 0.0, 0.0)[:3, :3]
    planted = PLANTED_CAM @ rot                                  # rows: R^T . cam
    step = np.array([0.37, -0.21, 0.11])
    xs, us = [], []
    for c in range(copies):
        xs.append((local if head is None else local[:head]) + c * step)
        us.append(g["uv_obs"] if head is None else g["uv_obs"][:head])
    if extra:
        xs.append(local[:extra] + copies * step)
        us.append(g["uv_obs"][:extra])
    return f32(np.vstack(xs + [planted])), f32(np.vstack(us + [PLANTED_UV]))


def populations(variant, n=P, seed=11):
    """(tame, wild): two (n, 25) candidate matrices of one kernel variant"""
    rng = np.random.default_rng(seed + VARIANTS.index(variant))
    base = orc.params_to_vector(base_params())
    tame, wild = np.tile(base, (n, 1)), np.tile(base, (n, 1))
    wild[:, 7:21] *= 1.0 + rng.uniform(-0.01, 0.01, (n, 14))     # a1 .. s4 within a per cent of g5's
    if variant == "general":
        wild[:, K_FOV] += rng.uniform(-1.0, 1.0, n)
        tame[:, K_PAN] += 20.0 + rng.uniform(0.0, 0.5, n)
        tame[best(n), K_PAN] = base[K_PAN] + 19.0                # a degree nearer: the smallest tame loss by some per cent
        tame[:, K_FOV] += rng.uniform(-1.0, 1.0, n)
        tame[:, 7:21] *= 1.0 + rng.uniform(-0.01, 0.01, (n, 14))
    else:
        tame[:, 9:21] = 0.0
        tame[:, K_K1] = 1e-13
        tame[:, K_A2] = 0.0
        tame[:, K_A1] = rng.uniform(1.0, 2.0, n)                 # vertical scale 2 .. 3
        tame[best(n), K_A1] = -0.95                              # ... and 0.05
    return tame, wild


def oracle(xyz, uv, cand):
    """{loss name: (P,) losses} of the float64 oracle on the arrays as given"""
    out = {k: np.empty(len(cand)) for k in LOSSES}
    with np.errstate(all="ignore"):
        for i, c in enumerate(cand):
            p = orc.vector_to_params(c)
            for name, (kind, fs) in LOSSES.items():
                out[name][i] = orc.loss_of(xyz, uv, p, kind, fs)
    return out


def flagged_sets(n=P):
    """the six flagged sets of the compaction seams: none, the first candidate, the last, exactly one tile, one tile and one,
    all.  The partial ones are scattered over all three tiles (and leave BEST out)."""
    rng = np.random.default_rng(3)
    others = np.array([i for i in range(1, n - 1) if i != best(n)])
    perm = rng.permutation(others)
    sets = {"none": [], "first": [0], "last": [n - 1], "tile": perm[:128], "tile_plus_one": perm[:129], "all": np.arange(n)}
    return {k: np.sort(np.asarray(v, dtype=np.int64)) for k, v in sets.items()}


def mix(tame, wild, flagged):
    cand = tame.copy()
    cand[flagged] = wild[flagged]
    return cand


def mix_losses(tame_l, wild_l, flagged):
    out = {}
    for k in tame_l:
        out[k] = tame_l[k].copy()
        out[k][flagged] = wild_l[k][flagged]
    return out


MARGIN = {("general", False): 1e-3, ("shared_pose", False): 0.1, ("general", True): 1e-5, ("shared_pose", True): 1e-5}   # (variant, all flagged)


def argmin_margin(losses):
    """(argmin, relative gap between the smallest loss and the runner-up)"""
    order = np.argsort(losses, kind="stable")
    a, b = losses[order[0]], losses[order[1]]
    return int(order[0]), float((b - a) / abs(a))


# ---------------------------------------------------------------- host::mend_grid restated (alproj_amd/csrc/host/alp_plan.h)
def mend_grid(n, Pn, V=5, TC=128, cu=256):
    rows, tiles = -(-n // 256), -(-Pn // TC)
    lo, hi = cu * 3, cu * 24
    nblk = min(max(-(-rows // (4 * V)), lo), hi)
    nblk = min(nblk, (128 << 20) // (8 * Pn), rows)
    return max(nblk, 1), max(tiles, 1)
