"""Shared by tests/test_gpu_residuals.py and tests/test_gpu_jacobian.py: the launch rules of the batched residual and Jacobian
entry points restated (alproj_amd/csrc/host/alp_plan.h: stage_chunk_points, stream_grid; alp_point_kernels.h: RES_V;
tests/test_launch_plan.py holds the restatement and the header to each other on the CPU),
scipy's 2-point finite-difference poses around a lens pose, seeded point sets, the bench-shaped 10 M DSM, and the float64 /
float32 references of the residual vectors with the float32 filters and their cap."""
import os

import numpy as np

from alproj_amd import synthetic as syn
from oracle import ref_numpy as orc
from tests.popeval_cases import local_inputs_f32

G = os.path.join(os.path.dirname(__file__), "golden")

RES_V = 3                              # points per lane of residual_batch_kernel: a workgroup covers 768 points per pass
RES_CHUNK_BYTES = 256 << 20            # output staged per launch, at most
B_MAX = 4096                           # alp_residuals_batch refuses more poses
# bounds of |got - ref| / max(|ref|, w): the suite's float64 and float32 residual bounds (tests/test_gpu_lsq.py)
F64_TOL = 1e-9
F32_TOL = 2e-5
# float32 filters (tests/test_gpu_points.py): points whose depth is at least 2 % of their distance, poses whose lens
# denominators stay >= 0.25 over the points; together they may drop at most 2 % of a case's points
F32_DEPTH_FRAC = 0.02
F32_MIN_DEN = 0.25
F32_DROP_CAP = 0.02


# ------------------------------------------------------------------ launch rules
def chunk_points(n, pairs_per_point):
    """points per launch (stage_chunk_points): residuals_impl stages B residual pairs per point, jacobian_impl D; 16 bytes each"""
    c = max(1024, (RES_CHUNK_BYTES // (16 * pairs_per_point)) // 1024 * 1024)
    return min(c, n)


def launches(n, pairs_per_point):
    return -(-n // chunk_points(n, pairs_per_point)) if n else 0


def stride_pass(cu_count):
    """points of one full grid-stride pass: stream_grid caps the grid at cu_count * 8 workgroups of 256 lanes x RES_V points"""
    return cu_count * 8 * 256 * RES_V


def boundary_points(n, chunk, reach=3):
    """every point within `reach` of a chunk boundary and of n"""
    ends = list(range(chunk, n, chunk)) + [n]
    idx = np.concatenate([np.arange(e - reach, e + reach + 1) for e in ends])
    return np.unique(idx[(idx >= 0) & (idx < n)])


def sample_points(n, chunk, step=997):
    """a strided sample, every point next to a chunk boundary and the last ones"""
    return np.unique(np.r_[np.arange(0, n, step), boundary_points(n, chunk)])


# ------------------------------------------------------------------ poses
def lens_pose():
    """g5's camera (UTM coordinates, every lens term non-zero)"""
    return orc.vector_to_params(np.load(os.path.join(G, "g5_population.npz"))["params_init"])


def fd_poses(p, targets=tuple(syn.TARGETS_D21)):
    """the D + 1 poses of scipy's 2-point differences at p (scipy.optimize._numdiff, no bounds): x0, then x0 + h_j e_j with
    h_j = sqrt(eps) sign(x0_j) max(1, |x0_j|), sign(0) = +1 -> (D + 1, 25)"""
    base = orc.params_to_vector(p)
    cols = [orc.PARAM_KEYS.index(t) for t in targets]
    x0 = base[cols]
    h = np.finfo(np.float64).eps ** 0.5 * np.where(x0 >= 0, 1.0, -1.0) * np.maximum(1.0, np.abs(x0))
    cand = np.tile(base, (len(cols) + 1, 1))
    cand[np.arange(1, len(cols) + 1), cols] += h
    return cand


def spread_poses(p, B, seed):
    """B poses: the 22 finite-difference poses at p, then poses moved around p by a few metres, a few tenths of a degree and
    a few thousandths in every lens term"""
    rng = np.random.default_rng(seed)
    fd = fd_poses(p)
    cand = np.tile(orc.params_to_vector(p), (B, 1))
    k = min(B, len(fd))
    cand[:k] = fd[:k]
    scale = {"x": 2.0, "y": 2.0, "z": 2.0, "fov": 0.3, "pan": 0.3, "tilt": 0.3, "roll": 0.3}
    for t in syn.TARGETS_D21:
        j = orc.PARAM_KEYS.index(t)
        cand[k:, j] += rng.uniform(-1, 1, B - k) * scale.get(t, 2e-3)
    return cand


def camera(p):
    return np.array([p["x"], p["y"], p["z"]])


# ------------------------------------------------------------------ point sets
def gcp_case(n, p, seed):
    """n GCP-like points in front of p (absolute coordinates) and their observations: the oracle's pixels + 1 px noise"""
    xyz = syn.gcp_points(n, p, seed=seed)
    uv = orc.project_points(xyz, p) + np.random.default_rng(seed).normal(0, 1.0, (n, 2))
    return xyz, uv


def dsm10_case(L):
    """bench.py's f1 leg: the 10 M DSM (local float32 vertices, origin at the standoff camera), its 22 poses (pan spread
    over +-0.5 degrees) and its observations (the device's float64 projection of the perturbed pose + 1 px noise)"""
    n10 = syn.grid_side(10_000_000)
    s10 = syn.surface(n10)
    x10 = syn.vert_to_xyz_local(s10["vert"])
    b10 = syn.local_params(syn.standoff_params(n10), s10["offsets"])
    t10 = syn.local_params(syn.perturbed(syn.standoff_params(n10)), s10["offsets"])
    del s10
    n = len(x10)
    with L.Points(x10, camera(b10), "f64") as p:
        p.project(L.params_vector(t10))
        u, v = p.fetch()
    uv = np.stack([u, v], 1) + np.random.default_rng(2).normal(0, 1.0, (n, 2))
    del u, v
    cand = np.tile(L.params_vector(b10), (22, 1))
    cand[:, orc.PARAM_KEYS.index("pan")] += np.linspace(-0.5, 0.5, 22)
    return x10, uv, cand, b10


# ------------------------------------------------------------------ references
def local_pose(c, o):
    """the parameters of candidate c with its camera position moved into the frame of origin o"""
    p = orc.vector_to_params(c)
    p.update(x=p["x"] - o[0], y=p["y"] - o[1], z=p["z"] - o[2])
    return p


def f32_filters(xyz, cand, well_conditioned):
    """float32 filters over the points xyz (in the frame of cand): (points kept for every pose, poses kept)"""
    keep_pts = np.ones(len(xyz), bool)
    keep_pose = np.ones(len(cand), bool)
    for b, c in enumerate(cand):
        p = orc.vector_to_params(c)
        keep_pts &= well_conditioned(xyz, p, F32_DEPTH_FRAC)
        keep_pose[b] = orc.conditioning(xyz, p)[1] >= F32_MIN_DEN
    return keep_pts, keep_pose


def worst_ratio(got, ref, w):
    """max |got - ref| / max(|ref|, w) over values of which both are finite; inf if one of them only is"""
    fin = np.isfinite(ref)
    if not np.array_equal(fin, np.isfinite(got)):
        return np.inf
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), w)).max())


def compare_with_oracle(got, xyz, uv, cand, prec, o, rows=None, well_conditioned=None, label=""):
    """rows `rows` (all by default) of every pose b of got (B, 2n) against the float64 oracle: on the absolute inputs within
    F64_TOL for a float64 set; on what a float32 set stores (coordinates relative to o and observations, rounded to float32)
    within F32_TOL, after the float32 filters, which may drop at most F32_DROP_CAP of the points (a dropped pose counts as all
    of them).  -> (worst ratio, points dropped, poses dropped)"""
    n = len(xyz)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    xs, us = np.asarray(xyz, np.float64)[rows], np.asarray(uv, np.float64)[rows]
    g = got.reshape(len(cand), n, 2)[:, rows]
    w = float(cand[0, orc.PARAM_KEYS.index("w")])
    worst = 0.0
    with np.errstate(all="ignore"):
        if prec == "f64":
            for b, c in enumerate(cand):
                ref = orc.residual_vector(xs, us, orc.vector_to_params(c)).reshape(-1, 2)
                r = worst_ratio(g[b], ref, w)
                assert r <= F64_TOL, (label, b, r)
                worst = max(worst, r)
            return worst, 0, 0
        keep_pts, keep_pose = f32_filters(xs, cand, well_conditioned)
        dropped_pts, dropped_poses = int((~keep_pts).sum()), int((~keep_pose).sum())
        assert dropped_pts <= F32_DROP_CAP * len(rows) and dropped_poses == 0, (label, dropped_pts, dropped_poses)
        xl, ul = local_inputs_f32(xs, us, o)
        for b, c in enumerate(cand):
            ref = orc.residual_vector(xl[keep_pts], ul[keep_pts], local_pose(c, o)).reshape(-1, 2)
            r = worst_ratio(g[b][keep_pts], ref, w)
            assert r <= F32_TOL, (label, b, r)
            worst = max(worst, r)
    print(f"[residuals f32] {label}: worst |d| / max(|ref|, w) = {worst:.3e}; the filters dropped {dropped_pts} of {len(rows)} "
          f"points and {dropped_poses} of {len(cand)} poses")
    return worst, dropped_pts, dropped_poses
