"""Drop-in counterpart of the reference module ``alproj.optimize`` (src/alproj/optimize.py)
whose per-point arithmetic runs on an MI355X through libalproj_hip.so.

Same names, argument meaning and return types as the reference:

============================  =======================================  ======================
here                          reference                                device entry point
============================  =======================================  ======================
``project``                   optimize.py:122-155                      alp_project
``rmse`` / ``huber_loss``     optimize.py:157-178 / :181-212           alp_loss_uv
``compute_residuals``         optimize.py:215-237                      alp_residuals
``bounds_to_array``           optimize.py:249-276                      (host, D <= 21 scalars)
``CMAOptimizer.optimize``     optimize.py:359-439                      alp_eval_population, alp_cma_*
``LsqOptimizer.optimize``     optimize.py:467-539                      alp_residuals; method="normal": alp_normal_equations(_batch)
``LsqOptimizer.cross_validate`` / ``.bootstrap``  (none: held-out error, parameter spread)  alp_normal_equations_batch_rows, alp_residuals_assigned
``parameter_covariance``      (none: standard errors of a fit)         alp_jacobian, alp_residuals; "normal": alp_normal_equations
``intrinsic_mat`` etc.        optimize.py:8-96                         (host, 3x3 / 4x4)
============================  =======================================  ======================

Extra keyword arguments (all optional, defaults keep the reference behaviour):
``precision`` (None | "f32" | "f64") selects the element type of the device-resident point set
-- None, the default, is the reference's own float64 arithmetic (optimize.py:329-357) for every
point set of up to ``F64_MAX_POINTS`` = 4 M points (any GCP-scale use of the reference: float64
costs nothing there) and float32 (20 B/vertex, ~1e-3 px) for DSM-sized sets above it;
``seed`` makes the CMA-ES trajectory reproducible; ``starts=K`` runs K seeded CMA-ES starts side by side and keeps the
best (``CMAOptimizer.optimize``); ``jac="analytic"`` gives ``LsqOptimizer.optimize`` the exact Jacobian (alp_jacobian).  There is no CPU fallback: without the
HIP library / a GPU every function that touches points raises ``AlprojHipError``.
"""
from contextlib import nullcontext
from math import cos, pi, sin, tan

import numpy as np
import pandas as pd
from scipy.optimize import least_squares
from tqdm import tqdm

from . import _lib, resample
from .cma import CMA

__all__ = ["intrinsic_mat", "extrinsic_mat", "project", "rmse", "huber_loss",
           "compute_residuals", "DEFAULT_BOUND_WIDTHS", "bounds_to_array", "BaseOptimizer",
           "CMAOptimizer", "LsqOptimizer", "start_seeds", "best_start", "normal_lm", "normal_lm_batch"]


# ------------------------------------------------------------------------------------------
# host scalars (per pose, not per point)
# ------------------------------------------------------------------------------------------
def intrinsic_mat(fov_x_deg, w, h, cx=None, cy=None):
    """OpenCV-style intrinsic matrix (reference optimize.py:8-44; fov_y = fov_x * h / w)."""
    if cx is None:
        cx = w / 2
    if cy is None:
        cy = h / 2
    half_x = fov_x_deg * pi / 180 / 2
    half_y = (fov_x_deg * pi / 180) * h / w / 2
    return np.array([[w / (2 * tan(half_x)), 0, cx],
                     [0, h / (2 * tan(half_y)), cy],
                     [0, 0, 1]], dtype=np.float64)


def extrinsic_mat(pan_deg, tilt_deg, roll_deg, t_x, t_y, t_z):
    """4x4 extrinsic matrix (reference optimize.py:46-96): Rx(-(tilt+90)) Ry(-roll) Rz(pan)."""
    a, b, c = pan_deg * pi / 180, -(tilt_deg + 90) * pi / 180, -roll_deg * pi / 180
    rz = np.array([[cos(a), -sin(a), 0], [sin(a), cos(a), 0], [0, 0, 1.0]])
    rx = np.array([[1.0, 0, 0], [0, cos(b), -sin(b)], [0, sin(b), cos(b)]])
    ry = np.array([[cos(c), 0, sin(c)], [0, 1.0, 0], [-sin(c), 0, cos(c)]])
    rot = rx @ ry @ rz
    m = np.eye(4)
    m[:3, :3] = rot
    m[:3, 3] = rot @ np.array([-t_x, -t_y, -t_z], dtype=np.float64)
    return m


def _camera_origin(params):
    return np.array([float(params["x"]), float(params["y"]), float(params["z"])])


def _columns(frame, names):
    """The named columns of a DataFrame as the device upload takes them, WITHOUT the copies of the reference's
    `obj_points[["x", "y", "z"]]` + `np.array(...)` (optimize.py:139-141; 96 ms for 10 M rows on one core): columns that lie
    contiguous in the frame's blocks are handed out as they are (a list of 1-D views); a frame that IS a row-major (N, k)
    float64 array hands out that array; only strided or non-float64 columns are copied, one by one."""
    cols = [frame[c].to_numpy() for c in names]                   # views of the frame's blocks: nothing is copied yet
    if all(c.dtype == np.float64 and c.flags["C_CONTIGUOUS"] for c in cols):
        return cols                                                # columns x rows blocks (or one block per column): as they lie
    if list(frame.columns) == list(names) and all(dt == np.float64 for dt in frame.dtypes):
        a = frame.to_numpy(copy=False)                             # one block holding a row-major (N, k) array: as it lies
        if a.flags["C_CONTIGUOUS"]:
            return a
    return [np.ascontiguousarray(c, dtype=np.float64) for c in cols]


def _first_two_columns(frame):
    """columns 0 and 1 of a DataFrame, whatever their labels, without copying where they lie contiguous"""
    if frame.shape[1] < 2:
        raise IndexError("index 1 is out of bounds for axis 1 with size %d" % frame.shape[1])      # numpy's, as the reference raises it
    cols = [frame.iloc[:, k].to_numpy() for k in (0, 1)]
    if all(c.dtype == np.float64 and c.flags["C_CONTIGUOUS"] for c in cols):
        return cols
    return [np.ascontiguousarray(c, dtype=np.float64) for c in cols]


def _xyz_array(obj_points):
    if isinstance(obj_points, pd.DataFrame):
        return _columns(obj_points, ["x", "y", "z"])
    return np.asarray(obj_points, dtype=np.float64)


def _uv_array(img_points):
    if isinstance(img_points, pd.DataFrame):
        return _columns(img_points, ["u", "v"])
    return np.asarray(img_points, dtype=np.float64)


def _rows(a):
    return len(a[0]) if isinstance(a, list) else len(a)


def _points(xyz, origin, precision):
    """device point set from what _xyz_array returned: an (N, 3) array or a list of three columns"""
    if isinstance(xyz, list):
        return _lib.Points.from_columns(xyz[0], xyz[1], xyz[2], origin, precision)
    return _lib.Points(xyz, origin, precision)


def _set_observed(pts, uv):
    if isinstance(uv, list):
        pts.set_observed_columns(uv[0], uv[1])
    else:
        pts.set_observed(uv)


def _as_rows(a):
    """(N, k) row-major float64 for the few callers that need the array itself"""
    return np.ascontiguousarray(np.column_stack(a) if isinstance(a, list) else a, dtype=np.float64)


# ------------------------------------------------------------------------------------------
# projection and losses
# ------------------------------------------------------------------------------------------
F64_MAX_POINTS = 4_000_000


def default_precision(n_points, precision=None):
    """The element type of a device-resident point set when the caller names none: the reference's float64
    (optimize.py:139-154, 329-357) up to F64_MAX_POINTS points, float32 above (DSM-sized sets, where the float64
    population kernel costs 3 x the float32 one and the set 2 x the HBM)."""
    if precision is not None:
        if precision not in ("f32", "f64"):
            raise ValueError("precision must be None, 'f32' or 'f64'")
        return precision
    return "f64" if int(n_points) <= F64_MAX_POINTS else "f32"


def project(obj_points, params, precision="f64"):
    """3D -> 2D perspective projection of ``obj_points`` (DataFrame with x, y, z) with the
    camera ``params``; returns a DataFrame with columns u, v (reference optimize.py:122-155).

    The points are uploaded relative to the camera position, projected by one HIP kernel and
    fetched back.  ``precision="f64"`` (default) reproduces the float64 reference to ~1e-12;
    ``"f32"`` streams 20 B/vertex and is accurate to ~1e-3 px.
    """
    xyz = _xyz_array(obj_points)
    with _points(xyz, _camera_origin(params), precision) as pts:
        pts.project(_lib.params_vector(params))
        u, v = pts.fetch(np.float64)
    return pd.DataFrame({"u": u, "v": v}, copy=False)      # the two result arrays ARE the columns (no 16 N-byte copy)


def _uv_pointers(a):
    """(pointer to u or to the interleaved pairs, pointer to v or None, rows, what must stay alive) for alp_loss_uv_columns"""
    if isinstance(a, list):
        cols = [np.ascontiguousarray(c, dtype=np.float64) for c in a]
        return _lib.as_dp(cols[0]), _lib.as_dp(cols[1]), len(cols[0]), cols
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("pixel coordinates must have shape (N, 2)")
    if not a.flags["C_CONTIGUOUS"] and a.shape[0] > 1 and a[:, 0].flags["C_CONTIGUOUS"] and a[:, 1].flags["C_CONTIGUOUS"]:
        cols = [a[:, 0], a[:, 1]]
        return _lib.as_dp(cols[0]), _lib.as_dp(cols[1]), a.shape[0], cols
    a = np.ascontiguousarray(a)
    return _lib.as_dp(a), None, a.shape[0], a


def _loss_uv(img_points, projected, kind, f_scale):
    """rmse / huber_loss of two tables of pixel coordinates: each goes to the device as it lies -- row-major pairs or two
    columns (what project() returns) -- through alp_loss_uv_columns; no host-side interleaving"""
    # the reference takes `projected` BY POSITION (projected.to_numpy()[:, 0], [:, 1]: optimize.py:175-176, 203-206) and only
    # img_points by name: an unlabelled frame works, a frame ordered [v, u] is read as it lies
    prj = _first_two_columns(projected) if isinstance(projected, pd.DataFrame) else projected
    ou, ov, n_obs, keep_o = _uv_pointers(_uv_array(img_points))
    pu, pv, n_prj, keep_p = _uv_pointers(prj)
    if n_obs != n_prj:
        raise ValueError("img_points and projected must have the same shape")
    out = _lib.ctypes.c_double()
    _lib.check(_lib.lib().alp_loss_uv_columns(ou, ov, pu, pv, n_obs, kind, float(f_scale), _lib.ctypes.byref(out)))
    del keep_o, keep_p
    return float(out.value)


def rmse(img_points, projected):
    """Mean Euclidean reprojection distance in pixels -- what the reference calls RMSE
    (optimize.py:157-178)."""
    return _loss_uv(img_points, projected, _lib.LOSS_MEAN_DIST, 0.0)


def huber_loss(img_points, projected, f_scale=10.0):
    """Mean Huber loss of the reprojection distance (reference optimize.py:181-212)."""
    return _loss_uv(img_points, projected, _lib.LOSS_HUBER, f_scale)


def compute_residuals(obj_points, img_points, params):
    """Flattened residual vector (observed - projected), reference optimize.py:215-237."""
    xyz = _xyz_array(obj_points)
    with _points(xyz, _camera_origin(params), "f64") as pts:
        _set_observed(pts, _uv_array(img_points))
        return pts.residuals(_lib.params_vector(params))


def _jacobian_targets(target_params):
    """PARAM_KEYS indices of the targets of an exact Jacobian (alp_jacobian); ValueError, before any GPU call, for w / h,
    an unknown key or a repeated one"""
    targets = list(target_params)
    for t in targets:
        if t not in _lib.PARAM_KEYS:
            raise ValueError(f"unknown parameter {t!r}")
    return _lib.normal_targets_check([_lib.PARAM_KEYS.index(t) for t in targets])


def _covariance_from_normal_equations(G, rtr, m):
    """s^2 G^-1 from the eigendecomposition of the Jacobi-scaled G (unit diagonal), s^2 = rtr / (m - D); inf when the scaled
    matrix is rank-deficient by numpy's matrix_rank rule (its smallest eigenvalue <= D eps times its largest) or a column of
    J is zero"""
    d = G.shape[0]
    dg = np.sqrt(np.diag(G))
    if not (dg > 0).all():
        return np.full((d, d), np.inf)
    lam, V = np.linalg.eigh(G / np.outer(dg, dg))
    if lam[0] <= d * np.finfo(np.float64).eps * lam[-1]:
        return np.full((d, d), np.inf)
    return (V / lam) @ V.T * (rtr / (m - d)) / np.outer(dg, dg)


def parameter_covariance(obj_points, img_points, params, target_params, method="svd"):
    """Covariance and standard errors of the camera parameters ``target_params`` fitted to the GCPs, at ``params``:
    ``cov`` = s^2 (J^T J)^-1 with s^2 = r^T r / (2N - D), J the exact (2N, D) Jacobian of the residual vector r (one
    ``alp_jacobian`` and one ``alp_residuals`` call on a float64 point set), formed from the SVD of J.  Returns
    ``(cov, std)`` with ``std = {target: sqrt(cov[j, j])}``.  When J is rank-deficient to working precision (a singular
    value <= max(2N, D) eps sigma_max, numpy's matrix_rank rule) the targets cannot all be determined from these GCPs:
    ``cov`` and ``std`` are inf.  With several ranks J and r are gathered first: every rank returns the same numbers.
    ValueError for w / h or repeated targets, or for 2N <= D.

    ``method="normal"`` (opt-in) never forms J: one ``alp_normal_equations`` call with the linear loss returns J^T J, r^T r
    and the point count, summed over the ranks on the device -- (D + 1)(D + 2) / 2 + 1 doubles cross PCIe instead of the
    (2N, D) matrix, and nothing is gathered.  ``cov`` then comes from the eigendecomposition of J^T J scaled to a unit
    diagonal, and rank deficiency is numpy's matrix_rank rule applied to THAT D x D matrix: lambda_min <= D eps lambda_max.
    This rule sees the SQUARED condition number of the column-scaled J -- the eigenvalues of J^T J are the squares of J's
    singular values -- so it declares deficiency earlier than the SVD of J does (at a condition number of about
    1 / sqrt(D eps) ~ 1e7 instead of 1 / (2N eps)), and the entries of ``cov`` carry a relative error of about the squared
    condition number times eps instead of the condition number times eps.  That is why ``"svd"`` stays the default: choose
    ``"normal"`` for point sets whose Jacobian is too large to move, with targets that are well determined."""
    if method not in ("svd", "normal"):
        raise ValueError("method must be 'svd' or 'normal'")
    targets = list(target_params)
    cols = _jacobian_targets(targets)
    xyz = _xyz_array(obj_points)
    _, world = _lib.comm_info()
    if world == 1 and 2 * _rows(xyz) <= len(targets):
        raise ValueError(f"{_rows(xyz)} points give {2 * _rows(xyz)} residuals: not more than the {len(targets)} targets")
    pvec = _lib.params_vector(params)
    with _points(xyz, _camera_origin(params), "f64") as pts:
        _set_observed(pts, _uv_array(img_points))
        if method == "normal":
            G, _, cost, n_total = pts.normal_equations(pvec, cols, "linear", 1.0)
        else:
            J = pts.jacobian(pvec, cols, of_residuals=True)
            r = pts.residuals(pvec)
    if method == "normal":
        m, d = 2 * n_total, len(targets)
        if m <= d:
            raise ValueError(f"{m} residuals: not more than the {d} targets")
        if not (np.isfinite(G).all() and np.isfinite(cost)):
            raise ValueError("the residuals or their Jacobian are not finite at these parameters")
        cov = _covariance_from_normal_equations(G, 2.0 * cost, m)
        return cov, {t: float(np.sqrt(cov[j, j])) for j, t in enumerate(targets)}
    if world > 1:
        J, r = _lib.comm_allgather(J), _lib.comm_allgather(r)
    m, d = J.shape
    if m <= d:
        raise ValueError(f"{m} residuals: not more than the {d} targets")
    if not (np.isfinite(J).all() and np.isfinite(r).all()):
        raise ValueError("the residuals or their Jacobian are not finite at these parameters")
    _, sv, vt = np.linalg.svd(J, full_matrices=False)
    if sv[-1] <= max(m, d) * np.finfo(np.float64).eps * sv[0]:
        cov = np.full((d, d), np.inf)
    else:
        s2 = float(r @ r) / (m - d)
        cov = (vt.T / sv ** 2) @ vt * s2
    return cov, {t: float(np.sqrt(cov[j, j])) for j, t in enumerate(targets)}


# ------------------------------------------------------------------------------------------
# optimisers
# ------------------------------------------------------------------------------------------
DEFAULT_BOUND_WIDTHS = {
    "fov": 45, "pan": 45, "tilt": 45, "roll": 45,
    "x": 30, "y": 30, "z": 30,
    "a1": 0.2, "a2": 0.2,
    "k1": 0.2, "k2": 0.2, "k3": 0.2, "k4": 0.2, "k5": 0.2, "k6": 0.2,
    "p1": 0.2, "p2": 0.2,
    "s1": 0.2, "s2": 0.2, "s3": 0.2, "s4": 0.2,
}


def bounds_to_array(params_init, target_params, bound_widths=None):
    """(D, 2) array [init - width, init + width] (reference optimize.py:249-276); keys missing
    from both ``bound_widths`` and DEFAULT_BOUND_WIDTHS get width 0.2."""
    widths = bound_widths or {}
    centre = np.array([params_init[k] for k in target_params], dtype=np.float64)
    half = np.array([widths.get(k, DEFAULT_BOUND_WIDTHS.get(k, 0.2)) for k in target_params],
                    dtype=np.float64)
    return np.column_stack([centre - half, centre + half]).reshape(len(target_params), 2)


def _scale_rows(a, sw):
    """a * sw where sw > 0, exact zeros elsewhere (a NaN or infinite row of a point of weight 0 stays out)"""
    with np.errstate(invalid="ignore"):
        return np.where(sw > 0, a * sw, 0.0)


class BaseOptimizer:
    """Holds GCP object/image points and the initial parameters (reference optimize.py:279-319).

    ``weights`` (not in the reference): one frequency weight per point, finite and >= 0, array-like of length N -- this rank's
    shard, like the points.  With integer weights every optimiser below solves the problem in which point i appears w_i
    times (a weight of 0 takes the point out without another upload), and the error returned is the weighted mean distance
    sum w_i d_i / sum w_i.  ValueError, before the GPU is touched, for another length, a negative or non-finite weight, or --
    without a communicator -- weights that are all 0."""

    def __init__(self, obj_points, img_points, params_init, weights=None):
        self.obj_points = obj_points
        self.img_points = img_points
        self.params_init = params_init
        self.weights = None if weights is None else _lib.weights_check(weights, len(obj_points)).astype(np.float64)

    def set_target(self, target_params=["fov", "pan", "tilt", "roll", "a1", "a2", "k1", "k2", "k3",
                                        "k4", "k5", "k6", "p1", "p2", "s1", "s2", "s3", "s4"]):
        """Choose the parameters to optimise (x, y, z may be added)."""
        self.target_params = target_params
        self.target_params_init = np.array([self.params_init[t] for t in target_params])

    # -- device-resident copy of the GCPs, shared by both optimisers -------------------------
    def _device_points(self, precision=None):
        xyz = _xyz_array(self.obj_points)
        pts = _points(xyz, _camera_origin(self.params_init), default_precision(_rows(xyz), precision))
        _set_observed(pts, _uv_array(self.img_points))
        if self.weights is not None:
            pts.set_weights(self.weights)
        return pts

    def _row_scale(self):
        """sqrt(w_i) for both residual rows of point i (2N,), or None without weights: what trf / dogbox / lm multiply the
        residual vector and the rows of the Jacobian by (a weight of 0 SELECTS 0: a non-finite row of an absent point stays out)"""
        return None if self.weights is None else np.repeat(np.sqrt(self.weights), 2)

    def _candidate_matrix(self, values):
        """(P, D) target values -> (P, 25) ABI parameter vectors (non-target keys from
        params_init), the vectorised form of reference optimize.py:341-350."""
        values = np.atleast_2d(np.asarray(values, dtype=np.float64))
        base = _lib.params_vector(self.params_init)
        cand = np.tile(base, (values.shape[0], 1))
        cols = [_lib.PARAM_KEYS.index(t) for t in self.target_params]
        cand[:, cols] = values
        return cand

    def _result_params(self, best_values):
        params = self.params_init.copy()
        for t in self.target_params:
            params.pop(t)
        params.update(dict(zip(self.target_params, best_values)))
        return params


def start_seeds(seed, starts):
    """The seeds of ``CMAOptimizer.optimize(..., starts=K)``: start k uses ``seed + k`` mod 2**63.  ``seed=None`` draws one
    base seed the way ``cma.CMA`` draws its own (with a communicator, rank 0's is broadcast before this is called)."""
    base = int(np.random.SeedSequence().entropy % (1 << 63)) if seed is None else int(seed)
    return [(base + k) % (1 << 63) for k in range(int(starts))]


def best_start(errors):
    """The start ``CMAOptimizer.optimize(..., starts=K)`` returns: the smallest final error, the lowest index on ties; a NaN
    error never wins unless every error is NaN, and then start 0 does."""
    e = np.asarray(errors, dtype=np.float64)
    ok = ~np.isnan(e)
    return int(np.flatnonzero(ok)[np.argmin(e[ok])]) if ok.any() else 0


class CMAOptimizer(BaseOptimizer):
    """CMA-ES optimiser of the camera parameters (reference optimize.py:322-439).

    One generation = one ``alp_eval_population`` call: all ``population_size`` candidates are
    projected against every point and reduced to their losses by a single kernel (plus, with
    several GPUs, one RCCL all-reduce of the per-candidate sums).
    """

    def _loss_function(self, bounds, f_scale=None, precision=None):
        """Population loss closure: X (P, D) in [0,1] -> (losses (P,), argmin).  Vectorised
        counterpart of the reference's per-candidate ``_proj_error`` (optimize.py:347-356)."""
        lower, upper = bounds[:, 0], bounds[:, 1]
        pts = self._device_points(precision)
        kind = _lib.LOSS_MEAN_DIST if f_scale is None else _lib.LOSS_HUBER
        fs = 0.0 if f_scale is None else float(f_scale)

        def _proj_error(normalized_values, want_argmin=True):
            x = np.atleast_2d(np.asarray(normalized_values, dtype=np.float64))
            cand = self._candidate_matrix(x * (upper - lower) + lower)
            return pts.eval_population(cand, kind, fs, want_argmin)

        _proj_error.points, _proj_error.kind, _proj_error.f_scale = pts, kind, fs
        return _proj_error

    DEVICE_LOOP_MAX_POPULATION = 4096
    DEVICE_LOOP_MAX_TARGETS = 32

    def _check_device_loop(self, generation, population_size):
        """the configurations device_loop=True does not cover: ValueError before the GPU is touched"""
        if int(generation) < 1:
            raise ValueError("device_loop=True needs generation >= 1")
        if int(population_size) > self.DEVICE_LOOP_MAX_POPULATION:
            raise ValueError(f"device_loop=True supports population_size <= {self.DEVICE_LOOP_MAX_POPULATION}")
        if len(self.target_params) > self.DEVICE_LOOP_MAX_TARGETS:
            raise ValueError(f"device_loop=True supports at most {self.DEVICE_LOOP_MAX_TARGETS} targets")
        if "w" in self.target_params or "h" in self.target_params:
            raise ValueError("w and h cannot be optimised: every candidate must share the image size")

    MAX_STARTS = 1024
    MAX_START_CANDIDATES = 65536

    def _check_starts(self, starts, population_size):
        """the multi-start configurations optimize() refuses: ValueError before the GPU is touched (a single start keeps
        alp_eval_population's own population limit)"""
        if int(starts) != starts or int(starts) < 1:
            raise ValueError("starts must be a positive integer")
        if int(starts) > self.MAX_STARTS:
            raise ValueError(f"starts must be at most {self.MAX_STARTS}")
        if int(starts) > 1 and int(starts) * int(population_size) > self.MAX_START_CANDIDATES:
            raise ValueError(f"starts * population_size must be at most {self.MAX_START_CANDIDATES}")

    def optimize(self, sigma=0.2, bound_widths=None, generation=1000, population_size=10,
                 n_max_resampling=100, f_scale=None, precision=None, seed=None, progress=True, device_loop=False, starts=1,
                 mend_nonfinite=False):
        """Run CMA-ES; returns ``(params, error)`` like the reference: the best candidate of
        the LAST generation (optimize.py:427, quirk Q9) and its mean reprojection distance.
        ``precision=None``: float64 like the reference up to F64_MAX_POINTS points (per rank), float32 above.
        ``starts=K``: K independent starts, start k the run ``optimize(seed=seed + k)`` (``start_seeds``) would make: one
        evaluation of all K * population_size candidates and K tells per generation, the last generation one evaluation (with
        its argmin) per start; returns the start with the smallest final error (``best_start``).  1 <= K <= 1024, K *
        population_size <= 65536 for K > 1.  ``self.start_results``: the ``(seed, params, error)`` of every start in start order.
        ``device_loop=True``: generations 0 .. G-2 of all starts run in one device loop (alp_cma_run: draw, candidate matrix,
        fold, evaluation, K tells, no host round trip in between); the states then come back into the host CMAs once and the
        LAST generation runs on the host.  population_size <= 4096, at most 32 targets.
        ``mend_nonfinite=True`` (float32 point sets; a float64 set ignores it): every candidate whose float32 loss comes out
        infinite or NaN -- a third of a first generation at sigma = 1, where a vertex next to a candidate's camera plane
        overflows float32 -- is evaluated again on the device in float64 arithmetic on the stored float32 points
        (``Points.set_mend``), in the host loop and in the device loop alike, so that CMA-ES ranks it by its loss and not as
        +inf.  A mended loss is exact for the stored points, not the reference's to 1e-5 (the float32 rounding of the points
        is its floor); one that float64 cannot hold either (an exact pole, a vertex at the camera) stays +inf or NaN.  Off by
        default: the pass costs a scan and three small launches per generation even when nothing is flagged -- 0.01 to 0.02
        ms, which is nothing next to the 21 ms of a 10 M x 2048 generation but 8 % of the 0.147 ms a float32 generation of
        the device loop takes at the GCP size (1127 points, pop 50; float64, the default there, runs no pass) -- and with
        several ranks one more all-reduce of population_size doubles."""
        self._check_starts(starts, population_size)
        if device_loop:
            self._check_device_loop(generation, population_size)
        bounds = bounds_to_array(self.params_init, self.target_params, bound_widths)
        lower, upper = bounds[:, 0], bounds[:, 1]
        normalized_init = (self.target_params_init - lower) / (upper - lower)
        d = len(self.target_params)
        normalized_bounds = np.column_stack([np.zeros(d), np.ones(d)])

        # Several ranks (one process per GPU, vertices sharded): every population evaluation
        # all-reduces the per-candidate sums, so every rank MUST evaluate the same candidates.
        # The reference seeds nothing (optimize.py:410-416); here rank 0's seed (its own entropy
        # when seed is None) and, every generation, rank 0's candidate matrix are broadcast.
        # Rank 0's element type travels with the seed: the float64 confirmation of near-tied float32
        # losses is a collective of its own, so shards on either side of F64_MAX_POINTS must not differ.
        precision = default_precision(len(self.obj_points), precision)
        _, world = _lib.comm_info()
        if world > 1:
            s = np.array([np.random.SeedSequence().entropy % (1 << 63) if seed is None else int(seed),
                          precision == "f64"], dtype=np.uint64)
            _lib.comm_bcast(s, root=0)
            seed, precision = int(s[0]), ("f64" if s[1] else "f32")
        loss_function = self._loss_function(bounds, f_scale, precision)
        pts = loss_function.points
        try:
            if mend_nonfinite:
                pts.set_mend(True)
            seeds = start_seeds(seed, starts)
            K, P = len(seeds), int(population_size)
            # the device sampler costs a launch + a copy (~0.07 ms): it pays from a few thousand
            # deviates per generation (pop 256 / D 21: 0.10 ms against 7 ms of numpy at sigma = 1);
            # at GCP scale (pop 50 / D 9) the numpy path is the faster one (0.17 vs 0.24 ms / generation)
            sampler = _lib.cma_sample if (device_loop or (d <= 32 and population_size * d >= 2048)) else None
            opts = [CMA(mean=normalized_init.astype("float64"), sigma=float(sigma), bounds=normalized_bounds,
                        population_size=population_size, n_max_resampling=n_max_resampling, seed=s, sampler=sampler) for s in seeds]
            first = 0
            if device_loop and generation > 1:
                # every rank runs the same replica: the sums are all-reduced, the tell is deterministic
                loop = _lib.CmaDevice(pts, _lib.params_vector(self.params_init), [_lib.PARAM_KEYS.index(t) for t in self.target_params],
                                      lower, upper, opts[0], seeds=[o._sampler_seed for o in opts])
                try:
                    for k, o in enumerate(opts):
                        loop.set_state(o.get_state(), start=k)
                    loop.run(generation - 1, loss_function.kind, loss_function.f_scale)
                    loop.wait()
                    for k, o in enumerate(opts):
                        o.set_state(loop.get_state(start=k))
                finally:
                    loop.close()
                first = generation - 1
            it = range(first, generation)
            best_normalized = [normalized_init] * K
            for g in (tqdm(it) if progress else it):
                X = np.ascontiguousarray(np.concatenate([o.ask_population() for o in opts]))
                if world > 1:
                    _lib.comm_bcast(X, root=0)
                if g == generation - 1:
                    # the result is the best candidate of the LAST generation (optimize.py:427, quirk Q9): only there is the
                    # argmin itself needed -- and confirmed in float64 among near-tied candidates of a float32 point set
                    for k, o in enumerate(opts):
                        Xk = X[k * P:(k + 1) * P]
                        losses, amin = loss_function(Xk, True)
                        best_normalized[k] = Xk[amin].copy()
                        o.tell_population(Xk, losses)
                else:
                    losses, _ = loss_function(X, False)
                    for k, o in enumerate(opts):
                        o.tell_population(X[k * P:(k + 1) * P], losses[k * P:(k + 1) * P])
            best_values = [b * (upper - lower) + lower for b in best_normalized]
            # final error is always the mean distance (optimize.py:435-437), and float64 like the
            # reference's (and like LsqOptimizer's): a float32 point set of GCP size is evaluated once
            # more from a float64 copy; DSM-sized sets keep their float32 residency (a collective when
            # several ranks hold shards: every rank must reach this line).  One evaluation per start.
            f64_copy = pts.precision == _lib.ALP_F32 and pts.n <= self.F64_FINAL_MAX_POINTS
            with (self._device_points("f64") if f64_copy else nullcontext(pts)) as p:
                errs = [float(p.eval_population(self._candidate_matrix(v), _lib.LOSS_MEAN_DIST, 0.0)[0][0]) for v in best_values]
        finally:
            pts.close()
        self.start_results = [(s, self._result_params(v), e) for s, v, e in zip(seeds, best_values, errs)]
        b = best_start(errs)
        return self.start_results[b][1], self.start_results[b][2]

    F64_FINAL_MAX_POINTS = F64_MAX_POINTS


def _normal_lm_steps(x0, lower, upper, ftol, xtol, gtol, max_nfev):
    """``normal_lm`` as a state machine: a generator that yields the next trial point, receives ``(G, g, cost)`` there and
    returns (StopIteration.value) the result dict.  Between two yields it may raise the damping several times (failed solves
    need no evaluation)."""
    x = np.clip(np.asarray(x0, dtype=np.float64), lower, upper)
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    d = len(x)
    max_nfev = 100 * d if max_nfev is None else int(max_nfev)
    G, g, cost = yield x
    nfev, iterations, status = 1, 0, None

    def free_of(x, g):
        return ~(((x <= lower) & (g > 0)) | ((x >= upper) & (g < 0)))

    if not (np.isfinite(cost) and np.isfinite(G).all() and np.isfinite(g).all()):
        return dict(x=x, cost=float(cost), grad_norm=float("nan"), iterations=0, evaluations=1, status=-1)
    scale = np.sqrt(np.diag(G))
    mu, nu = 1e-3 * float(np.max(np.diag(G))), 2.0
    if not mu > 0:
        mu = 1e-3
    while True:
        free = free_of(x, g)
        g_norm = float(np.max(np.abs(g[free]))) if free.any() else 0.0
        if g_norm < gtol:
            status = 1
            break
        if nfev >= max_nfev:
            status = 0
            break
        scale = np.maximum(scale, np.sqrt(np.diag(G)))
        s2 = scale[free] ** 2
        top = float(np.max(scale ** 2))
        A = G[np.ix_(free, free)] + np.diag(mu * (s2 / top if top > 0 else np.ones_like(s2)))
        step = np.zeros(d)
        ok = False
        dA = np.diag(A)
        if (dA > 0).all():
            j = 1.0 / np.sqrt(dA)
            try:
                L = np.linalg.cholesky(A * np.outer(j, j))
                delta = -j * np.linalg.solve(L.T, np.linalg.solve(L, j * g[free]))
                ok = bool(np.isfinite(delta).all())
            except np.linalg.LinAlgError:
                ok = False
        predicted = -1.0
        if ok:
            step[free] = delta
            x_new = np.clip(x + step, lower, upper)
            step = x_new - x
            predicted = -(float(g @ step) + 0.5 * float(step @ G @ step))
        if not ok or not predicted > 0:
            # no usable step at this damping.  Once mu dwarfs G, the step is -g / mu scaled: when even that is below xtol, stop
            if ok and np.linalg.norm(step) < xtol * (xtol + np.linalg.norm(x)):
                status = 3
                break
            mu, nu = mu * nu, nu * 2.0
            if not np.isfinite(mu):
                status = 3
                break
            continue
        G_new, g_new, cost_new = yield x_new
        nfev += 1
        actual = cost - cost_new
        step_norm, x_norm = float(np.linalg.norm(step)), float(np.linalg.norm(x))
        accepted = bool(np.isfinite(cost_new) and np.isfinite(G_new).all() and np.isfinite(g_new).all() and cost_new < cost)
        ratio = actual / predicted if accepted else -1.0
        f_stop = accepted and actual < ftol * cost and ratio > 0.25
        x_stop = step_norm < xtol * (xtol + x_norm)
        if accepted:
            x, G, g, cost = x_new, G_new, g_new, float(cost_new)
            iterations += 1
            mu, nu = mu * max(1.0 / 3.0, 1.0 - (2.0 * ratio - 1.0) ** 3), 2.0
        else:
            mu, nu = mu * nu, nu * 2.0
        if f_stop or x_stop:
            status = 4 if (f_stop and x_stop) else (2 if f_stop else 3)
            break
    free = free_of(x, g)
    return dict(x=x, cost=float(cost), grad_norm=float(np.max(np.abs(g[free]))) if free.any() else 0.0,
                iterations=iterations, evaluations=nfev, status=status)




def normal_lm(fun, x0, lower, upper, ftol=1e-10, xtol=1e-10, gtol=1e-10, max_nfev=None):
    """Bounded Levenberg-Marquardt on the normal equations.  ``fun(x) -> (G, g, cost)``: G = J^T J (D, D), g = J^T r (D,),
    cost = the objective (0.5 r^T r for the linear loss), all at x -- ``Points.normal_equations`` on the device, or any
    oracle.  Minimises cost over lower <= x <= upper (either may be infinite).

    Damping (Nielsen): mu_0 = 1e-3 max diag G; an accepted step with gain ratio rho = actual / predicted reduction gives
    mu *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; a failed one mu *= nu, nu *= 2.  The damping matrix is
    mu diag(scale^2) / max(scale^2) with scale the running maximum of sqrt(diag G) (Marquardt's scaling, kept monotone).
    Solve: Cholesky of the damped matrix scaled to a unit diagonal; a factorisation that fails is a failed step.
    Bounds: a variable on a bound whose gradient pushes outward is left out of the solve for that iteration; the trial point
    is clipped into the box and the predicted reduction is that of the clipped step.
    A step is accepted only when the new cost is finite and smaller.
    Stopping, with scipy.optimize.least_squares' names and status codes: 1 ``gtol`` (the infinity norm of g over the free
    variables), 2 ``ftol`` (actual reduction < ftol * cost on a step with rho > 0.25), 3 ``xtol`` (|step| < xtol (xtol + |x|)),
    4 both, 0 ``max_nfev`` evaluations (default 100 D), -1 the cost at x0 is not finite.

    Returns a dict: x, cost, grad_norm, iterations (accepted steps), evaluations, status."""
    steps = _normal_lm_steps(x0, lower, upper, ftol, xtol, gtol, max_nfev)
    try:
        x = next(steps)
        while True:
            x = steps.send(fun(x))
    except StopIteration as stop:
        return stop.value


def normal_lm_batch(fun, X0, lower, upper, ftol=1e-10, xtol=1e-10, gtol=1e-10, max_nfev=None, indexed=False):
    """K runs of ``normal_lm`` in lockstep.  ``fun(X (k, D)) -> (G (k, D, D), g (k, D), cost (k,))``, row by row what
    ``normal_lm``'s ``fun`` returns -- ``Points.normal_equations_batch`` on the device.  ``X0`` (K, D): the starts; bounds,
    tolerances and ``max_nfev`` (per start) as for ``normal_lm``.  A round: every start that has not stopped advances to its
    next trial point, and all of them go to ``fun`` in one call, in start order; a start that has stopped drops out of the
    later calls.  Every start does the arithmetic of ``normal_lm`` run alone on its rows.  ``indexed=True``: ``fun`` is called
    as ``fun(X, starts)`` with the (k,) indices of the starts whose trial points the rows of X are -- for a ``fun`` whose
    problem differs from start to start (``Points.normal_equations_batch_rows``).  Returns the K result dicts in start
    order."""
    X0 = np.asarray(X0, dtype=np.float64)
    if X0.ndim != 2:
        raise ValueError("X0 must have shape (K, D)")
    runs = [_normal_lm_steps(x0, lower, upper, ftol, xtol, gtol, max_nfev) for x0 in X0]
    results = [None] * len(runs)
    pending = {k: next(run) for k, run in enumerate(runs)}        # the first yield needs no input and always comes
    while pending:
        order = sorted(pending)
        X = np.array([pending[k] for k in order], dtype=np.float64)
        G, g, cost = fun(X, np.array(order, dtype=np.int32)) if indexed else fun(X)
        for row, k in enumerate(order):
            try:
                pending[k] = runs[k].send((G[row], g[row], cost[row]))
            except StopIteration as stop:
                results[k] = stop.value
                del pending[k]
    return results


class LsqOptimizer(BaseOptimizer):
    """scipy.optimize.least_squares driver (reference optimize.py:442-539); the residual
    vector of every trial point comes from ``alp_residuals`` on a float64 point set, and with
    ``jac="analytic"`` its exact Jacobian from ``alp_jacobian``.  ``method="normal"`` solves on the normal equations the
    device forms (``alp_normal_equations``) instead, for point sets whose residual vector and Jacobian are too large to move.

    Several ranks (points sharded, one process per GPU): the reference solves ONE problem over all points
    (optimize.py:510-528), so every rank all-gathers the residual vector -- and the rows of the batched Jacobian -- of
    all shards, in rank order (``alp_comm_allgatherv``): contiguous shards concatenate to the single-process vector,
    every rank runs the identical scipy solve on it and gets the identical optimum."""

    def _residual_function(self):
        pts = self._device_points("f64")
        _, world = _lib.comm_info()
        sw = self._row_scale()

        def _residuals(values):
            r = pts.residuals(self._candidate_matrix(values)[0])
            if sw is not None:
                r = _scale_rows(r, sw)
            return _lib.comm_allgather(r) if world > 1 else r

        _residuals.points = pts
        return _residuals

    def _jacobian_function(self, pts, bounds=None):
        """2-point finite-difference Jacobian with scipy's own step rule (relative step
        sqrt(eps), sign-aware, flipped or shrunk at the bounds), but all D+1 residual vectors
        come from ONE ``alp_residuals_batch`` launch instead of D+1 sequential calls."""
        eps = np.finfo(np.float64).eps ** 0.5
        _, world = _lib.comm_info()
        lb = np.full(len(self.target_params), -np.inf) if bounds is None else np.asarray(bounds[0], dtype=np.float64)
        ub = np.full(len(self.target_params), np.inf) if bounds is None else np.asarray(bounds[1], dtype=np.float64)
        sw = self._row_scale()

        def _jac(values, *args, **kw):
            x0 = np.asarray(values, dtype=np.float64)
            h = eps * np.where(x0 >= 0, 1.0, -1.0) * np.maximum(1.0, np.abs(x0))
            lower_dist, upper_dist = x0 - lb, ub - x0
            x = x0 + h
            violated = (x < lb) | (x > ub)
            fitting = np.abs(h) <= np.maximum(lower_dist, upper_dist)
            h = np.where(violated & fitting, -h, h)
            h = np.where((upper_dist >= lower_dist) & ~fitting, upper_dist, h)
            h = np.where((upper_dist < lower_dist) & ~fitting, -lower_dist, h)
            d = len(x0)
            trial = np.tile(x0, (d + 1, 1))
            trial[np.arange(1, d + 1), np.arange(d)] += h
            dx = trial[np.arange(1, d + 1), np.arange(d)] - x0          # the representable step
            res = pts.residuals_batch(self._candidate_matrix(trial))
            jac = ((res[1:] - res[0]) / dx[:, None]).T               # (2 n_local, D): this rank's rows
            if sw is not None:
                jac = _scale_rows(jac, sw[:, None])
            return _lib.comm_allgather(np.ascontiguousarray(jac)) if world > 1 else jac

        return _jac

    def _analytic_jacobian_function(self, pts, cols):
        """The exact Jacobian of the residual vector at ``values`` (alp_jacobian): one launch, no step, nothing to do at a
        bound.  With several ranks the rows are all-gathered in rank order as in the batched path."""
        _, world = _lib.comm_info()
        sw = self._row_scale()

        def _jac(values, *args, **kw):
            jac = pts.jacobian(self._candidate_matrix(values)[0], cols, of_residuals=True)
            if sw is not None:
                jac = _scale_rows(jac, sw[:, None])
            return _lib.comm_allgather(jac) if world > 1 else jac

        return _jac

    MAX_STARTS = _lib.NORMAL_BATCH_MAX

    def _start_matrix(self, starts, seed, lower, upper):
        """the (K, D) starting points of optimize(method="normal", starts=...), clipped into the box as normal_lm clips x0;
        ValueError for K outside 1 .. MAX_STARTS, malformed starts, or an integer K with an infinite bound.  Host arithmetic."""
        d = len(self.target_params)
        if isinstance(starts, (bool, np.bool_)):
            raise ValueError("starts must be a positive integer, a list of parameter dicts or a (K, D) array")
        if isinstance(starts, (int, np.integer)):
            k = int(starts)
            if not 1 <= k <= self.MAX_STARTS:
                raise ValueError(f"starts must be 1 .. {self.MAX_STARTS}")
            if not (np.isfinite(lower).all() and np.isfinite(upper).all()):
                raise ValueError("starts=K draws the starts uniformly in the box: every bound must be finite")
            X0 = np.empty((k, d), dtype=np.float64)
            X0[0] = self.target_params_init
            X0[1:] = np.random.default_rng(seed).uniform(lower, upper, (k - 1, d))
        else:
            try:
                rows = starts if isinstance(starts, np.ndarray) else list(starts)
                if len(rows) and all(isinstance(r, dict) for r in rows):
                    for r in rows:
                        missing = [t for t in self.target_params if t not in r]
                        if missing:
                            raise ValueError(f"a start lacks the target parameters {missing}")
                    rows = [[r[t] for t in self.target_params] for r in rows]
                X0 = np.array(rows, dtype=np.float64)
            except TypeError:
                raise ValueError("starts must be a positive integer, a list of parameter dicts or a (K, D) array") from None
            if X0.ndim != 2 or X0.shape[1] != d or not np.isfinite(X0).all():
                raise ValueError(f"starts must hold K rows of {d} finite target values")
            if not 1 <= X0.shape[0] <= self.MAX_STARTS:
                raise ValueError(f"starts must be 1 .. {self.MAX_STARTS}")
        return np.ascontiguousarray(np.clip(X0, lower, upper))

    _RESULT_KEYS = ("cost", "iterations", "evaluations", "status", "grad_norm")

    @staticmethod
    def _check_every_check(device_loop, check_every):
        if device_loop and (isinstance(check_every, (bool, np.bool_)) or not isinstance(check_every, (int, np.integer)) or check_every < 1):
            raise ValueError("check_every must be a positive integer")

    def _device_runs(self, pts, cols, bounds, X0, loss, f_scale, ftol, xtol, gtol, max_nfev, check_every, weight_rows=False):
        """the K = len(X0) runs on the device (alp_lm_*; ``weight_rows``: run k under row k of the set's weight table) -> the K
        result dicts of normal_lm.  Every rank enqueues the same rounds on the same all-reduced sums and computes the same
        states; max_nfev stops every start, so the loop ends."""
        with _lib.LmDevice(pts, _lib.params_vector(self.params_init), cols, bounds[:, 0], bounds[:, 1], X0, loss, f_scale, ftol, xtol,
                           gtol, max_nfev, weight_rows=weight_rows) as loop:
            pending = len(X0)
            while pending:
                loop.run(int(check_every))
                pending = loop.wait()
            rec = loop.get()
        return [dict(x=rec["x"][k], cost=float(rec["cost"][k]), grad_norm=float(rec["grad_norm"][k]), iterations=int(rec["iterations"][k]),
                     evaluations=int(rec["evaluations"][k]), status=int(rec["status"][k])) for k in range(len(X0))]

    def _optimize_normal(self, bound_widths, loss, f_scale, ftol=1e-10, xtol=1e-10, gtol=1e-10, max_nfev=None, precision=None,
                         starts=None, seed=None, device_loop=False, check_every=8, **kwargs):
        """optimize(method="normal"); every refusal comes before the device is touched"""
        self._check_every_check(device_loop, check_every)
        if "jac" in kwargs:
            raise ValueError("method='normal' takes no jac=: it solves on J^T J and J^T r, no Jacobian exists in it")
        if kwargs:
            raise TypeError(f"method='normal' got unexpected keyword arguments {sorted(kwargs)}")
        if starts is None and seed is not None:
            raise TypeError("method='normal' takes seed= with starts=K alone")
        cols = _jacobian_targets(self.target_params)
        _lib.normal_loss_check(loss, f_scale)
        bounds = bounds_to_array(self.params_init, self.target_params, bound_widths)
        X0 = None if starts is None else self._start_matrix(starts, seed, bounds[:, 0], bounds[:, 1])
        single = X0 is None                  # decides the reporting alone: no "start" key, start_results not set
        if device_loop and single:           # the K = 1 case, from params_init (clipped on the device, as normal_lm clips x0)
            X0 = np.ascontiguousarray(np.asarray(self.target_params_init, dtype=np.float64)[None, :])
        pts = self._device_points(precision)
        try:
            _, world = _lib.comm_info()
            # rank 0's starts (its own draw when seed is None) are everybody's: the sums arrive all-reduced, so every rank then
            # runs the same iterations in lockstep
            if world > 1 and X0 is not None:
                _lib.comm_bcast(X0, root=0)
            if device_loop:
                runs = self._device_runs(pts, cols, bounds, X0, loss, f_scale, ftol, xtol, gtol, max_nfev, check_every)
            elif single:
                def sums(values):
                    return pts.normal_equations(self._candidate_matrix(values)[0], cols, loss, f_scale)[:3]

                runs = [normal_lm(sums, self.target_params_init, bounds[:, 0], bounds[:, 1], ftol=ftol, xtol=xtol, gtol=gtol,
                                  max_nfev=max_nfev)]
            else:                            # one alp_normal_equations_batch call per round
                def sums_batch(X):
                    return pts.normal_equations_batch(self._candidate_matrix(X), cols, loss, f_scale)[:3]

                runs = normal_lm_batch(sums_batch, X0, bounds[:, 0], bounds[:, 1], ftol=ftol, xtol=xtol, gtol=gtol, max_nfev=max_nfev)
            # rank 0's solutions are broadcast before the final errors, a collective over the shards, as for the other methods
            finals = np.ascontiguousarray([r["x"] for r in runs], dtype=np.float64)
            if world > 1:
                _lib.comm_bcast(finals, root=0)
            errs, _ = pts.eval_population(self._candidate_matrix(finals), _lib.LOSS_MEAN_DIST, 0.0, want_argmin=False)
        finally:
            pts.close()
        results = [(self._result_params(x), float(e), {k: r[k] for k in self._RESULT_KEYS}) for x, e, r in zip(finals, errs, runs)]
        if single:
            self.result_ = results[0][2]
            return results[0][0], results[0][1]
        self.start_results = results
        b = best_start([r["cost"] for r in runs])
        self.result_ = dict(results[b][2], start=b)
        return results[b][0], results[b][1]

    # -- K fits under K weight rows: cross-validation and bootstrap ---------------------------
    def _resample_checks(self, loss, f_scale, device_loop, check_every):
        """the refusals cross_validate and bootstrap share with optimize(method="normal"): host arithmetic"""
        self._check_every_check(device_loop, check_every)
        _lib.normal_loss_check(loss, f_scale)
        return _jacobian_targets(self.target_params)

    def _shard(self, world, seed):
        """(lo, hi, n_global, seed): this rank's columns [lo, hi) of the global index range -- the shards lie in rank order,
        their sizes come from one comm_allgather -- and the seed every rank uses: rank 0's (its own entropy for None)"""
        n = len(self.obj_points)
        if world == 1:
            return 0, n, n, seed
        rank, _ = _lib.comm_info()
        sizes = _lib.comm_allgather(np.array([n], dtype=np.int64))
        s = np.array([np.random.SeedSequence().entropy % (1 << 63) if seed is None else int(seed)], dtype=np.uint64)
        _lib.comm_bcast(s, root=0)
        lo = int(sizes[:rank].sum())
        return lo, lo + n, int(sizes.sum()), int(s[0])

    def _global_weights(self, lo, hi, n_global):
        """(n_global,) float64: the constructor's weights (ones without) in this rank's columns, zeros elsewhere"""
        w = np.zeros(n_global, dtype=np.float64)
        w[lo:hi] = 1.0 if self.weights is None else self.weights
        return w

    def _fit_rows(self, pts, table, cols, bounds, world, loss, f_scale, ftol, xtol, gtol, max_nfev, device_loop, check_every):
        """K = len(table) fits from params_init in one lockstep, fit b under row b of ``table`` (uploaded here as the set's
        weight table) -> (the K result dicts of normal_lm, finals (K, D)).  The host lockstep (normal_lm_batch on
        Points.normal_equations_batch_rows) or, ``device_loop``, LmDevice(weight_rows=True)."""
        K = len(table)
        pts.set_weight_table(table)
        X0 = np.ascontiguousarray(np.tile(np.clip(np.asarray(self.target_params_init, dtype=np.float64), bounds[:, 0], bounds[:, 1]), (K, 1)))
        if device_loop:
            runs = self._device_runs(pts, cols, bounds, X0, loss, f_scale, ftol, xtol, gtol, max_nfev, check_every, weight_rows=True)
        else:
            def sums_rows(X, starts):
                return pts.normal_equations_batch_rows(self._candidate_matrix(X), starts, cols, loss, f_scale)[:3]

            runs = normal_lm_batch(sums_rows, X0, bounds[:, 0], bounds[:, 1], ftol=ftol, xtol=xtol, gtol=gtol, max_nfev=max_nfev, indexed=True)
        finals = np.ascontiguousarray([r["x"] for r in runs], dtype=np.float64)
        if world > 1:
            _lib.comm_bcast(finals, root=0)
        return runs, finals

    def cross_validate(self, folds=5, seed=None, bound_widths=None, loss="linear", f_scale=1.0, ftol=1e-10, xtol=1e-10, gtol=1e-10,
                       max_nfev=None, precision=None, device_loop=False, check_every=8):
        """k-fold cross-validation of the ``method="normal"`` fit: how large is the reprojection error on points the fit has
        not seen -- the held-out check-point accuracy -- and which point disagrees with the model fitted without it.

        ``folds``: an integer k (2 <= k <= min(N, 1024): a permutation from ``np.random.default_rng(seed)`` dealt round-robin,
        fold sizes differ by at most 1), ``"loo"`` (every point its own fold, at most 1024 points) or N explicit integer
        labels (``resample.fold_labels``; with several ranks the labels of ALL points, in rank order).  The k fits start
        from ``params_init`` and run in ONE lockstep: fit b sees the weights ``w_i [label_i != b]`` as row b of a weight
        table on the device (``Points.set_weight_table``), and every round is one alp_normal_equations_batch_rows launch
        over the folds that have not stopped -- or, ``device_loop=True``, the device loop of optimize(method="normal") with a
        row per start.  The points are uploaded once.  Then one more such launch at the k optima under the held-out rows
        ``w_i [label_i == b]`` with the linear loss gives every fold's held-out error, and one alp_residuals_assigned launch
        every point's residual under the parameters fitted WITHOUT its fold.  ``bound_widths``, ``loss`` / ``f_scale``, the
        tolerances, ``max_nfev``, ``precision``, ``device_loop`` and ``check_every`` as for optimize(method="normal"); the
        constructor's ``weights`` multiply both tables.

        Returns -- and keeps as ``self.cv_`` -- a dict: ``labels`` (N,) of this rank's points; ``fold_params`` (k parameter
        dicts); ``fold_results`` (k dicts: cost, iterations, evaluations, status, grad_norm of the training fit, as in
        ``start_results``); ``fold_rmse`` (k,): sqrt(sum w_i d_i^2 / sum w_i) over fold b's own points under fit b, from the
        device's sums as sqrt(2 cost_b / W_b); ``rmse``: the same pooled over all points, sqrt(sum_b 2 cost_b / sum_b W_b);
        ``residuals`` (N, 2) and ``distance`` (N,): the held-out residual pair (observed - projected) and its length for
        this rank's points.  With several ranks the sums arrive all-reduced and rank 0's seed is everybody's.

        ValueError, before the device is touched (with several ranks: before anything but the exchange of the shard sizes),
        for ``folds`` out of range, a table above ``resample.WEIGHT_TABLE_MAX_BYTES``, targets w / h, an unknown loss, and
        -- without a communicator -- a fold whose training weights are all zero."""
        cols = self._resample_checks(loss, f_scale, device_loop, check_every)
        bounds = bounds_to_array(self.params_init, self.target_params, bound_widths)
        world = _lib.comm_world()
        lo, hi, n_global, seed = self._shard(world, seed)
        labels = resample.fold_labels(n_global, folds, seed)
        k = int(labels.max()) + 1
        precision = default_precision(hi - lo, precision)
        resample.table_check(k, hi - lo, 4 if precision == "f32" else 8)                   # before the tables exist: they are O(k N)
        train, held = resample.fold_tables(labels, self._global_weights(lo, hi, n_global), lo, hi)
        resample.table_check(k, hi - lo, 4 if precision == "f32" else 8, train.sum(axis=1) if world == 1 else None)
        pts = self._device_points(precision)
        try:
            runs, finals = self._fit_rows(pts, train, cols, bounds, world, loss, f_scale, ftol, xtol, gtol, max_nfev, device_loop, check_every)
            cand = self._candidate_matrix(finals)
            pts.set_weight_table(held)
            _, _, cost, W = pts.normal_equations_batch_rows(cand, np.arange(k, dtype=np.int32), cols, "linear", 1.0)
            res = pts.residuals_assigned(cand, labels[lo:hi]).reshape(-1, 2)
        finally:
            pts.close()
        with np.errstate(invalid="ignore", divide="ignore"):
            fold_rmse = np.sqrt(2.0 * cost / W)
            pooled = float(np.sqrt(2.0 * cost.sum() / W.sum()))
        self.cv_ = dict(labels=labels[lo:hi].copy(), fold_params=[self._result_params(x) for x in finals],
                        fold_results=[{key: r[key] for key in self._RESULT_KEYS} for r in runs], fold_rmse=fold_rmse, rmse=pooled,
                        residuals=res, distance=np.hypot(res[:, 0], res[:, 1]))
        return self.cv_

    def bootstrap(self, n_boot=200, seed=None, bound_widths=None, loss="linear", f_scale=1.0, ftol=1e-10, xtol=1e-10, gtol=1e-10,
                  max_nfev=None, precision=None, device_loop=False, check_every=8):
        """Bootstrap of the ``method="normal"`` fit: how uncertain are the fitted parameters -- the answer that, unlike the
        linearised ``parameter_covariance``, survives a robust loss and active bounds.

        ``n_boot`` (1 .. 1024) resamples of the N points, N draws with replacement each from ONE
        ``np.random.default_rng(seed)`` (``resample.bootstrap_table``); resample b is fitted from ``params_init`` under the
        weights ``count_b[i] w_i`` -- row b of a weight table on the device -- and all fits run in ONE lockstep, as in
        ``cross_validate`` (same arguments, same two loops).  The points are uploaded once.

        Returns -- and keeps as ``self.boot_`` -- a dict: ``samples`` (n_boot, D): the fitted values in ``target_params``
        order; ``results`` (n_boot dicts: cost, iterations, evaluations, status, grad_norm); ``counts`` (n_boot, N): how often
        each of this rank's points was drawn; ``kept`` (n_boot,) bool: the fits with status > 0 and a finite cost, over which
        the statistics run; ``dropped``: how many were left out; ``mean`` (D,), ``std`` (D,; ddof = 1) and ``cov`` (D, D;
        ``np.cov``) of the kept samples (NaN with fewer than two); ``interval``: a function, ``interval(level=0.95)`` ->
        (lower (D,), upper (D,)), the percentiles 50 (1 -+ level) of the kept samples.

        ValueError, before the device is touched, for ``n_boot`` out of range, a table above
        ``resample.WEIGHT_TABLE_MAX_BYTES``, targets w / h, an unknown loss, and -- without a communicator -- a resample
        whose weights are all zero (every point it drew has weight 0)."""
        cols = self._resample_checks(loss, f_scale, device_loop, check_every)
        bounds = bounds_to_array(self.params_init, self.target_params, bound_widths)
        world = _lib.comm_world()
        lo, hi, n_global, seed = self._shard(world, seed)
        precision = default_precision(hi - lo, precision)
        if isinstance(n_boot, (int, np.integer)) and not isinstance(n_boot, (bool, np.bool_)):
            resample.table_check(n_boot, hi - lo, 4 if precision == "f32" else 8)        # before the draws: they are O(n_boot N)
        counts = resample.bootstrap_table(n_global, n_boot, seed, None, lo, hi)
        table = counts if self.weights is None else counts * self.weights[None, :]
        resample.table_check(len(table), hi - lo, 4 if precision == "f32" else 8, table.sum(axis=1) if world == 1 else None)
        pts = self._device_points(precision)
        try:
            runs, finals = self._fit_rows(pts, table, cols, bounds, world, loss, f_scale, ftol, xtol, gtol, max_nfev, device_loop, check_every)
        finally:
            pts.close()
        kept = np.array([r["status"] > 0 and bool(np.isfinite(r["cost"])) for r in runs], dtype=bool)
        good = finals[kept]
        d = finals.shape[1]
        if len(good) >= 2:
            mean, std, cov = good.mean(axis=0), good.std(axis=0, ddof=1), np.atleast_2d(np.cov(good, rowvar=False))
        else:
            mean = good.mean(axis=0) if len(good) else np.full(d, np.nan)
            std, cov = np.full(d, np.nan), np.full((d, d), np.nan)

        def interval(level=0.95):
            if not 0 < level < 1:
                raise ValueError("level must lie in (0, 1)")
            if not len(good):
                return np.full(d, np.nan), np.full(d, np.nan)
            q = np.percentile(good, [50.0 * (1.0 - level), 50.0 * (1.0 + level)], axis=0)
            return q[0], q[1]

        self.boot_ = dict(samples=finals, results=[{key: r[key] for key in self._RESULT_KEYS} for r in runs], counts=counts, kept=kept,
                          dropped=int((~kept).sum()), mean=mean, std=std, cov=cov, interval=interval)
        return self.boot_

    def optimize(self, method="trf", bound_widths=None, loss="linear", f_scale=1.0, **kwargs):
        """scipy.optimize.least_squares on the device residuals.  ``jac``: "batched" (the default for trf and dogbox: 2-point
        differences, D + 1 trial points per launch), "analytic" (the exact Jacobian, alp_jacobian; targets w / h refused),
        anything scipy accepts (for lm the default stays MINPACK's own differences).

        ``method="normal"``: a bounded Levenberg-Marquardt (``normal_lm``) on J^T J, J^T r and the cost, which the device forms
        in one kernel per trial point (alp_normal_equations): no residual vector and no Jacobian reaches the host, and with
        several ranks the sums arrive all-reduced -- nothing is gathered.  ``loss`` / ``f_scale`` as for scipy (linear,
        soft_l1, huber, cauchy); bounds as for trf (``bound_widths=None``: the default widths; a width of inf leaves a target
        unbounded); ``ftol``, ``xtol``, ``gtol`` (1e-10 each) and ``max_nfev`` with scipy's meaning; ``precision`` as for
        CMAOptimizer (None: float64 up to F64_MAX_POINTS points, float32 above).  ``jac=`` is refused (there is no Jacobian in
        this method), and so are targets w / h.  ``self.result_``: cost, iterations, evaluations, status, grad_norm.

        ``method="normal", starts=...``: K runs of that iteration in lockstep (``normal_lm_batch``), the trial points of all
        runs that have not stopped evaluated by ONE alp_normal_equations_batch launch per round -- at GCP size a single trial
        point leaves the device almost empty.  ``starts`` is a list of parameter dicts (``[r[1] for r in cma.start_results]``
        polishes the K optima ``CMAOptimizer.optimize(starts=K)`` leaves) or a (K, D) array of target values: explicit starts,
        clipped into the box, which stays centred on ``params_init``; or an integer K: start 0 is ``params_init`` and starts
        1 .. K-1 are drawn uniformly in the box from ``np.random.default_rng(seed)`` (every bound must be finite; ``seed=None``
        draws fresh entropy; with a communicator rank 0's starts are broadcast).  1 <= K <= 1024; ``max_nfev`` counts per
        start.  Returns the ``(params, error)`` of the start with the smallest final cost (``best_start``'s rule);
        ``self.result_`` is that start's record plus ``"start"``, its index; ``self.start_results``: the
        ``(params, error, result)`` of every start in start order.  ``starts=`` with another method is refused.

        ``method="normal", device_loop=True`` (opt-in; ``check_every=8``): the K runs keep their state on the device
        (alp_lm_*): a round -- the evaluation of the running starts' trial points, the state-machine step of every start with
        its Cholesky solve, the plan of the next trial point, the list of the starts that still run -- is four launches
        enqueued with no copy and no synchronisation; the host looks every ``check_every`` rounds (8 bytes come back) until
        no start runs, then fetches the K records once.  Without ``starts=`` it is the K = 1 case from ``params_init`` and
        ``result_`` has no ``"start"``.  Results and attributes as above.  A device run's trajectory is NOT the host run's: the
        device's sines and cosines in the plan and its Cholesky round differently from libm and LAPACK; near convergence
        ``cost_new < cost`` is decided at rounding level, so evaluation counts and the status among 2 / 3 / 4 may differ; and
        the host lockstep shrinks its batch as starts stop, which changes the stripes of the sums above 256 points, while
        the device loop keeps K's.  What is held instead: the state machine to ``_normal_lm_steps`` on shared sums, the sums
        to ``alp_normal_equations_batch``, the end result to the cost and the optimum.  At most 23 targets, not w / h;
        ``device_loop`` with another method and a ``check_every`` that is no positive integer are refused.

        ``weights=`` of the constructor: ``method="normal"`` weights on the device, for all four losses (both rows of point i
        count w_i times); trf, dogbox and lm get residuals and Jacobian rows scaled by sqrt(w_i) on the host (0 where w_i = 0),
        which is that problem for ``loss="linear"``; a robust loss with weights is refused there."""
        if method == "normal":
            return self._optimize_normal(bound_widths, loss, f_scale, **kwargs)
        if kwargs.get("device_loop"):
            raise ValueError("device_loop=True belongs to method='normal' (CMAOptimizer.optimize has its own)")
        if "device_loop" in kwargs:          # device_loop=False: the default, said aloud
            kwargs = {k: v for k, v in kwargs.items() if k not in ("device_loop", "check_every")}
        if "starts" in kwargs:
            raise ValueError("starts= belongs to method='normal' (CMAOptimizer.optimize has its own)")
        analytic = kwargs.get("jac") == "analytic"
        cols = _jacobian_targets(self.target_params) if analytic else None
        if method == "lm" and bound_widths is not None:
            raise ValueError("method='lm' does not support bounds. Set bound_widths=None or use 'trf'/'dogbox'.")
        if method == "lm" and loss != "linear":
            raise ValueError("method='lm' does not support robust loss functions. Use loss='linear' or method='trf'/'dogbox'.")
        if self.weights is not None and loss != "linear":
            # scipy applies rho to the scaled residual, rho(w r^2): another problem than w rho(r^2), the duplicated rows'
            raise ValueError("weights with a robust loss need method='normal' (it weights rho itself); "
                             f"method='{method}' scales the residuals by sqrt(w), which is the weighted problem for loss='linear' alone")

        residual_func = self._residual_function()
        pts = residual_func.points
        try:
            if method == "lm":
                # MINPACK's own forward differences unless the caller asks for the batched ones
                if kwargs.get("jac") == "batched":
                    kwargs = dict(kwargs, jac=self._jacobian_function(pts))
                elif analytic:
                    kwargs = dict(kwargs, jac=self._analytic_jacobian_function(pts, cols))
                result = least_squares(residual_func, self.target_params_init, method=method, **kwargs)
            else:
                bounds = bounds_to_array(self.params_init, self.target_params, bound_widths)
                if kwargs.get("jac", "batched") == "batched":
                    kwargs = dict(kwargs, jac=self._jacobian_function(pts, (bounds[:, 0], bounds[:, 1])))
                elif analytic:
                    kwargs = dict(kwargs, jac=self._analytic_jacobian_function(pts, cols))
                result = least_squares(residual_func, self.target_params_init, method=method,
                                       bounds=(bounds[:, 0], bounds[:, 1]), loss=loss,
                                       f_scale=f_scale, **kwargs)
            # With a communicator every rank has solved the SAME gathered problem; the final error below is a collective
            # over the shards and must be evaluated for one solution on all of them: rank 0's is broadcast (bit-identical
            # to the others' on identical hosts; the broadcast makes it so on any).
            best = np.ascontiguousarray(result.x, dtype=np.float64)
            _, world = _lib.comm_info()
            if world > 1:
                _lib.comm_bcast(best, root=0)
            params = self._result_params(best)
            err, _ = pts.eval_population(self._candidate_matrix(best), _lib.LOSS_MEAN_DIST, 0.0)
        finally:
            pts.close()
        return params, float(err[0])
