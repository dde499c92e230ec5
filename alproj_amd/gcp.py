"""Drop-in counterpart of the functions of the reference module ``alproj.gcp`` that sit between the
render and the optimiser:

* ``set_gcp``              src/alproj/gcp.py:614-648
* ``filter_gcp_distance``  src/alproj/gcp.py:651-726

and of the arithmetic core of its two built-in matchers (``_opencv_match``, src/alproj/gcp.py:52-70):
the brute-force 2-nearest-neighbour search of every photograph descriptor against every
simulated-image descriptor (``cv2.BFMatcher().knnMatch(des1, des2, k=2)``, L2 norm for AKAZE's bytes
too) and Lowe's ratio test:

* ``knn_match``          the two nearest train rows of every query row and their distances
* ``match_descriptors``  the (query, train) index pairs that pass the ratio test
* ``match_keypoints``    lines 52-70 as a whole: descriptors + keypoint coordinates -> pts1, pts2

AKAZE descriptors are bytes and OpenCV's SIFT descriptors are float32 holding the integers 0..255,
so the squared distances are exact integers formed on the int8 matrix cores (``alp_match_knn2``).

The two steps that ``image_match`` runs on every set of matches before it returns (src/alproj/gcp.py:507-544):

* ``filter_geometric``   ``_filter_geometric`` with ``outlier_filter="fundamental"`` (gcp.py:254-273): H fundamental
                         matrices from 8-point samples, each scored on all matches, the best one refitted
                         (``alp_epipolar_ransac``); and with ``outlier_filter="essential"`` (gcp.py:200-252) given a focal
                         length: up to 10 essential matrices from each of H 5-point samples (Nister's solver), scored
                         and chosen the same way in pixel coordinates, the refit projected onto the essential matrices
                         (``alp_essential_ransac``).  The inlier set is NOT cv2's: cv2's random stream and MAGSAC
                         scoring cannot be restated, so the algorithm is this project's own, plain inlier counting
                         with the error measure of cv2's classic ``FM_RANSAC``; ``ransac_method="LMEDS"`` (gcp.py:160-161)
                         replaces the fixed threshold by least median of squares over the same hypotheses: the r-th
                         smallest error of every hypothesis by an exact radix select on the device
                         (``alp_epipolar_lmeds`` / ``alp_essential_lmeds``), the bound from the smallest one;
                         ``filter_matches`` forwards it with its ``**ransac``
* ``filter_spatial``     ``_filter_spatial`` (gcp.py:282-357), bit for bit (``alp_grid_thin``)
* ``filter_matches``     lines 507-544 as a whole: points -> the DataFrame u_org, v_org, u_sim, v_sim

Detection (``detectAndCompute``), the essential-matrix filter's guess of a focal length that nobody
gave it (gcp.py:206-220), cv2's USAC / MAGSAC scoring and the learned matchers behind
``vismatch`` stay with the reference: cv2 is neither imported nor needed here.  ``set_gcp`` accepts, besides the reference's
``reverse_proj`` DataFrame, the device-resident ``alproj_amd.project.ReverseProjection``: the
(u_sim, v_sim) -> (x, y, z) join then becomes one gather from the coordinate image in HBM
(``alp_render_gather``) and the multi-million-row table is never built.
"""
import math

import numpy as np
import pandas as pd

from . import _lib
from .project import ReverseProjection

__all__ = ["set_gcp", "filter_gcp_distance", "knn_match", "match_descriptors", "match_keypoints", "filter_geometric",
           "filter_spatial", "filter_matches"]


def set_gcp(match, rev_proj):
    """Add geographic coordinates to matched point pairs (reference gcp.py:614-648).

    match : DataFrame with u_org, v_org, u_sim, v_sim (result of image_match).
    rev_proj : DataFrame of ``reverse_proj`` -- or a ``ReverseProjection`` on the device.

    Returns a DataFrame u, v, x, y, z: the matches whose simulated-image pixel sees the surface
    (left join on (u_sim, v_sim) = (u, v), rows with any NaN dropped, labels of the join kept)."""
    if isinstance(rev_proj, ReverseProjection):
        xyz = rev_proj.lookup(match["u_sim"].to_numpy(), match["v_sim"].to_numpy())
        gcp = pd.DataFrame({"u": match["u_org"].to_numpy(), "v": match["v_org"].to_numpy(),
                            "x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2]})
    else:
        gcp = pd.merge(match, rev_proj, how="left", left_on=["u_sim", "v_sim"], right_on=["u", "v"])
        gcp = gcp[["u_org", "v_org", "x", "y", "z"]].rename(columns={"u_org": "u", "v_org": "v"})
    return gcp.dropna(how="any", axis=0)


def filter_gcp_distance(gcp, params, min_distance=None, max_distance=None):
    """Keep the GCPs whose 3-D distance from the camera position lies in
    [min_distance, max_distance] (reference gcp.py:651-726): same validation and messages, rows
    with NaN coordinates dropped, index reset; a copy when there is nothing to filter.  The mask is
    formed on the device (``alp_distance_mask``), next to the gather that made the coordinates."""
    for key in ("x", "y", "z"):
        if key not in params:
            raise KeyError(f"params must contain '{key}' key")
    if min_distance is not None and min_distance < 0:
        raise ValueError("min_distance must be non-negative")
    if min_distance is not None and max_distance is not None and max_distance < min_distance:
        raise ValueError("max_distance must be >= min_distance")
    if len(gcp) == 0 or (min_distance is None and max_distance is None):
        return gcp.copy()
    xyz = np.column_stack([gcp["x"].to_numpy(dtype=np.float64), gcp["y"].to_numpy(dtype=np.float64),
                           gcp["z"].to_numpy(dtype=np.float64)])
    keep = _lib.distance_mask(xyz, [params["x"], params["y"], params["z"]], min_distance, max_distance)
    return gcp[keep].reset_index(drop=True)


def knn_match(des1, des2):
    """``cv2.BFMatcher().knnMatch(des1, des2, k=2)`` as arrays (reference gcp.py:55-56): for every row of ``des1`` the two nearest
    rows of ``des2`` by L2 distance, the lower index first on a tie.

    des1, des2 : C-contiguous (N1, L) and (N2, L) arrays, both uint8 or both float32 holding the integers 0..255; N2 >= 2.
    Returns (idx (N1, 2) int32, dist (N1, 2) float32): ``DMatch.trainIdx`` and ``DMatch.distance`` of the pair."""
    r = _lib.match_knn2(des1, des2)
    return r["idx"], r["dist"]


def match_descriptors(des1, des2, ratio=0.7):
    """The matches that pass Lowe's ratio test (reference gcp.py:55-64), in query order.

    Returns (query_idx, train_idx), int32: ``m.queryIdx`` and ``m.trainIdx`` of the reference's ``good`` list."""
    r = _lib.match_knn2(des1, des2, ratio)
    query_idx = np.flatnonzero(r["good"]).astype(np.int32)
    return query_idx, r["idx"][query_idx, 0]


def _no_points():
    return np.array([]).reshape(0, 2).astype("int32"), np.array([]).reshape(0, 2).astype("int32")


def match_keypoints(pts_org, des_org, pts_sim, des_sim, ratio=0.7):
    """``_opencv_match`` from its line 52 on (reference gcp.py:52-70), given what ``detectAndCompute`` returned for the photograph
    and for the simulated image.

    pts_org, pts_sim : (N, 2) arrays of ``kp.pt``; des_org, des_sim : the descriptors (or None, as cv2 returns for no keypoint).
    Returns (pts1, pts2): int32 (N, 2) pixel coordinates of the matches that pass the ratio test, in query order, the
    coordinates through ``np.float32(...).astype("int32")`` as in lines 69-70; empty (0, 2) arrays when either side has
    fewer than 2 keypoints or nothing passes."""
    if des_org is None or des_sim is None or len(pts_org) < 2 or len(pts_sim) < 2:
        return _no_points()
    pts_org, pts_sim = np.asarray(pts_org), np.asarray(pts_sim)
    for pts, des in ((pts_org, des_org), (pts_sim, des_sim)):
        if pts.ndim != 2 or pts.shape[1] != 2 or not isinstance(des, np.ndarray) or des.ndim != 2 or pts.shape[0] != des.shape[0]:
            raise ValueError("keypoint coordinates must be (N, 2) with one row per descriptor")
    query_idx, train_idx = match_descriptors(des_org, des_sim, ratio)
    if len(query_idx) == 0:
        return _no_points()
    return np.float32(pts_org[query_idx]).astype("int32"), np.float32(pts_sim[train_idx]).astype("int32")


RANSAC_METHODS = ("RANSAC", "LMEDS")


def filter_geometric(pts1, pts2, method="fundamental", threshold=10.0, hypotheses=16384, seed=0, refits=4, samples=None,
                     return_model=False, focal_length=None, principal_point=None, image_size=None, *, ransac_method="RANSAC",
                     quantile=0.5, min_threshold=1.0):
    """``_filter_geometric`` (reference gcp.py:160-279) for ``method="fundamental"`` and ``method="essential"``, on the device: a
    bool mask of the matches that agree with one fundamental or essential matrix.

    ``"fundamental"``: ``hypotheses`` 8-point samples are drawn from ``seed`` (or taken from ``samples``, (H, 8) indices), each
    solved by the normalised 8-point algorithm and scored by its number of matches whose larger squared point-to-epipolar-line
    distance is at most ``threshold``^2 (cv2's classic ``FM_RANSAC`` measure); the best one is refitted on its inliers up to
    ``refits`` times while that strictly grows the count.  The inlier set is not cv2's: another sampler, and plain counting
    instead of MAGSAC.

    ``"essential"``: the samples hold 5 matches (``samples``: (H, 5)), each solved by the five-point algorithm in coordinates
    normalised by K = (``focal_length``, ``principal_point``), one K for both images as the reference builds it (gcp.py:232-236).
    Each of the up to 10 essential matrices of a sample is scored as the pixel-space matrix K^-T E K^-1 with the same measure
    and the same ``threshold`` in pixels; the refit is projected onto the essential matrices.  ``principal_point`` missing:
    half of ``image_size``, else the midpoint of the bounding box of ``pts1`` (gcp.py:223-229).  ``focal_length`` missing:
    ``NotImplementedError``: the reference's guess "focal length = image width" (gcp.py:206-220) stays with the reference,
    because a filter that is preferred for its use of the intrinsics should not invent them.

    The default ``hypotheses = 16384`` is what confidence 0.999 needs for 8-point samples down to an inlier share w of about
    0.38: H = log(1 - 0.999) / log(1 - w^8), about 16 000 at w = 0.38 (3 100 at w = 0.5, 118 at w = 0.7); for 5-point samples
    it reaches down to w of about 0.21 (2 800 samples at w = 0.3).  The device evaluates all of them outright, so nothing is
    saved by stopping early; the essential filter scores ten slots per sample.

    The edge cases are the reference's (gcp.py:189-203, 254-257, 275-279): an empty input gives an empty bool array, ``"none"``
    all True, fewer than 8 points (``"essential"``: 5) all True, an unknown method the reference's ``ValueError``; fewer than 8
    (5) inliers anywhere give all True as well (cv2 returning no mask, gcp.py:249-250, 270-271).

    ``ransac_method`` (keyword only, case-insensitive; reference gcp.py:160-161, 239-245, 260-266): ``"RANSAC"``, the default, is
    the inlier counting at ``threshold`` described above.  ``"LMEDS"`` is least median of squares, which needs no threshold and
    ignores ``threshold`` as cv2 does: the value of a hypothesis is the r-th smallest error over all n matches, r = min(n,
    max(m + 1, ceil(quantile * n))) with m = 8 (5) the size of a minimal sample (below n = 2 (m + 1) that is m + 1 whatever the
    quantile); the hypothesis with the smallest value v is chosen (the lowest index on a tie), a match is an inlier iff its
    error is at most b^2 = max(scale^2 * v, min_threshold^2) with scale = 2.5 * (1 / Phi^-1((1 + quantile) / 2)) * (1 + 5 / (n -
    m)) (Rousseeuw and Leroy's robust standard deviation, 1.4826 at the median), and the refit on the inliers is kept while it
    strictly lowers the value (``alp_epipolar_lmeds`` / ``alp_essential_lmeds``; not cv2's LMedS either).  ``quantile`` in
    (0, 1]: below the inlier share when more than half of the matches are outliers.  ``min_threshold`` (pixels, finite, >= 0):
    the floor of the bound, 1 px by default because ``astype("int32")`` (gcp.py:69-70) moves every coordinate by up to a pixel.
    With n <= m every match is kept before any device call; a smallest value that is not finite keeps every match.
    ``"USAC_MAGSAC"`` and ``"USAC_DEFAULT"`` raise ``NotImplementedError`` (cv2's scoring cannot be restated), anything else
    ``ValueError``: the reference's silent fall-back to MAGSAC is not repeated.

    ``return_model=True`` returns (mask, F, info): F (3, 3) in pixel coordinates with b^T F a = 0 for a = (x1, y1, 1),
    b = (x2, y2, 1), or None when no model was fitted, and the info dict of ``_lib.epipolar_ransac``; for ``"essential"`` info
    also holds ``"E"`` = K^T F K and ``chosen`` counts slots, sample * 10 + slot.  With ``"LMEDS"`` info is that of
    ``_lib.epipolar_lmeds`` and also holds ``method``, ``rank``, ``value``, ``final_value``, ``bound`` (pixels) and
    ``refit_values``."""
    pts1 = np.asarray(pts1, dtype=np.float64)
    pts2 = np.asarray(pts2, dtype=np.float64)

    def result(mask, F=None, info=None):
        return (mask, F, info or {}) if return_model else mask

    if len(pts1) == 0:
        return result(np.array([], dtype=bool))
    method_lower = method.lower()
    if method_lower == "none":
        return result(np.ones(len(pts1), dtype=bool))
    if method_lower not in ("essential", "fundamental"):
        raise ValueError(
            f"Unknown outlier_filter '{method}'. "
            "Available: 'essential', 'fundamental', 'none'"
        )
    essential = method_lower == "essential"
    ransac_upper = str(ransac_method).upper()
    if ransac_upper in ("USAC_MAGSAC", "USAC_DEFAULT"):
        raise NotImplementedError(f"ransac_method='{ransac_method}': cv2's USAC / MAGSAC scoring cannot be restated and stays with the "
                                  "reference; available here: 'RANSAC', 'LMEDS'")
    if ransac_upper not in RANSAC_METHODS:
        raise ValueError(f"Unknown ransac_method '{ransac_method}'. Available: 'RANSAC', 'LMEDS'")
    lmeds = ransac_upper == "LMEDS"
    m = 5 if essential else 8
    if lmeds:
        if not (isinstance(quantile, (int, float)) and 0.0 < quantile <= 1.0):
            raise ValueError("quantile must lie in (0, 1]")
        if not (np.isfinite(min_threshold) and min_threshold >= 0):
            raise ValueError("min_threshold must be finite and not negative")
    if len(pts1) < m or (lmeds and len(pts1) <= m):
        return result(np.ones(len(pts1), dtype=bool))
    if essential and focal_length is None:
        raise NotImplementedError("outlier_filter='essential' without a focal length: the guess 'focal length = image width' stays "
                                  "with the reference; pass focal_length (filter_matches: params with 'fov' and 'w'), or use "
                                  "'fundamental' or 'none'")
    if pts1.ndim != 2 or pts1.shape[1] != 2 or pts1.shape != pts2.shape:
        raise ValueError(f"points must be two (n, 2) arrays of one length, not {pts1.shape} and {pts2.shape}")
    if not (np.isfinite(pts1).all() and np.isfinite(pts2).all()):
        raise ValueError("point coordinates must be finite")
    if not (np.isfinite(threshold) and threshold >= 0):
        raise ValueError("threshold must be finite and not negative")
    if samples is None and int(hypotheses) < 1:
        raise ValueError("hypotheses must be at least 1")
    if not 0 <= int(refits) <= _lib.EPI_MAX_REFITS:
        raise ValueError(f"refits must be 0..{_lib.EPI_MAX_REFITS}")
    if lmeds:
        rank = _lib.lmeds_rank(len(pts1), m, quantile)
        criterion = (rank, _lib.lmeds_scale2(len(pts1), m, quantile), float(min_threshold) * float(min_threshold))
    else:
        criterion = (threshold,)
    camera = ()
    if essential:
        if principal_point is None:
            # reference gcp.py:223-229, verbatim
            if image_size is not None:
                principal_point = (image_size[0] / 2, image_size[1] / 2)
            else:
                cx = (pts1[:, 0].max() + pts1[:, 0].min()) / 2
                cy = (pts1[:, 1].max() + pts1[:, 1].min()) / 2
                principal_point = (cx, cy)
        K = _lib._epi_K(focal_length, principal_point)
        camera = (K[0], K[1:])
    fn = {(False, False): _lib.epipolar_ransac, (False, True): _lib.epipolar_lmeds, (True, False): _lib.essential_ransac,
          (True, True): _lib.essential_lmeds}[essential, lmeds]
    r = fn(pts1, pts2, *camera, *criterion, hypotheses=hypotheses, seed=seed, refits=refits, samples=samples)
    info = r["info"]
    if lmeds:
        info = dict(info, method="LMEDS", rank=rank, value=r["value"], final_value=r["final_value"], bound=r["bound"],
                    refit_values=r["refit_values"])
    if essential:
        Km = np.array([[K[0], 0.0, K[1]], [0.0, K[0], K[2]], [0.0, 0.0, 1.0]])
        info = dict(info, E=Km.T @ r["F"] @ Km)
    return result(r["mask"], r["F"], info)


def _spatial_cells(pts, grid_size, image_size):
    # reference gcp.py:322-325, verbatim: what this arithmetic does to a point outside the image is part of the contract
    cell_col = (pts[:, 0] // grid_size).astype(int)
    cell_row = (pts[:, 1] // grid_size).astype(int)
    n_cols = int(np.ceil(image_size[0] / grid_size))
    return cell_col, cell_row, cell_row * n_cols + cell_col


def filter_spatial(pts, grid_size, image_size, selection="first", random_state=None):
    """``_filter_spatial`` (reference gcp.py:282-357), bit for bit: a bool mask that keeps one point per grid cell of
    ``grid_size`` pixels.

    ``"first"`` keeps the lowest index of each cell and ``"center"`` the point nearest the cell centre (the lowest index on an
    equal distance); both run on the device (``alp_grid_thin``), on the cell ids and distances formed with the reference's own
    expressions (gcp.py:322-325, 339-345).  ``"random"`` groups on the host and draws with the reference's own calls,
    ``default_rng(random_state)`` and one ``rng.choice`` per cell in ascending cell order: numpy's stream cannot be restated on
    the device.  Validation, messages and the empty case are the reference's (gcp.py:315-319, 349-353)."""
    if grid_size <= 0:
        raise ValueError("grid_size must be positive")
    if len(pts) == 0:
        return np.array([], dtype=bool)
    pts = np.asarray(pts)
    cell_col, cell_row, cell_id = _spatial_cells(pts, grid_size, image_size)
    if selection == "first":
        return _lib.grid_thin(cell_id)
    if selection == "random":
        rng = np.random.default_rng(random_state)
        order = np.argsort(cell_id, kind="stable")              # ascending cells, input order within a cell: pandas' groups
        starts = np.flatnonzero(np.r_[True, cell_id[order][1:] != cell_id[order][:-1]])
        selected = [rng.choice(group) for group in np.split(order.astype(np.int64), starts[1:])]
        mask = np.zeros(len(pts), dtype=bool)
        mask[selected] = True
        return mask
    if selection == "center":
        cell_center_x = (cell_col + 0.5) * grid_size
        cell_center_y = (cell_row + 0.5) * grid_size
        dist_to_center = np.sqrt(
            (pts[:, 0] - cell_center_x) ** 2 +
            (pts[:, 1] - cell_center_y) ** 2
        )
        return _lib.grid_thin(cell_id, dist_to_center)
    raise ValueError(
        f"Unknown selection '{selection}'. "
        "Available: 'first', 'random', 'center'"
    )


def filter_matches(pts1, pts2, image_size, outlier_filter="fundamental", threshold=10.0, spatial_thin_grid=None,
                   spatial_thin_selection="first", spatial_thin_random_state=None, params=None, **ransac):
    """``image_match`` from its line 507 to 544 (reference gcp.py), given the points ``match_keypoints`` returns: the geometric
    filter, then the spatial thinning on ``pts1``, then the DataFrame ``u_org, v_org, u_sim, v_sim`` (the empty frame with those
    columns when nothing is left).  ``image_size`` is (width, height) of the photograph, or None when no thinning is asked for;
    ``**ransac`` goes to ``filter_geometric`` (hypotheses, seed, refits, samples, and ransac_method, quantile, min_threshold: the
    reference's ``ransac_method`` argument, gcp.py:160-161).  ``params``: the camera parameters the
    simulated image was rendered from; ``outlier_filter="essential"`` takes its focal length and principal point from them as
    ``image_match`` does (gcp.py:466-474): f = (w / 2) / tan(fov / 2) from ``fov`` (degrees) and ``w``, (cx, cy) from ``cx``
    and ``cy``, else (w / 2, h / 2)."""
    pts1, pts2 = np.asarray(pts1), np.asarray(pts2)
    focal_length = None
    principal_point = None
    if params is not None:
        if "fov" in params and "w" in params:
            focal_length = (params["w"] / 2) / math.tan(params["fov"] * math.pi / 180 / 2)
        if "cx" in params and "cy" in params:
            principal_point = (params["cx"], params["cy"])
        elif "w" in params and "h" in params:
            principal_point = (params["w"] / 2, params["h"] / 2)
    if outlier_filter != "none" and len(pts1) > 0:
        mask = filter_geometric(pts1, pts2, method=outlier_filter, threshold=threshold, focal_length=focal_length,
                                principal_point=principal_point, image_size=image_size, **ransac)
        pts1 = pts1[mask]
        pts2 = pts2[mask]
    if spatial_thin_grid is not None and len(pts1) > 0:
        if image_size is None:
            raise ValueError(
                "image_size could not be determined. "
                "Ensure path_org is a valid image file."
            )
        mask = filter_spatial(pts1, grid_size=spatial_thin_grid, image_size=image_size, selection=spatial_thin_selection,
                              random_state=spatial_thin_random_state)
        pts1 = pts1[mask]
        pts2 = pts2[mask]
    if len(pts1) == 0:
        return pd.DataFrame(columns=["u_org", "v_org", "u_sim", "v_sim"])
    pts1 = np.atleast_2d(pts1)
    pts2 = np.atleast_2d(pts2)
    return pd.DataFrame(np.hstack((pts1, pts2)), columns=["u_org", "v_org", "u_sim", "v_sim"])
