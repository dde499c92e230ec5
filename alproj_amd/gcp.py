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
Detection (``detectAndCompute``), the geometric filters (cv2's USAC / RANSAC), ``_filter_spatial``
and the learned matchers behind ``vismatch`` stay with the reference: cv2 is neither imported nor
needed here.  ``set_gcp`` accepts, besides the reference's
``reverse_proj`` DataFrame, the device-resident ``alproj_amd.project.ReverseProjection``: the
(u_sim, v_sim) -> (x, y, z) join then becomes one gather from the coordinate image in HBM
(``alp_render_gather``) and the multi-million-row table is never built.
"""
import numpy as np
import pandas as pd

from . import _lib
from .project import ReverseProjection

__all__ = ["set_gcp", "filter_gcp_distance", "knn_match", "match_descriptors", "match_keypoints"]


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
