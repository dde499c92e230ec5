"""The numpy restatement of the reference's matcher core (src/alproj/gcp.py:55-70) and the builders of the cases that
tests/test_gpu_match.py runs.  cv2 is not available where this project is built, so no fixture can come from cv2.BFMatcher
itself; what the restatement takes from cv2's documented behaviour is stated in DESIGN.md section 2.

restate(des1, des2, ratio) -> dict idx (N1, 2) int32, dist2 (N1, 2) int32, dist (N1, 2) float32, good (N1,) bool
  d^2   a float64 matmul of the integer-valued descriptors: every product and partial sum is an integer below 2^53, so it is
        exact in any order of summation (the largest d^2 here is 512 * 255^2 < 2^25)
  best  a stable argsort of d^2 per query: the lower train index first on a tie
  dist  np.sqrt(np.float32(d^2)): the correctly rounded float32 square root
  good  float(dist[0]) < ratio * float(dist[1]): Python's comparison of gcp.py:63 on DMatch.distance, a float32 read as a double
"""
import numpy as np


def dist2_matrix(des1, des2):
    a = np.asarray(des1, dtype=np.float64)
    b = np.asarray(des2, dtype=np.float64)
    d2 = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    return d2.astype(np.int64)


def restate(des1, des2, ratio=0.7):
    d2 = dist2_matrix(des1, des2)
    order = np.argsort(d2, axis=1, kind="stable")[:, :2]
    best = np.take_along_axis(d2, order, axis=1)
    dist = np.sqrt(best.astype(np.float32))
    good = dist[:, 0].astype(np.float64) < ratio * dist[:, 1].astype(np.float64)
    return {"idx": order.astype(np.int32), "dist2": best.astype(np.int32), "dist": dist, "good": good}


def restate_two_pass(des1, des2, ratio=0.7):
    """restate() for the one large case: two passes of argmin (numpy's returns the FIRST minimum, the lowest index) instead of
    a full stable sort of every row -- the same best two, ties included (tests/test_match_cases.py holds it to restate)"""
    d2 = dist2_matrix(des1, des2)
    rows = np.arange(len(d2))
    i0 = d2.argmin(axis=1)
    b0 = d2[rows, i0]
    d2[rows, i0] = np.iinfo(np.int64).max
    i1 = d2.argmin(axis=1)
    b1 = d2[rows, i1]
    best = np.stack([b0, b1], axis=1)
    dist = np.sqrt(best.astype(np.float32))
    good = dist[:, 0].astype(np.float64) < ratio * dist[:, 1].astype(np.float64)
    return {"idx": np.stack([i0, i1], axis=1).astype(np.int32), "dist2": best.astype(np.int32), "dist": dist, "good": good}


def restate_loops(des1, des2, ratio=0.7):
    """the same by three loops in Python integers (tests/test_match_cases.py holds restate to it)"""
    n1, n2, length = len(des1), len(des2), len(des1[0])
    idx = np.zeros((n1, 2), dtype=np.int32)
    dist2 = np.zeros((n1, 2), dtype=np.int32)
    for i in range(n1):
        pairs = []
        for j in range(n2):
            s = 0
            for k in range(length):
                d = int(des1[i][k]) - int(des2[j][k])
                s += d * d
            pairs.append((s, j))
        pairs.sort()                       # by (d^2, index)
        idx[i] = [pairs[0][1], pairs[1][1]]
        dist2[i] = [pairs[0][0], pairs[1][0]]
    dist = np.sqrt(dist2.astype(np.float32))
    good = np.array([float(dist[i, 0]) < ratio * float(dist[i, 1]) for i in range(n1)], dtype=bool)
    return {"idx": idx, "dist2": dist2, "dist": dist, "good": good}


def assert_same(got, want, what=""):
    """bit equality of idx, dist2, dist and good (and of n_good with the mask's sum, where `got` carries one)"""
    for key in ("idx", "dist2", "dist", "good"):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {key}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        if key == "dist":
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what} {key}: {len(bad)} differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"
    if "n_good" in got:
        assert got["n_good"] == int(np.asarray(want["good"]).sum()), f"{what} n_good"


# ---------------------------------------------------------------------------------------------------------------- builders
def random_bytes(n, length, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, length), dtype=np.uint8)


def unit_queries(length, pad=128):
    """e_k: 255 at k, the padding value elsewhere"""
    q = np.full((length, length), pad, dtype=np.uint8)
    q[np.arange(length), np.arange(length)] = 255
    return q


def asymmetric_train(n, length):
    """t[j][k] = (7 j + 13 k) % 251: no symmetry between rows and bytes, none under a reordering of k"""
    j, k = np.arange(n)[:, None], np.arange(length)[None, :]
    return ((7 * j + 13 * k) % 251).astype(np.uint8)


def noisy_copies(train, n, seed, noise=6):
    """n queries = train rows (drawn with replacement) + small noise, clipped to bytes: a healthy share passes the ratio test"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(train), size=n)
    q = train[pick].astype(np.int64) + rng.integers(-noise, noise + 1, size=(n, train.shape[1]))
    return np.clip(q, 0, 255).astype(np.uint8)
