"""Resampling tables for ``LsqOptimizer.cross_validate`` and ``LsqOptimizer.bootstrap``: which point counts how often in
which fit.  Pure host code, numpy only; nothing here loads the HIP library.

A table has one row per fit and one column per point: row b holds the frequency weights the device gives point i in fit b
(``Points.set_weight_table``).  Every function takes the GLOBAL point count / labels and an optional column slice
``[lo, hi)``: with several ranks every rank builds the same global labels or counts from one seed and keeps the columns of
its own shard, and the slices of all ranks, side by side, are the whole table.
"""
import numpy as np

__all__ = ["FOLDS_MAX", "WEIGHT_TABLE_MAX_BYTES", "fold_labels", "fold_tables", "bootstrap_table", "table_check"]

FOLDS_MAX = 1024                      # rows of a weight table: alp_normal_equations_batch's poses per call
WEIGHT_TABLE_MAX_BYTES = 1 << 30      # ALP_WEIGHT_TABLE_MAX_BYTES: a guard, not a tuned number


def _slice(n, lo, hi):
    hi = n if hi is None else int(hi)
    lo = int(lo)
    if not 0 <= lo <= hi <= n:
        raise ValueError(f"the column slice [{lo}, {hi}) does not lie in [0, {n}]")
    return lo, hi


def _weights(weights, n):
    """(n,) float64 weights, finite and >= 0; ones for None"""
    if weights is None:
        return np.ones(n, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != (n,):
        raise ValueError(f"weights must have shape ({n},)")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights must be finite and >= 0")
    return w


def fold_labels(n, folds=5, seed=None):
    """(n,) int32 fold labels 0 .. k-1 of n points.  ``folds``: an integer k, 2 <= k <= min(n, FOLDS_MAX) -- a permutation
    from ``np.random.default_rng(seed)`` dealt round-robin, so the fold sizes differ by at most 1; ``"loo"`` -- every point
    its own fold (k = n, refused above FOLDS_MAX points); or n explicit integer labels, relabelled 0 .. k-1 in the order of
    their first appearance.  ValueError for anything else."""
    n = int(n)
    if isinstance(folds, str):
        if folds != "loo":
            raise ValueError("folds must be an integer, 'loo' or an array of n labels")
        if not 2 <= n <= FOLDS_MAX:
            raise ValueError(f"folds='loo' needs 2 .. {FOLDS_MAX} points, not {n}")
        return np.arange(n, dtype=np.int32)
    if isinstance(folds, (bool, np.bool_)):
        raise ValueError("folds must be an integer, 'loo' or an array of n labels")
    if isinstance(folds, (int, np.integer)):
        k = int(folds)
        if not 2 <= k <= min(n, FOLDS_MAX):
            raise ValueError(f"folds must be 2 .. min(n, {FOLDS_MAX}) = {min(n, FOLDS_MAX)}, not {k}")
        labels = np.empty(n, dtype=np.int32)
        labels[np.random.default_rng(seed).permutation(n)] = np.arange(n, dtype=np.int32) % k
        return labels
    given = np.asarray(folds)
    if given.shape != (n,):
        raise ValueError(f"explicit fold labels must have shape ({n},)")
    if given.dtype.kind == "f":
        if not np.isfinite(given).all() or (given != np.floor(given)).any():
            raise ValueError("explicit fold labels must be integers")
    elif given.dtype.kind not in "iu":
        raise ValueError("explicit fold labels must be integers")
    _, first, inverse = np.unique(given, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int32)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first), dtype=np.int32)      # order of first appearance
    k = len(first)
    if not 2 <= k <= FOLDS_MAX:
        raise ValueError(f"explicit fold labels must name 2 .. {FOLDS_MAX} folds, not {k}")
    return rank[inverse.reshape(-1)].astype(np.int32)


def fold_tables(labels, weights=None, lo=0, hi=None):
    """-> (train, held), two (k, hi - lo) float64 tables for the labels 0 .. k-1 of ``fold_labels``:
    ``train[b, i] = w_i [label_i != b]`` and ``held[b, i] = w_i [label_i == b]`` for the columns [lo, hi) of the global
    index range (``weights``: n global weights, ones for None).  train + held = w in every row, exactly: each entry of one
    of them is 0."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.dtype.kind not in "iu" or (len(labels) and labels.min() < 0):
        raise ValueError("labels must be a one-dimensional array of integers >= 0")
    n = len(labels)
    lo, hi = _slice(n, lo, hi)
    w = _weights(weights, n)[lo:hi]
    k = int(labels.max()) + 1 if n else 0
    own = labels[None, lo:hi] == np.arange(k, dtype=labels.dtype)[:, None]
    return np.where(own, 0.0, w[None, :]), np.where(own, w[None, :], 0.0)


def bootstrap_table(n, n_boot, seed=None, weights=None, lo=0, hi=None):
    """(n_boot, hi - lo) float64: row b = how often each point is drawn in n draws with replacement from the n points,
    times w_i.  The rows are drawn one after the other from ONE ``np.random.default_rng(seed)``; a slice is that slice of
    the global rows, so the slices of all ranks side by side are the whole table (with ``seed=None`` every call draws
    anew: name a seed to get the same table twice)."""
    if isinstance(n_boot, (bool, np.bool_)) or not isinstance(n_boot, (int, np.integer)) or not 1 <= n_boot <= FOLDS_MAX:
        raise ValueError(f"n_boot must be an integer 1 .. {FOLDS_MAX}")
    n, n_boot = int(n), int(n_boot)
    if n < 1:
        raise ValueError("a bootstrap needs at least one point")
    lo, hi = _slice(n, lo, hi)
    w = _weights(weights, n)[lo:hi]
    rng = np.random.default_rng(seed)
    out = np.empty((n_boot, hi - lo), dtype=np.float64)
    for b in range(n_boot):
        counts = np.bincount(rng.integers(0, n, n), minlength=n)
        out[b] = counts[lo:hi] * w
    return out


def table_check(rows, n_local, element_bytes, row_sums=None):
    """The refusals of a weight table that need no device: more than FOLDS_MAX rows, a stored size (rows x n_local values
    of ``element_bytes`` bytes) above WEIGHT_TABLE_MAX_BYTES, and -- ``row_sums``: the global sum of every row, when the
    caller knows it -- a resample whose weights are all zero.  ValueError."""
    rows, n_local = int(rows), int(n_local)
    if not 1 <= rows <= FOLDS_MAX:
        raise ValueError(f"a weight table has 1 .. {FOLDS_MAX} rows, not {rows}")
    if rows * n_local * int(element_bytes) > WEIGHT_TABLE_MAX_BYTES:
        raise ValueError(f"a weight table of {rows} x {n_local} values of {element_bytes} bytes exceeds "
                         f"{WEIGHT_TABLE_MAX_BYTES} bytes: use fewer folds / resamples or fewer points")
    if row_sums is not None:
        empty = np.flatnonzero(~(np.asarray(row_sums, dtype=np.float64) > 0))
        if len(empty):
            raise ValueError(f"the weights of resample {int(empty[0])} are all zero: no point is left to fit")
