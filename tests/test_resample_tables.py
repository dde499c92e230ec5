"""CPU checks of the resampling tables (alproj_amd/resample.py) and of the refusals LsqOptimizer.cross_validate / .bootstrap
make before the device is touched.  No GPU is needed: a refusal that reached the device would raise AlprojHipError here."""
import numpy as np
import pandas as pd
import pytest

from alproj_amd import resample as rs


# ---------------------------------------------------------------------------------------------------- fold labels
@pytest.mark.parametrize("n,k", [(2, 2), (7, 2), (10, 3), (11, 5), (100, 7), (1024, 1024), (1500, 1024)])
def test_fold_sizes_differ_by_at_most_one(n, k):
    labels = rs.fold_labels(n, k, seed=3)
    assert labels.shape == (n,) and labels.dtype == np.int32
    sizes = np.bincount(labels, minlength=k)
    assert len(sizes) == k and sizes.min() >= 1 and sizes.max() - sizes.min() <= 1
    assert np.array_equal(labels, rs.fold_labels(n, k, seed=3))
    if n >= 10:
        assert not np.array_equal(labels, rs.fold_labels(n, k, seed=4))


def test_loo_is_the_identity_labelling_up_to_the_permutation():
    labels = rs.fold_labels(12, "loo", seed=1)
    assert np.array_equal(np.sort(labels), np.arange(12))
    train, held = rs.fold_tables(labels)
    assert train.shape == held.shape == (12, 12)
    assert (held.sum(axis=0) == 1).all() and (held.sum(axis=1) == 1).all()
    assert rs.fold_labels(1024, "loo").shape == (1024,)


def test_explicit_labels_are_relabelled_in_order_of_first_appearance():
    given = np.array([7, 7, -2, 40, -2, 7, 3, 40])
    assert rs.fold_labels(8, given).tolist() == [0, 0, 1, 2, 1, 0, 3, 2]
    assert rs.fold_labels(8, list(given.astype(np.float64))).tolist() == [0, 0, 1, 2, 1, 0, 3, 2]
    already = np.array([0, 1, 2, 0, 1, 2])
    assert np.array_equal(rs.fold_labels(6, already), already)


@pytest.mark.parametrize("n,folds", [(10, 1), (10, 0), (10, -3), (10, 11), (2000, 1025), (10, True), (10, "kfold"), (10, 2.5),
                                     (1025, "loo"), (1, "loo"), (5, [0, 1, 0, 1]), (4, [0.5, 1, 0, 1]), (4, [0, 0, 0, 0]),
                                     (4, [np.nan, 1, 0, 1]), (4, ["a", "b", "a", "b"]), (4, [[0, 1], [0, 1]])])
def test_fold_labels_refusals(n, folds):
    with pytest.raises(ValueError):
        rs.fold_labels(n, folds, seed=0)


def test_more_than_1024_explicit_folds_are_refused():
    with pytest.raises(ValueError):
        rs.fold_labels(1025, np.arange(1025))


# ---------------------------------------------------------------------------------------------------- fold tables
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,k", [(5, 2), (11, 5), (257, 8), (12, "loo")])
def test_every_point_is_held_out_exactly_once(n, k, weighted):
    labels = rs.fold_labels(n, k, seed=9)
    w = np.random.default_rng(2).uniform(0.1, 3.0, n) if weighted else None
    train, held = rs.fold_tables(labels, w)
    folds = int(labels.max()) + 1
    assert train.shape == held.shape == (folds, n) and train.dtype == held.dtype == np.float64
    want = np.ones(n) if w is None else w
    assert ((held != 0).sum(axis=0) == 1).all()                      # once, and in the fold the labels name
    assert np.array_equal(held[labels, np.arange(n)], want)
    assert np.array_equal(train + held, np.tile(want, (folds, 1)))    # exact: one of the two entries is 0
    assert ((train == 0) | (held == 0)).all()


def test_zero_weights_stay_zero_in_both_tables():
    labels = rs.fold_labels(9, 3, seed=0)
    w = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2], dtype=np.float64)
    train, held = rs.fold_tables(labels, w)
    assert (train[:, w == 0] == 0).all() and (held[:, w == 0] == 0).all()
    assert np.array_equal(train + held, np.tile(w, (3, 1)))


# ---------------------------------------------------------------------------------------------------- bootstrap tables
@pytest.mark.parametrize("n,n_boot", [(1, 1), (7, 3), (300, 16)])
def test_bootstrap_rows_sum_to_n_and_the_seed_fixes_them(n, n_boot):
    t = rs.bootstrap_table(n, n_boot, seed=5)
    assert t.shape == (n_boot, n) and t.dtype == np.float64
    assert (t == np.floor(t)).all() and (t >= 0).all()
    assert (t.sum(axis=1) == n).all()
    assert np.array_equal(t, rs.bootstrap_table(n, n_boot, seed=5))
    if n >= 7:
        assert not np.array_equal(t, rs.bootstrap_table(n, n_boot, seed=6))
        assert not np.array_equal(t[0], t[1])
    w = np.random.default_rng(0).uniform(0, 2, n)
    assert np.array_equal(rs.bootstrap_table(n, n_boot, seed=5, weights=w), t * w)
    # row b is the b-th draw of n indices from ONE generator
    rng = np.random.default_rng(5)
    for b in range(n_boot):
        assert np.array_equal(t[b], np.bincount(rng.integers(0, n, n), minlength=n))


@pytest.mark.parametrize("n_boot", [0, -1, 1025, True, 2.0, "3"])
def test_bootstrap_refusals(n_boot):
    with pytest.raises(ValueError):
        rs.bootstrap_table(10, n_boot, seed=0)


# ---------------------------------------------------------------------------------------------------- slices
def test_slices_side_by_side_are_the_whole_table():
    n = 23
    labels = rs.fold_labels(n, 4, seed=1)
    w = np.random.default_rng(3).uniform(0, 2, n)
    train, held = rs.fold_tables(labels, w)
    boot = rs.bootstrap_table(n, 6, seed=2, weights=w)
    for a in (0, 1, n - 1, n):
        tl, hl = rs.fold_tables(labels, w, 0, a)
        tr, hr = rs.fold_tables(labels, w, a, n)
        assert tl.shape == (4, a) and tr.shape == (4, n - a)
        assert np.array_equal(np.hstack([tl, tr]), train) and np.array_equal(np.hstack([hl, hr]), held)
        bl, br = rs.bootstrap_table(n, 6, 2, w, 0, a), rs.bootstrap_table(n, 6, 2, w, a, None)
        assert bl.shape == (6, a) and br.shape == (6, n - a)
        assert np.array_equal(np.hstack([bl, br]), boot)
    for lo, hi in ((-1, 3), (3, 2), (0, n + 1)):
        with pytest.raises(ValueError):
            rs.fold_tables(labels, w, lo, hi)
        with pytest.raises(ValueError):
            rs.bootstrap_table(n, 2, 0, None, lo, hi)


def test_table_check():
    rs.table_check(1024, (1 << 30) // (1024 * 8), 8)
    rs.table_check(2, 10, 8, [1.0, 0.5])
    for args in [(0, 10, 8), (1025, 10, 8), (1024, (1 << 30) // (1024 * 8) + 1, 8), (1024, (1 << 30) // (1024 * 4) + 1, 4)]:
        with pytest.raises(ValueError):
            rs.table_check(*args)
    with pytest.raises(ValueError, match="resample 1"):
        rs.table_check(3, 10, 8, [1.0, 0.0, 2.0])
    assert rs.WEIGHT_TABLE_MAX_BYTES == 1 << 30 and rs.FOLDS_MAX == 1024


# ---------------------------------------------------------------------------------------------------- the optimiser's refusals
def optimizer(n=40, weights=None, targets=("fov", "pan", "tilt", "roll")):
    from alproj_amd import _lib
    from alproj_amd import optimize as aopt
    rng = np.random.default_rng(0)
    obj = pd.DataFrame(rng.uniform(-100, 100, (n, 3)), columns=["x", "y", "z"])
    img = pd.DataFrame(rng.uniform(0, 1000, (n, 2)), columns=["u", "v"])
    init = {k: 0.0 for k in _lib.PARAM_KEYS}
    init.update(fov=60.0, w=1000.0, h=800.0, cx=500.0, cy=400.0)
    o = aopt.LsqOptimizer(obj, img, init, weights=weights)
    o.set_target(list(targets))
    return o


@pytest.mark.parametrize("folds", [1, 0, 41, 1025, "kfold", True, np.zeros(40, dtype=int), np.arange(39)])
def test_cross_validate_refuses_folds_out_of_range_before_the_device(folds):
    with pytest.raises(ValueError):
        optimizer().cross_validate(folds=folds, seed=0)


@pytest.mark.parametrize("n_boot", [0, 1025, 2.5, True])
def test_bootstrap_refuses_n_boot_out_of_range_before_the_device(n_boot):
    with pytest.raises(ValueError):
        optimizer().bootstrap(n_boot=n_boot, seed=0)


def test_a_table_over_the_cap_is_refused_before_the_device():
    n = (1 << 30) // (1024 * 8) + 1              # 1024 rows of n float64 weights: one row over 1 GiB
    o = optimizer(n)
    with pytest.raises(ValueError, match="exceeds"):
        o.cross_validate(folds=1024, seed=0)
    with pytest.raises(ValueError, match="exceeds"):
        o.bootstrap(n_boot=1024, seed=0)


@pytest.mark.parametrize("targets", [("fov", "w"), ("h",), ("fov", "fov")])
def test_targets_w_and_h_are_refused_before_the_device(targets):
    with pytest.raises(ValueError):
        optimizer(targets=targets).cross_validate(folds=2, seed=0)
    with pytest.raises(ValueError):
        optimizer(targets=targets).bootstrap(n_boot=2, seed=0)


def test_a_resample_whose_weights_are_all_zero_is_refused_before_the_device():
    labels = np.arange(40) % 4
    w = np.where(labels == 2, 1.0, 0.0)          # fold 2 holds every point of positive weight: its training row is empty
    with pytest.raises(ValueError, match="all zero"):
        optimizer(weights=w).cross_validate(folds=labels)
    # a bootstrap row that drew none of the two points of positive weight (the seed is chosen for it)
    w = np.zeros(40)
    w[:2] = 1.0
    seed = next(s for s in range(200) if (rs.bootstrap_table(40, 4, s, w).sum(axis=1) == 0).any())
    with pytest.raises(ValueError, match="all zero"):
        optimizer(weights=w).bootstrap(n_boot=4, seed=seed)


@pytest.mark.parametrize("kw", [dict(loss="l2"), dict(f_scale=0.0), dict(device_loop=True, check_every=0)])
def test_the_shared_arguments_are_checked_before_the_device(kw):
    with pytest.raises(ValueError):
        optimizer().cross_validate(folds=2, seed=0, **kw)
    with pytest.raises(ValueError):
        optimizer().bootstrap(n_boot=2, seed=0, **kw)
