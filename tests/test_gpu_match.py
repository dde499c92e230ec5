"""GPU: alp_match_knn2 and the Python layer over it (knn_match, match_descriptors, match_keypoints) -- the exact brute-force
2-nearest-neighbour search and ratio test of the reference's built-in matchers (src/alproj/gcp.py:52-70) -- against the numpy
restatement of tests/match_cases.py.  Every comparison is bit equality of idx, dist2, dist and good.

what can go wrong                                             where it is held
the i8 fragment's lane-to-k map, rows against columns         test_fragment_map: unit queries x asymmetric train rows, every
                                                              (query, row) distance, rows in slices of 2 and in their tile places
partial tiles of queries / train rows, padding of L           test_launch_seams (sizes either side of 32, 64, 128, 256; nine L)
the plan's own tile sizes and split boundaries                test_seams_from_the_plan (read from info)
the split merge                                               test_splits_give_one_answer
the order on equal distance                                   test_ties
the key's high word, -128 * 127, padding rows                 test_range
the float32 square root and the double comparison             test_ratio_boundaries, test_ratio_on_noisy_copies
float32 input and its refusals                                test_float32_input
more workgroups than the GPU holds at once                    test_beyond_one_wave_of_workgroups
lines 52-70 as a whole, the refusals of the C entry point     test_match_keypoints_reproduces_the_reference_lines, test_entry_point_refusals

The refusals of the Python layer (every one a ValueError raised with no device call) need no GPU: tests/test_match_cases.py.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
LENGTHS = (1, 31, 32, 33, 61, 64, 65, 128, 512)


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def check(L, des1, des2, ratio=0.7, splits=0, what="", restate=mc.restate):
    got = L.match_knn2(des1, des2, ratio, splits)
    mc.assert_same(got, restate(des1, des2, ratio), f"{what} {des1.shape} x {des2.shape} splits {splits} ->")
    return got


# ------------------------------------------------------------------------------------------------------------ fragment map
@pytest.mark.parametrize("length", [64, 128])
def test_fragment_map(L, length):
    """Unit queries e_k (255 at k, the padding value elsewhere) pick byte k of every train row; the train rows
    t[j][k] = (7 j + 13 k) % 251 differ under any exchange of rows with columns and any reordering of k that is not applied
    to both operands alike.  The full (query, row) matrix of dist2: two rows at a time, (a) as a train set of 2, (b) in their own
    places of a 32-row tile whose other rows are all 0 -- no closer to any e_k than a row of values 0..250."""
    q = mc.unit_queries(length)[:32]
    q_all = mc.unit_queries(length)
    t = mc.asymmetric_train(32, length)
    want = mc.dist2_matrix(q_all, t)
    assert len(np.unique(want)) > 500                         # the case distinguishes positions
    full = np.zeros_like(want)
    for a in range(0, 32, 2):
        got = check(L, q_all, t[a:a + 2].copy(), what=f"slice {a}")
        full[np.arange(length)[:, None], a + got["idx"]] = got["dist2"]
        placed = np.zeros_like(t)
        placed[a:a + 2] = t[a:a + 2]
        got = check(L, q_all, placed, what=f"rows {a}, {a + 1} in place")
        assert sorted(set(got["idx"].ravel().tolist())) == [a, a + 1]
    np.testing.assert_array_equal(full, want)
    check(L, q, t, what="32 x 32")
    check(L, t, q, what="32 x 32 transposed roles")


# ------------------------------------------------------------------------------------------------------------ launch seams
def seam_pairs():
    pairs = [(n1, n2) for n1 in SIZES for n2 in (2, 129)] + [(n1, n2) for n2 in SIZES if n2 >= 2 for n1 in (1, 33)]
    return sorted(set(pairs))


@pytest.mark.parametrize("length", LENGTHS)
def test_launch_seams(L, length):
    # a small alphabet at L = 1 would make everything a tie (held in test_ties); bytes are drawn from the whole range
    q_all, t_all = mc.random_bytes(257, length, 100 + length), mc.random_bytes(257, length, 200 + length)
    for n1, n2 in seam_pairs():
        check(L, q_all[:n1].copy(), t_all[:n2].copy(), what=f"L {length}")


@pytest.mark.parametrize("length", [61, 128, 512])
def test_seams_from_the_plan(L, length):
    """query tile +- 1, train tile +- 1 and train tile x splits +- 1, with the tile sizes and the split count the plan reports"""
    q_all, t_all = mc.random_bytes(600, length, 7), mc.random_bytes(1200, length, 8)
    info = L.match_knn2(q_all[:33].copy(), t_all[:129].copy())["info"]
    qt, tt = info["query_tile"], info["train_tile"]
    assert info["padded_len"] >= length and info["padded_len"] % 32 == 0 and qt % 32 == 0 and tt == 32
    for n1 in (qt - 1, qt, qt + 1, 2 * qt + 1):
        for n2 in (tt - 1, tt, tt + 1):
            check(L, q_all[:n1].copy(), t_all[:n2].copy(), what=f"L {length}")
        for forced in (3, 7):
            for n2 in (tt * forced - 1, tt * forced, tt * forced + 1):
                got = check(L, q_all[:n1].copy(), t_all[:n2].copy(), splits=forced, what=f"L {length}")
                assert got["info"]["splits"] == forced
    # the plan's own choice on a train set of many tiles: the rows either side of tiles x splits
    s = L.match_knn2(q_all[:qt + 1].copy(), t_all[:1000].copy())["info"]["splits"]
    assert s >= 2
    for n2 in (tt * s - 1, tt * s, tt * s + 1):
        got = check(L, q_all[:qt + 1].copy(), t_all[:n2].copy(), what=f"L {length}")
        assert got["info"]["workgroups"] == got["info"]["splits"] * 2


# ------------------------------------------------------------------------------------------------------------ splits
PLACES = [(0, 160), (5, 100), (101, 6), (40, 41), (31, 32), (63, 64), (65, 96), (158, 159), (130, 20)]


@pytest.mark.parametrize("reverse", [False, True])
def test_splits_give_one_answer(L, reverse):
    """N2 = 5 train tiles + 1; the best (an exact copy, d2 = 0) and the second best (one byte off by one, d2 = 1) of each query
    sit in different splits, in the same split, and at train indices 0 and N2 - 1.  splits forced to 1, 2, 3 and the maximum."""
    n2 = 5 * 32 + 1
    t = mc.random_bytes(n2, 61, 31)
    q = np.zeros((len(PLACES), 61), dtype=np.uint8)
    for i, (b, s) in enumerate(PLACES):
        if reverse:
            b, s = s, b
        q[i] = t[b]
        t[s] = t[b]
        t[s, i] ^= 1
    q = np.concatenate([q, mc.random_bytes(40, 61, 32)])
    results = []
    for splits in (1, 2, 3, 6):
        got = check(L, q, t, splits=splits, what="placed")
        assert got["info"]["splits"] == splits
        results.append(got)
    for i, (b, s) in enumerate(PLACES):
        assert results[0]["idx"][i].tolist() == ([s, b] if reverse else [b, s]) and results[0]["dist2"][i].tolist() == [0, 1]
    for r in results[1:]:
        mc.assert_same(r, results[0], "splits")
    with pytest.raises(L.AlprojHipError, match="splits = 7") as e:
        L.match_knn2(q, t, 0.7, 7)
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------------------ ties
def test_ties(L):
    n2 = 5 * 32 + 1
    t = mc.random_bytes(n2, 61, 41)
    t[7] = t[3]              # inside one tile
    t[32] = t[31]            # across a tile boundary
    t[96] = t[95]            # across the boundary of the two splits of 6 tiles (tiles 0-2 | 3-5)
    t[160] = t[0]            # first and last row
    q = np.stack([t[3], t[31], t[95], t[0], t[50]])
    q = np.concatenate([q, mc.noisy_copies(q, 30, 42, noise=1)])       # near the duplicates: equal second-best distances too
    for splits in (1, 2, 6):
        got = check(L, q, t, splits=splits, what="duplicates")
        assert got["idx"][:4].tolist() == [[3, 7], [31, 32], [95, 96], [0, 160]] and not got["dist2"][:4].any()
        assert got["idx"][4, 0] == 50 and got["dist2"][4, 0] == 0
        assert not got["good"][:4].any()                       # 0 < ratio * 0 never holds
    # all train rows identical: every distance ties, the two lowest indices win
    for n2 in (2, 33, 161):
        same = np.tile(mc.random_bytes(1, 61, 43), (n2, 1))
        for splits in (1, min(6, (n2 + 31) // 32)):
            got = check(L, q, same, splits=splits, what="identical rows")
            assert (got["idx"] == [0, 1]).all()
    # L = 1, 2: a small alphabet, ties everywhere
    for length in (1, 2):
        check(L, mc.random_bytes(70, length, 44) // 32, mc.random_bytes(161, length, 45) // 32, what=f"alphabet L {length}")
        check(L, mc.random_bytes(70, length, 44) // 32, mc.random_bytes(161, length, 45) // 32, splits=6, what=f"alphabet L {length}")


# ------------------------------------------------------------------------------------------------------------ range
def test_range(L):
    zeros, ones = np.zeros((3, 512), dtype=np.uint8), np.full((2, 512), 255, dtype=np.uint8)
    got = check(L, zeros, ones, what="0 against 255")          # one real tile of 2 rows: padding must never win
    assert (got["dist2"] == 33292800).all() and (got["idx"] == [0, 1]).all()
    got = check(L, np.full((3, 512), 255, dtype=np.uint8), np.zeros((2, 512), dtype=np.uint8), what="255 against 0")
    assert (got["dist2"] == 33292800).all()
    got = check(L, zeros, np.zeros((2, 512), dtype=np.uint8), what="0 against 0")        # (-128)^2 x 512 in the accumulator
    assert not got["dist2"].any()
    got = check(L, np.full((3, 512), 255, dtype=np.uint8), ones, what="255 against 255")
    assert not got["dist2"].any()
    mixed = np.concatenate([ones, np.zeros((31, 512), dtype=np.uint8), ones])            # the far rows first and last, over two tiles
    got = check(L, zeros, mixed, what="far rows around near ones")
    assert (got["idx"] == [2, 3]).all()
    for length in LENGTHS:
        check(L, np.zeros((2, length), dtype=np.uint8), np.full((2, length), 255, dtype=np.uint8), what=f"extremes L {length}")


# ------------------------------------------------------------------------------------------------------------ ratio
def test_ratio_on_noisy_copies(L):
    t = mc.random_bytes(700, 61, 51)
    t[350:] = np.clip(t[:350].astype(np.int64) + np.random.default_rng(52).integers(-9, 10, size=(350, 61)), 0, 255)   # near pairs: some fail
    q = np.concatenate([mc.noisy_copies(t, 300, 53), mc.random_bytes(60, 61, 54)])
    for ratio in (0.7, 0.5, 1.0, 0.0, -1.0, 1e300):
        got = check(L, q, t, ratio=ratio, what=f"ratio {ratio}")
        assert got["n_good"] == int(got["good"].sum())
    share = L.match_knn2(q, t, 0.7)["good"].mean()
    assert 0.2 < share < 0.95, share


def test_ratio_boundaries(L):
    """d2 pairs on and next to the boundary of the comparison: (49, 100) is 7 against 0.7 * 10, (25, 100) 5 against 0.5 * 10,
    equal distances against ratio 1.0 -- each a train set of two rows around the query (100, ...)"""
    firsts = {1: [(7,), (5,), (1,), (0,), (10,)], 2: [(7, 0), (7, 1), (6, 3), (5, 5), (5, 0), (0, 0), (1, 0), (10, 0), (8, 6)]}
    seconds = {1: [(10,), (7,), (2,), (0,), (1,), (5,)], 2: [(10, 0), (10, 1), (7, 7), (8, 6), (9, 4), (9, 5), (0, 0), (1, 0), (2, 0), (7, 0), (5, 0)]}
    seen = set()
    for length in (1, 2):
        q = np.full((1, length), 100, dtype=np.uint8)
        for a in firsts[length]:
            for b in seconds[length]:
                t = np.array([np.add(100, a), np.subtract(100, b)], dtype=np.uint8)
                for ratio in (0.7, 0.5, 1.0):
                    got = check(L, q, t, ratio=ratio, what=f"offsets {a} {b} ratio {ratio}")
                    seen.add((tuple(got["dist2"][0].tolist()), ratio, bool(got["good"][0])))
    # the boundary itself was there, and it falls as the double comparison says
    for d2, ratio in (((49, 100), 0.7), ((25, 100), 0.5), ((49, 49), 1.0), ((0, 0), 1.0), ((100, 100), 1.0)):
        want = float(np.sqrt(np.float32(d2[0]))) < ratio * float(np.sqrt(np.float32(d2[1])))
        assert (d2, ratio, want) in seen and (d2, ratio, not want) not in seen
    assert ((49, 101), 0.7, True) in seen and ((50, 100), 0.7, False) in seen


# ------------------------------------------------------------------------------------------------------------ float32 input
def test_float32_input(L):
    q, t = mc.random_bytes(70, 128, 61), mc.random_bytes(161, 128, 62)
    q[0], t[5] = 0, 255
    got8 = check(L, q, t, what="uint8")
    got32 = check(L, q.astype(np.float32), t.astype(np.float32), what="float32")
    mc.assert_same(got32, got8, "float32 against uint8")
    # values that are no byte: ALP_EINVAL naming the lowest offending flat index, whichever array and however many there are
    for value in (0.5, -1.0, 256.0, float("nan"), float("inf"), 255.5, -0.5):
        for at in ((0, 0), (69, 127), (33, 61)):
            bad = q.astype(np.float32)
            bad[at] = value
            bad[69, 127] = value
            with pytest.raises(L.AlprojHipError, match=rf"query value at flat index {at[0] * 128 + at[1]} ") as e:
                L.match_knn2(bad, t.astype(np.float32))
            assert e.value.code == -1
        bad = t.astype(np.float32)
        bad[160, 3] = value
        bad[100, 9] = value
        with pytest.raises(L.AlprojHipError, match=rf"train value at flat index {100 * 128 + 9} "):
            L.match_knn2(q.astype(np.float32), bad)
    assert L.match_knn2(q.astype(np.float32), t.astype(np.float32))["n_good"] == got8["n_good"]      # and the library goes on
    zero = np.zeros((3, 128), dtype=np.float32)
    zero[1, 7] = -0.0                                            # minus zero is the integer 0
    check(L, zero, t.astype(np.float32), what="-0.0")


# ------------------------------------------------------------------------------------------------------------ a larger size
def test_beyond_one_wave_of_workgroups(L):
    """4096 x 8192 at L = 61: more query tiles x splits than one round of workgroups, thousands of rows per lane"""
    t = mc.random_bytes(8192, 61, 71)
    q = np.concatenate([mc.noisy_copies(t, 2048, 72, noise=20), mc.random_bytes(2048, 61, 73)])
    got = check(L, q, t, what="large", restate=mc.restate_two_pass)
    assert got["info"]["workgroups"] >= 32


# ------------------------------------------------------------------------------------------------------------ Python layer
def reference_lines_52_70(pts1_all, des1, pts2_all, des2, ratio):
    """src/alproj/gcp.py:52-70 with the restatement in place of cv2.BFMatcher().knnMatch"""
    empty = np.array([]).reshape(0, 2).astype("int32"), np.array([]).reshape(0, 2).astype("int32")
    if des1 is None or des2 is None or len(pts1_all) < 2 or len(pts2_all) < 2:
        return empty
    r = mc.restate(des1, des2, ratio)
    good = [(i, int(r["idx"][i, 0])) for i in range(len(des1)) if float(r["dist"][i, 0]) < ratio * float(r["dist"][i, 1])]
    if len(good) == 0:
        return empty
    pts1 = np.float32([tuple(pts1_all[i]) for i, _ in good]).astype("int32")
    pts2 = np.float32([tuple(pts2_all[j]) for _, j in good]).astype("int32")
    return pts1, pts2


def test_match_keypoints_reproduces_the_reference_lines(L):
    from alproj_amd import gcp
    rng = np.random.default_rng(81)
    des2 = mc.random_bytes(300, 61, 82)
    des1 = np.concatenate([mc.noisy_copies(des2, 150, 83), mc.random_bytes(50, 61, 84)])
    pts1 = np.floor(rng.uniform(0, 5616, size=(200, 2))) + 0.9        # x.9 coordinates: truncated, not rounded
    pts2 = rng.uniform(0, 3744, size=(300, 2))
    pts1[0] = [5615.9, 0.9]
    for ratio in (0.7, 0.9):
        got = gcp.match_keypoints(pts1, des1, pts2, des2, ratio)
        want = reference_lines_52_70(pts1, des1, pts2, des2, ratio)
        for g, w in zip(got, want):
            assert g.dtype == np.int32 and g.shape == w.shape and len(g) > 20
            np.testing.assert_array_equal(g, w)
        assert (got[0] == np.floor(got[0])).all() and got[0].max() <= 5615
    f1, f2 = des1.astype(np.float32), des2.astype(np.float32)          # SIFT's dtype
    for g, w in zip(gcp.match_keypoints(pts1, f1, pts2, f2), reference_lines_52_70(pts1, des1, pts2, des2, 0.7)):
        np.testing.assert_array_equal(g, w)
    # keypoints as a list of kp.pt tuples, as the reference holds them
    for g, w in zip(gcp.match_keypoints([tuple(p) for p in pts1], des1, [tuple(p) for p in pts2], des2),
                    reference_lines_52_70(pts1, des1, pts2, des2, 0.7)):
        np.testing.assert_array_equal(g, w)
    # nothing passes: every train row twice
    twice = np.concatenate([des2[:20], des2[:20]])
    for g in gcp.match_keypoints(pts1, des1, pts2[:40], twice):
        assert g.shape == (0, 2) and g.dtype == np.int32
    # fewer than 2 keypoints on either side, or no descriptors
    for args in ((pts1[:1], des1[:1], pts2, des2), (pts1, des1, pts2[:1], des2[:1]), (pts1, None, pts2, des2), (pts1, des1, pts2, None)):
        for g in gcp.match_keypoints(*args):
            assert g.shape == (0, 2) and g.dtype == np.int32
    # the two smaller functions
    idx, dist = gcp.knn_match(des1, des2)
    r = mc.restate(des1, des2)
    assert idx.dtype == np.int32 and dist.dtype == np.float32
    np.testing.assert_array_equal(idx, r["idx"])
    np.testing.assert_array_equal(dist.view(np.uint32), r["dist"].view(np.uint32))
    qi, ti = gcp.match_descriptors(des1, des2, 0.7)
    np.testing.assert_array_equal(qi, np.flatnonzero(r["good"]))
    np.testing.assert_array_equal(ti, r["idx"][r["good"], 0])
    assert qi.dtype == ti.dtype == np.int32
    idx, dist = gcp.knn_match(des1[:0], des2)                          # no query: nothing happens
    assert idx.shape == dist.shape == (0, 2)
    assert all(len(a) == 0 for a in gcp.match_descriptors(des1[:0], des2))


def test_entry_point_refusals(L):
    """alp_match_knn2 itself: ALP_EINVAL before anything is uploaded"""
    lib = L.lib()
    q, t = mc.random_bytes(8, 61, 91), mc.random_bytes(40, 61, 92)
    qp, tp = q.ctypes.data_as(ctypes.c_void_p), t.ctypes.data_as(ctypes.c_void_p)
    n_good = ctypes.c_int64(-5)

    def call(query=qp, n_query=8, train=tp, n_train=40, length=61, dtype=L.ALP_U8, ratio=0.7, splits=0):
        return lib.alp_match_knn2(query, n_query, train, n_train, length, dtype, ratio, splits, None, None, None, None, ctypes.byref(n_good), None)
    assert call() == 0 and n_good.value >= 0                    # every output but the count NULL
    for kw, text in ((dict(query=None), "NULL"), (dict(train=None), "NULL"), (dict(length=0), "1..512"), (dict(length=513), "1..512"),
                     (dict(n_train=1), "n_train"), (dict(n_train=0), "n_train"), (dict(n_query=-1), "n_query"),
                     (dict(ratio=float("nan")), "finite"), (dict(ratio=float("inf")), "finite"), (dict(splits=3), "splits"),
                     (dict(splits=-1), "splits"), (dict(dtype=L.ALP_F64), "dtype"), (dict(dtype=L.ALP_U16), "dtype"),
                     (dict(n_train=(1 << 31) // 64), "2^31"), (dict(n_query=(1 << 31) // 64), "2^31"),
                     (dict(n_train=(1 << 31) // 512, length=512), "2^31")):
        assert call(**kw) == -1, kw
        assert text in lib.alp_last_error().decode(), (kw, lib.alp_last_error())
    assert call(splits=2) == 0
    info = (ctypes.c_int64 * 6)()
    assert lib.alp_match_knn2(None, 0, tp, 40, 61, L.ALP_U8, 0.7, 0, None, None, None, None, ctypes.byref(n_good), info) == 0
    assert n_good.value == 0 and info[1] == 32 and info[3] == 64 and info[4] == 0
