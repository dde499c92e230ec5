"""CPU: the layouts of tests/rasterize_seam_cases.py do what they say -- asserted on the REALISED sorted cell array, not on
the lists they were built from -- and sit on the constants of rasterize_runs.h, rasterize_median.h and rasterize_tail.h,
which are read from the source: a changed constant fails here and does not silently move the seams that
tests/test_gpu_rasterize_seams.py aims at."""
import os
import re
import warnings

import numpy as np
import pytest

from oracle import ref_numpy as orc
from tests import rasterize_seam_cases as sc

CSRC = os.path.join(os.path.dirname(os.path.dirname(__file__)), "alproj_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_cases_sit_on_the_kernels_constants():
    runs, median, tail = _src("rasterize_runs.h"), _src("rasterize_median.h"), _src("rasterize_tail.h")
    assert int(re.search(r"constexpr int RZ_SEG = (\d+);", runs).group(1)) == sc.RZ_SEG
    m = re.search(r"constexpr int RZ_MED_GROUPS = (\d+), RZ_MED_TURN = RZ_MED_GROUPS \* (\d+);", median)
    assert int(m.group(1)) == sc.RZ_MED_GROUPS and int(m.group(1)) * int(m.group(2)) == sc.RZ_MED_TURN and int(m.group(2)) == 64
    m = re.search(r"constexpr int RZ_TW = (\d+), RZ_TH = (\d+), RZ_SMAX = (\d+);", tail)
    assert tuple(int(g) for g in m.groups()) == (sc.RZ_TW, sc.RZ_TH, sc.RZ_SMAX)
    assert int(re.search(r"constexpr int RZ_TILE_BITS = (\d+);", tail).group(1)) == sc.RZ_TILE_BITS
    # the files' capacities: TURN, TURN / 3 + 4, / 5, / 9 (16-bit entries) and / 17 (the long runs' two arrays)
    m = re.search(r"unsigned short file0\[TURN\], file1\[TURN / (\d+) \+ (\d+)\], file2\[TURN / (\d+) \+ (\d+)\], "
                  r"file3\[TURN / (\d+) \+ (\d+)\];", median)
    assert tuple(int(g) for g in m.groups()) == (3, 4, 5, 4, 9, 4)
    m = re.search(r"unsigned long_off\[TURN / (\d+) \+ (\d+)\], long_len\[TURN / (\d+) \+ (\d+)\];", median)
    assert tuple(int(g) for g in m.groups()) == (17, 4, 17, 4)
    assert "constexpr int TURN = GROUPS * 64;" in median
    for shortest, heads in sc.CAPACITY_HEADS.items():
        assert heads == -(-sc.RZ_MED_TURN // shortest) <= sc.FILE_CAPACITY[shortest]
    # the file classes the layouts aim at
    for text in ("len >= 1u && len <= 2u", "len >= 3u && len <= 4u", "len >= 5u && len <= 8u", "len >= 9u && len <= 16u", "len > 16u"):
        assert median.count(text) >= 2
    # the runs kernel walks eight points at a time, the join four segments at a time
    assert "for (; k + 8 <= j; k += 8)" in runs and "for (; u + 4 <= e + 1; u += 4)" in runs


@pytest.mark.parametrize("width", [2, 3, 4, 6])
def test_table_from_runs_reproduces_its_raster(width):
    """zero-length cells included: the oracle derives the raster size from the table and finds `lengths` points per cell"""
    lengths = [2, 0, 1, 3, 0, 1, 1, 0, 0, 2, 1, 4, 1, 0, 5, 0, 1, 2, 0, 1, 1, 1, 0, 3]
    x, y, (w, h) = sc.table_from_runs(lengths, width, seed=width)
    assert w == width and h == len(lengths) // width
    count, bounds = orc.rasterize_points(x, y, np.ones((len(x), 1)), 1.0, False, 1.0, "mean", 0, return_float=True)
    assert bounds == (0.0, 0.0, float(w), float(h), w, h)
    np.testing.assert_array_equal(np.isfinite(count[0]).ravel(), np.array(lengths) > 0)
    np.testing.assert_array_equal(np.bincount(sc.cells_of(x, y, (w, h)), minlength=len(lengths)), lengths)
    assert (np.diff(sc.cells_of(x, y, (w, h))) < 0).any()            # not in cell order
    with pytest.raises(AssertionError, match="rim"):
        sc.table_from_runs([0, 1, 0, 1], 2)
    x, y, size = sc.one_cell_table(50)
    assert size == (1, 1) and orc.rasterize_points(x, y, np.ones((50, 1)), 1.0, False)[1][4:] == (1, 1)


def test_segments_layout():
    tables = {t.name: t for t in sc.segments()}
    assert [tables[f"n%16={m}"].n % 16 for m in (0, 1, 15)] == [0, 1, 15]
    assert tables["n<16"].n < 16 and len(tables["n<16"].starts) == 6
    assert tables["one_cell"].n == 1000 and list(tables["one_cell"].lengths) == [1000]
    for m in (0, 1, 15):
        t = tables[f"n%16={m}"]
        assert t.n < 5000
        for length in sc.SEGMENT_LENGTHS:
            for off in sc.SEGMENT_OFFSETS:
                assert t.start(f"len{length}@{off}") % 16 == off and t.length(f"len{length}@{off}") == length
        for k in (1, 2, 4):             # fills k segments exactly; the run before it ends on the boundary by construction
            s = t.start(f"fill{k}")
            assert s % 16 == 0 and t.length(f"fill{k}") == 16 * k and s > 0 and t.sorted_cells[s - 1] != t.sorted_cells[s]
        followers = []
        for k in range(1, 10):          # the join's four-wide loop: every quad count and every remainder
            s, length = t.start(f"tail{k}"), t.length(f"tail{k}")
            assert s % 16 == 8
            followers.append((s + length - 1) // 16 - s // 16)
        assert followers == list(range(1, 10))
        assert {(f // 4, f % 4) for f in followers} == {(0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (2, 1)}
        s, length = t.start("nan_mid"), t.length("nan_mid")
        middle = s // 16 + 1
        assert (s + length - 1) // 16 == middle + 1
        assert set(range(middle * 16, middle * 16 + 16)) <= set(t.nan_positions.tolist())
        assert s not in t.nan_positions and s + length - 1 not in t.nan_positions
        s, length = t.start("nan_all"), t.length("nan_all")
        assert set(range(s, s + length)) <= set(t.nan_positions.tolist()) and (s + length - 1) // 16 > s // 16
        v = sc.sorted_values(t, "bytes_nan", 3)
        assert np.isnan(v[t.nan_positions]).all() and np.isnan(v).sum() == 3 * len(t.nan_positions) + 1


def test_turns_layout():
    (t,) = sc.turns()
    heads = np.zeros(t.n, dtype=bool)
    heads[t.starts] = True
    assert set(list(range(1, 18)) + [64, 65, 600, 1100]) <= set(t.lengths.tolist())
    for length in sc.LANE63_LENGTHS:                          # a head on lane 63 of a group, one run of each file class
        assert t.start(f"lane63_{length}") % 64 == 63 and t.length(f"lane63_{length}") == length
    for shortest, want in sc.CAPACITY_HEADS.items():          # capacity turns from a turn boundary
        s = t.start(f"cap{shortest}")
        assert s % sc.RZ_MED_TURN == 0
        in_turn = t.lengths[(t.starts >= s) & (t.starts < s + sc.RZ_MED_TURN)]
        assert len(in_turn) == want and (in_turn == shortest).all()
        assert want <= sc.FILE_CAPACITY[shortest]
    classes = ((1, 2), (3, 4), (5, 8), (9, 16), (17, 1 << 30))
    ends = t.starts + t.lengths - 1
    for lo, hi in classes:                                    # of every class: across a group boundary, across a turn boundary
        of_class = (t.lengths >= lo) & (t.lengths <= hi)
        assert (of_class & (t.starts // 64 != ends // 64)).any()
        assert (of_class & (t.starts // sc.RZ_MED_TURN != ends // sc.RZ_MED_TURN)).any()
    assert t.start("turn_cross_2") % sc.RZ_MED_TURN == sc.RZ_MED_TURN - 1
    turn_heads = np.add.reduceat(heads.astype(int), np.arange(0, t.n, sc.RZ_MED_TURN))
    assert (turn_heads == 0).any()                            # a turn that a run covers whole: no head in it
    s = t.start("whole_turn")
    assert (s + t.length("whole_turn") - 1) // sc.RZ_MED_TURN - s // sc.RZ_MED_TURN >= 2
    assert t.start("last_long") + t.length("last_long") == t.n and t.length("last_long") > 16
    three = [t.start(f"three_{k}") for k in "abc"]
    assert len({s // sc.RZ_MED_TURN for s in three}) == 1 and all(t.length(f"three_{k}") > 16 for k in "abc")
    assert (t.start("three_c") + t.length("three_c") - 1) // sc.RZ_MED_TURN == three[0] // sc.RZ_MED_TURN
    between = t.lengths[t.marks["three_a"] + 1:t.marks["three_b"]].tolist() + t.lengths[t.marks["three_b"] + 1:t.marks["three_c"]].tolist()
    assert between and max(between) <= 16
    # the bytes: medians 0, 255 and x.5 in every class; the middle pair 3 | 4 and 251 | 252 (adjacent lanes' bins: four to a lane)
    v = sc.sorted_values(t, "bytes", 3)
    med = lambda name: np.median(v[t.start(name):t.start(name) + t.length(name)], axis=0)       # noqa: E731
    for length in (1, 2, 3, 4, 6, 8, 12, 16, 40):
        assert (med(f"zero{length}") == 0).all() and (med(f"full{length}") == 255).all()
    for length in (2, 4, 8, 16, 40):
        assert (med(f"half{length}") == 10.5).all()
    for name, lo, hi in (("mid34", 3, 4), ("mid251", 251, 252)):
        run = np.sort(v[t.start(name):t.start(name) + t.length(name)], axis=0)
        k = t.length(name)
        assert (run[k // 2 - 1] == lo).all() and (run[k // 2] == hi).all() and lo // 4 + 1 == hi // 4
    run = v[t.start("const"):t.start("const") + t.length("const")]
    assert (run == run[0, 0]).all() and t.length("const") > 16


def test_kahan_layout_and_the_cancellation_run():
    (t,) = sc.kahan()
    for length in sc.KAHAN_LENGTHS:
        assert t.length(f"len{length}") == length
    assert t.inf_positions.tolist() == [t.start("inf7") + 7, t.start("inf8") + 8]
    assert t.length("inf7") == 17 and t.length("inf8") == 17
    v = sc.sorted_values(t, "kahan", 2)
    s = t.start("cancellation")
    np.testing.assert_array_equal(v[s:s + 9, 1], sc.CANCELLATION)
    assert np.isinf(v[t.inf_positions]).all()
    # the handed-over rows come back in sorted-position order under a stable sort
    np.testing.assert_array_equal(sc.values(t, "kahan", 2)[t.order], v)
    # the oracle's mean of the run depends on the order of its rows, at float32
    x, y, _ = sc.one_cell_table(9)

    def mean(run):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return orc.rasterize_points(x, y, run[:, None], 1.0, False, 1.0, "mean", 255, return_float=True)[0][0, 0, 0]

    in_rows, in_order, backwards = mean(sc.CANCELLATION), mean(np.sort(sc.CANCELLATION)), mean(sc.CANCELLATION[::-1])
    print(in_rows, in_order, backwards)
    assert in_rows.dtype == np.float32 and in_rows != in_order and in_rows != backwards
    assert in_rows == np.float32(2.1111112) and in_order == np.float32(2.0)


def test_value_kinds_are_what_the_device_checks_look_for():
    (t,) = sc.turns()
    is_f32 = lambda a: (a.astype(np.float32).astype(np.float64) == a) | np.isnan(a)      # noqa: E731
    b = sc.sorted_values(t, "bytes", 4)
    assert (b == np.floor(b)).all() and b.min() == 0 and b.max() == 255
    bn = sc.sorted_values(t, "bytes_nan", 4)
    assert np.isnan(bn).sum() == 1 and np.nanmax(bn) == 255
    u = sc.sorted_values(t, "u16", 3)
    assert (u == np.floor(u)).all() and u.max() == 65535 and (u > 255).mean() > 0.3 and (u <= 255).mean() > 0.3
    f = sc.sorted_values(t, "f32", 4)
    assert is_f32(f).all() and (f < 0).any() and np.isposinf(f).any() and np.isneginf(f).any()
    zeros = f[:, 0] == 0
    assert zeros.sum() == 2 and sorted(np.signbit(f[zeros, 0]).tolist()) == [False, True]
    assert len(set(t.sorted_cells[zeros].tolist())) == 2                 # one zero per run
    assert not is_f32(sc.sorted_values(t, "f53", 3)).any()


def test_tail_cases():
    sizes = {(w, h) for w, h, _, _ in sc.TAIL_CASES.values()}
    assert sizes == {(64, 32), (65, 33), (63, 31), (73, 41), (2, 40)}
    seen = set()
    for name, (w, h, cells, nb) in sc.TAIL_CASES.items():
        table, v = sc.tail_case(name)
        assert table.size == (w, h) and v.shape == (table.n, nb)
        assert w * h * nb * 9 <= 3000 * 2 * 9
        assert (v < 0).any() or (v > 255).any()
        seen |= set(sc.window_counts(table).tolist())
        pair = v[table.order][table.starts[np.flatnonzero(table.lengths == 2)[0]]:][:2]
        assert (pair == [[10.0] * nb, [13.0] * nb]).all()
    assert set(range(1, 9)) <= seen                                     # an empty centre sees at most eight values
    for row, col in ((31, 63), (31, 64), (32, 63), (32, 64)):           # each on its own; the two tiles beside it stay empty
        table, _ = sc.tail_case(f"73x41_corner_r{row}c{col}_a")
        rows, cols = np.divmod(np.unique(table.cells), 73)
        assert sorted(zip(rows.tolist(), cols.tolist())) == sorted([(0, 0), (40, 72), (row, col)])
    # the ring whose mean depends on the order of its sum, at byte level
    table, v = sc.tail_case("64x32_sum_order")
    w = np.zeros(9)
    w[[0, 1, 2, 3, 5, 6, 7, 8]] = [sc.TAIL_EXPLICIT["64x32_sum_order"][(9 + k // 3, 20 + k % 3)] for k in (0, 1, 2, 3, 5, 6, 7, 8)]
    ring = v[table.order][np.isin(table.sorted_cells, [(9 + k // 3) * 64 + 20 + k % 3 for k in (0, 1, 2, 3, 5, 6, 7, 8)]), 0]
    np.testing.assert_array_equal(ring, w[[0, 1, 2, 3, 5, 6, 7, 8]])
    assert (w.astype(np.float32) == w).all()
    left_to_right = 0.0
    for value in w:
        left_to_right += value
    assert int(np.float32(np.sum(w) / 8)) == 20 and int(np.float32(left_to_right / 8)) == 19
    table, _ = sc.tail_case("73x41_reach")
    rows, cols = np.divmod(np.unique(table.cells), 73)
    have = set(zip(rows.tolist(), cols.tolist()))
    for s in (1, 2, 7, 8):                                              # S and S + 1 cells from the tile edges
        assert {(r, c) for r, c in have if c == 64 - s} and {(r, c) for r, c in have if c == 64 - s - 1}
        assert (32 - s, 66) in have and (32 - s - 1, 70) in have
        assert {(r, c) for r, c in have if r == 31 + s} and {(r, c) for r, c in have if r == 31 + s + 1}


def test_sparse_tiles_table():
    t = sc.sparse_tiles_table(5, 4)
    assert t.size == (320, 128) and t.n == 20
    rows, cols = np.divmod(t.cells, 320)
    assert sorted(((rows // 32) * 5 + cols // 64).tolist()) == list(range(20))      # one point per tile
    assert len({(r % 32, c % 64) for r, c in zip(rows.tolist(), cols.tolist())}) >= 18


def test_the_tails_float_multiply_division_is_exact():
    """rz_tail_kernel splits an LDS index into row and column as int((idx + 0.5f) * (1.0f / w)): exact for every width it
    uses -- lw = 64 + 2 S and every lw - 2 (s + 1), S from 0 to 8 -- over the whole LDS extent"""
    tail = _src("rasterize_tail.h")
    assert "const int r = (int)(((float)idx + 0.5f) * inv_lw), c = idx - r * lw;" in tail
    assert "int r = (int)(((float)idx + 0.5f) * inv_rw), c = idx - r * rw;" in tail
    checked = 0
    for S in range(sc.RZ_SMAX + 1):
        lw, lh = sc.RZ_TW + 2 * S, sc.RZ_TH + 2 * S
        assert sc.tail_index_split_mismatches(lw, lw * lh) == 0
        for s in range(S):
            rw, rh = lw - 2 * (s + 1), lh - 2 * (s + 1)
            assert sc.tail_index_split_mismatches(rw, rw * rh) == 0
            checked += 1
    assert checked == 36 and (sc.RZ_TW + 16) * (sc.RZ_TH + 16) == 3840
