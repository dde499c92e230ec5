"""Tables that put the rasterisation kernels (alproj_amd/csrc/rasterize_runs.h, rasterize_median.h, rasterize_tail.h) on
their internal seams on purpose.  HIP-free: numpy only; tests/test_rasterize_seam_cases.py asserts on the CPU that every
layout does what it says, tests/test_gpu_rasterize_seams.py holds the kernels to the oracle on them.

The cell sort is stable and keyed by ``row * width + col``, so a table built run by run has a known sorted layout: the
head of run r sits at sorted position ``sum(lengths[:r])``.  Rows are handed over in a fixed-seed permutation, never in
cell order, so that the stable sort and the row-order Kahan mean have something to preserve; band values are made in
SORTED order (``Table.scatter`` puts the value of sorted position p into the row that the stable sort brings there)."""
import functools

import numpy as np

# what the cases are built for (test_rasterize_seam_cases.py reads the same constants from the headers)
RZ_SEG = 16
RZ_MED_GROUPS = 8
RZ_MED_TURN = RZ_MED_GROUPS * 64
RZ_TW, RZ_TH, RZ_SMAX = 64, 32, 8
RZ_TILE_BITS = 20
FILE_CAPACITY = {1: RZ_MED_TURN, 3: RZ_MED_TURN // 3 + 4, 5: RZ_MED_TURN // 5 + 4, 9: RZ_MED_TURN // 9 + 4, 17: RZ_MED_TURN // 17 + 4}
# the most heads of runs of that length a turn can hold, the run that leaves the turn included
CAPACITY_HEADS = {1: 512, 3: 171, 5: 103, 9: 57, 17: 31}

# pandas' Kahan mean of this run depends on the order of its rows at float32 level: 2.1111112 in this order, 2.0 sorted
# by value, 2.2222223 reversed
CANCELLATION = np.array([1e16, 3.0, -1e16, 5.0, 1e16, 7.0, -1e16, 2.0, 1.0])

AGGS = ("mean", "max", "min", "median")


def cells_of(x, y, size):
    """row * width + col of every point by the reference's formula (project.py:435-436, oracle/ref_numpy.py:351-352) at
    resolution 1, the extent taken from the table as the reference does (project.py:420-425)"""
    width, height = size
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    x_min, x_max, y_min, y_max = x.min(), x.max(), y.min(), y.max()
    assert int(np.ceil(x_max - x_min)) == width and int(np.ceil(y_max - y_min)) == height, "the table does not span the raster"
    col = ((x - x_min) / 1.0).astype(int).clip(0, width - 1)
    row = ((y_max - y) / 1.0).astype(int).clip(0, height - 1)
    return row * width + col


def table_from_runs(lengths, width, seed=0):
    """x, y, (width, height): run r has lengths[r] points in cell r of a raster `width` wide (0: the cell stays empty).
    Cells on the raster's rim put their points ON the rim (x = 0 in column 0, x = width in the last column, y = height in
    row 0, y = 0 in the last row), the interior uses cell centres: the reference's own ceil(max - min) extent and its clip
    reproduce exactly this raster, no anchor points added.  Rows come in a fixed-seed permutation."""
    lengths = np.asarray(lengths, dtype=np.int64)
    ncell = len(lengths)
    height = -(-ncell // width)
    assert width >= 2 and height >= 2, "one-cell rasters: one_cell_table"
    cell = np.repeat(np.arange(ncell), lengths)
    row, col = np.divmod(cell, width)
    assert (row == 0).any() and (row == height - 1).any() and (col == 0).any() and (col == width - 1).any(), \
        "every rim row and rim column needs a non-empty cell"
    x = np.where(col == 0, 0.0, np.where(col == width - 1, float(width), col + 0.5))
    y = np.where(row == 0, float(height), np.where(row == height - 1, 0.0, height - row - 0.5))
    perm = np.random.default_rng(seed).permutation(len(cell))
    x, y = np.ascontiguousarray(x[perm]), np.ascontiguousarray(y[perm])
    realised = np.bincount(cells_of(x, y, (width, height)), minlength=ncell)
    assert len(realised) == ncell and (realised == lengths).all(), "the realised per-cell counts are not `lengths`"
    return x, y, (width, height)


def one_cell_table(n, seed=0):
    """all n points in the one cell of a 1 x 1 raster: spread over the closed unit square, both corners present"""
    assert n >= 2
    rng = np.random.default_rng(seed)
    x, y = rng.random(n), rng.random(n)
    a, b = rng.choice(n, 2, replace=False)
    x[a], y[a], x[b], y[b] = 0.0, 0.0, 1.0, 1.0
    assert (cells_of(x, y, (1, 1)) == 0).all()
    return x, y, (1, 1)


class Table:
    """a table with its sorted layout: `starts[r]` the sorted position of run r's head (empty cells left out of the runs),
    `marks[name]` the run a layout named, `order` the stable cell sort of the handed-over rows"""

    def __init__(self, name, x, y, size, marks=None, forced=None, nan_positions=(), inf_positions=(), cancel_start=None):
        self.name, self.x, self.y, self.size = name, x, y, size
        self.n = len(x)
        self.cells = cells_of(x, y, size)
        self.order = np.argsort(self.cells, kind="stable")
        self.sorted_cells = self.cells[self.order]
        heads = np.flatnonzero(np.r_[True, self.sorted_cells[1:] != self.sorted_cells[:-1]])
        self.starts = heads
        self.lengths = np.diff(np.r_[heads, self.n])
        self.marks = dict(marks or {})
        self.forced = dict(forced or {})
        self.nan_positions = np.asarray(sorted(nan_positions), dtype=np.int64)
        self.inf_positions = np.asarray(sorted(inf_positions), dtype=np.int64)
        self.cancel_start = cancel_start

    def start(self, name):
        return int(self.starts[self.marks[name]])

    def length(self, name):
        return int(self.lengths[self.marks[name]])

    def scatter(self, sorted_values):
        """values made for the sorted positions -> the rows as they are handed over"""
        out = np.empty_like(sorted_values)
        out[self.order] = sorted_values
        return out


class _Runs:
    """a layout under construction: runs appended one after the other, padded so that the stated offsets hold"""

    def __init__(self):
        self.lengths, self.pos = [], 0
        self.marks, self.forced, self.nan, self.inf, self.cancel = {}, {}, [], [], None

    def run(self, length, name=None, force=None):
        r = len(self.lengths)
        if name:
            assert name not in self.marks
            self.marks[name] = r
        if force:
            self.forced[r] = force
        self.lengths.append(int(length))
        start = self.pos
        self.pos += int(length)
        return start

    def align(self, offset, modulus, filler=7):
        """filler runs (of at most `filler` points) until the next head sits at `offset` mod `modulus`"""
        gap = (offset - self.pos) % modulus
        while gap:
            k = min(gap, filler)
            self.run(k)
            gap -= k

    def table(self, name, width, seed=0):
        x, y, size = table_from_runs(self.lengths, width, seed)
        return Table(name, x, y, size, self.marks, self.forced, self.nan, self.inf, self.cancel)


SEGMENT_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 48)
SEGMENT_OFFSETS = (0, 1, 15)


def _segments_runs():
    b = _Runs()
    for length in SEGMENT_LENGTHS:
        for off in SEGMENT_OFFSETS:
            b.align(off, RZ_SEG)
            b.run(length, f"len{length}@{off}")
    for k in (1, 2, 4):                       # fills k segments exactly, behind a run that ends on the boundary
        b.align(0, RZ_SEG)
        b.run(k * RZ_SEG, f"fill{k}")
    for m in range(1, 10):                    # head in one segment, tail over the m following ones
        b.align(8, RZ_SEG)
        b.run(8 + RZ_SEG * (m - 1) + 5, f"tail{m}")
    b.align(8, RZ_SEG)
    s = b.run(8 + RZ_SEG + 8, "nan_mid")      # its piece in the middle segment is all NaN
    b.nan += list(range(s + 8, s + 8 + RZ_SEG))
    b.align(8, RZ_SEG)
    s = b.run(8 + RZ_SEG + 4, "nan_all")      # every value NaN: the cell stays NaN
    b.nan += list(range(s, s + 8 + RZ_SEG + 4))
    b.run(3)
    return b


@functools.lru_cache(maxsize=None)
def segments():
    """rz_pieces_kernel / rz_join_kernel: tables of n % 16 = 0, 1, 15 over the same runs, a table of n < 16, one cell of 1000"""
    tables = []
    for mod in (0, 1, 15):
        b = _segments_runs()
        b.align(mod, RZ_SEG)
        if b.pos % RZ_SEG != mod or b.lengths[-1] == 0:
            raise AssertionError("segments: the table's length is off")
        tables.append(b.table(f"n%16={mod}", 12, seed=mod))
    x, y, size = table_from_runs([3, 1, 2, 4, 2, 1], 3, seed=3)
    tables.append(Table("n<16", x, y, size))
    x, y, size = one_cell_table(1000, seed=4)
    tables.append(Table("one_cell", x, y, size))
    return tuple(tables)


LANE63_LENGTHS = (2, 4, 8, 16, 17)            # one run of each file class: 1-2, 3-4, 5-8, 9-16, longer


@functools.lru_cache(maxsize=None)
def turns():
    """rz_median_packed_kernel: groups of 64 positions, turns of 512, five files by run length"""
    b = _Runs()
    # capacity turns, each from a turn boundary; the space behind each is used for the other cases
    b.run(1, "cap1")
    for _ in range(511):
        b.run(1)
    b.run(3, "cap3")                          # 171 heads: the 171st run leaves the turn (a 3-4 run across a turn boundary)
    for _ in range(170):
        b.run(3)
    for length in list(range(1, 18)) + [64, 65]:
        b.run(length, f"every{length}")
    b.align(0, RZ_MED_TURN, filler=16)
    b.run(5, "cap5")                          # 103 heads, the last across the boundary (5-8)
    for _ in range(102):
        b.run(5)
    for length in LANE63_LENGTHS:             # a head on lane 63 of a group: the run crosses the group boundary
        b.align(63, 64)
        b.run(length, f"lane63_{length}")
    b.align(0, RZ_MED_TURN, filler=16)
    b.run(9, "cap9")                          # 57 heads, the last across the boundary (9-16)
    for _ in range(56):
        b.run(9)
    b.run(40, "three_a")                      # three long runs in one turn, short runs between them
    b.run(3)
    b.run(100, "three_b")
    b.run(1)
    b.run(1)
    b.run(64, "three_c")
    b.run(5)
    for length in (1, 2, 3, 4, 6, 8, 12, 16, 40):
        b.run(length, f"zero{length}", force="zero")
        b.run(length, f"full{length}", force="full")
    b.align(0, RZ_MED_TURN, filler=16)
    b.run(17, "cap17")                        # 31 heads, the last across the boundary (longer)
    for _ in range(30):
        b.run(17)
    for length in (2, 4, 8, 16, 40):
        b.run(length, f"half{length}", force="half")
    b.run(100, "mid34", force="mid34")        # the two middle values in adjacent lanes' bins: 3 | 4 and 251 | 252
    b.run(100, "mid251", force="mid251")
    b.run(90, "const", force="const")
    b.run(101, "odd_long")
    b.run(1100, "whole_turn")                 # covers a whole turn: that turn has no head
    b.run(600, "long600")
    b.align(RZ_MED_TURN - 1, RZ_MED_TURN, filler=16)
    b.run(2, "turn_cross_2")                  # a 1-2 run across a turn boundary
    b.run(4)
    b.run(70, "last_long")                    # a long run ending at n - 1
    return (b.table("turns", 33, seed=7),)


KAHAN_LENGTHS = (7, 8, 9, 15, 16, 17)


@functools.lru_cache(maxsize=None)
def kahan():
    """rz_runs_kernel's eight-at-a-time walk"""
    b = _Runs()
    for length in KAHAN_LENGTHS:
        b.run(2)
        b.run(length, f"len{length}")
    s = b.run(17, "inf7")                     # the compensation reset on the last value of a batch of eight ...
    b.inf.append(s + 7)
    b.run(1)
    s = b.run(17, "inf8")                     # ... and on the first of the next
    b.inf.append(s + 8)
    b.cancel = b.run(len(CANCELLATION), "cancellation")
    for length in (3, 24, 1, 5, 33, 2):
        b.run(length)
    return (b.table("kahan", 5, seed=11),)


LAYOUTS = {"segments": segments, "turns": turns, "kahan": kahan}

# (value kind, bands) of the aggregate matrix: the kinds that reach each kernel, band counts 1, 3, 4 and 5 = 4 + 1
VALUE_PLAN = (("bytes", 1), ("bytes", 3), ("bytes", 4), ("bytes", 5), ("bytes_nan", 1), ("bytes_nan", 4), ("u16", 3),
              ("f32", 1), ("f32", 4), ("f32", 5), ("f53", 1), ("f53", 3))
KINDS = ("bytes", "bytes_nan", "u16", "f32", "f53", "kahan")


def value_plan(layout):
    return VALUE_PLAN + ((("kahan", 1), ("kahan", 5)) if layout == "kahan" else ())


def _force(v, s, length, pattern, rng):
    nb = v.shape[1]
    half = length // 2
    if pattern == "zero":
        v[s:s + length] = 0.0
    elif pattern == "full":
        v[s:s + length] = 255.0
    elif pattern == "const":
        v[s:s + length] = 77.0
    elif pattern == "half":                   # an even run: median x.5
        assert length % 2 == 0
        block = np.r_[np.full(half, 10.0), np.full(half, 11.0)]
        v[s:s + length] = rng.permutation(block)[:, None]
    elif pattern in ("mid34", "mid251"):
        assert length % 2 == 0
        lo_top, hi_bottom = (3, 4) if pattern == "mid34" else (251, 252)
        lower = rng.integers(0, lo_top + 1, (half, nb)).astype(np.float64)
        upper = rng.integers(hi_bottom, 256, (half, nb)).astype(np.float64)
        lower[0], upper[0] = lo_top, hi_bottom
        v[s:s + length] = rng.permutation(np.concatenate([lower, upper]))
    else:
        raise ValueError(pattern)


def sorted_values(table, kind, nb, seed=0):
    """band values (n, nb) for the SORTED positions of `table`:
    bytes       integers in [0, 255], the extremes 0 and 255 sprinkled and forced into the runs the layout chose
    bytes_nan   the same with NaN: the layout's whole segments and runs, and one NaN of its own
    u16         integers up to 65535, half of them above 255
    f32         float32-valued floats, negatives included, -0.0, +0.0, +inf and -inf each at the head of a run of its own
                (one zero per run: which of two equal zeros a median picks is not defined), the layout's NaN and infinities
    f53         53-bit fractions that no float32 holds
    kahan       f32 plus the layout's cancellation run"""
    rng = np.random.default_rng([seed, nb, KINDS.index(kind), table.n])
    n = table.n
    if kind in ("bytes", "bytes_nan"):
        v = rng.integers(0, 256, (n, nb)).astype(np.float64)
        k = max(2, n // 40)
        v[rng.integers(0, n, k), rng.integers(0, nb, k)] = 0.0
        v[rng.integers(0, n, k), rng.integers(0, nb, k)] = 255.0
        for r, pattern in table.forced.items():
            _force(v, int(table.starts[r]), int(table.lengths[r]), pattern, rng)
        if kind == "bytes_nan":
            v[n // 3, nb - 1] = np.nan
    elif kind == "u16":
        v = np.where(rng.random((n, nb)) < 0.5, rng.integers(0, 256, (n, nb)), rng.integers(256, 65536, (n, nb))).astype(np.float64)
        v[0, 0], v[n - 1, nb - 1] = 65535.0, 256.0
    elif kind in ("f32", "kahan"):
        v = rng.uniform(-300.0, 300.0, (n, nb)).astype(np.float32).astype(np.float64)
        if len(table.starts) >= 8:
            runs = rng.choice(len(table.starts), 4, replace=False)
            for r, special in zip(runs, (-0.0, 0.0, np.inf, -np.inf)):
                v[table.starts[r]] = special
        else:
            v[0] = -0.0
            v[n // 2] = np.inf
    elif kind == "f53":
        v = rng.uniform(-300.0, 300.0, (n, nb))
        assert (v.astype(np.float32).astype(np.float64) != v).mean() > 0.9
    else:
        raise ValueError(kind)
    if kind in ("bytes_nan", "f32", "kahan", "f53") and len(table.nan_positions):
        v[table.nan_positions] = np.nan
    if kind in ("f32", "kahan") and len(table.inf_positions):
        v[table.inf_positions] = np.inf
    if kind == "kahan":
        v[table.cancel_start:table.cancel_start + len(CANCELLATION)] = CANCELLATION[:, None]
    return v


def values(table, kind, nb, seed=0):
    """the rows' band values as they are handed over"""
    return np.ascontiguousarray(table.scatter(sorted_values(table, kind, nb, seed)))


# ---------------------------------------------------------------------------------------------- the tail
# tiles of 64 x 32 cells, a halo of S <= 8.  A case: raster size, {(row, col): points}, bands.  Every raster stays at or
# under 3 000 cells: the oracle's generic_filter costs about 17 us per cell, sweep and band.
TAIL_SWEEPS = (0, 1, 2, 7, 8)
NODATA = (255, 0, 7)


def _blob(r0, c0):
    """a 7 x 7 patch that leaves NaN cells with 1 to 8 values in their 3 x 3 window after the first sweep's look: a ring
    around a hole (8), a pair of holes, notches in the rim and a detached cell"""
    cells = {}
    for r in range(5):
        for c in range(5):
            cells[(r0 + r, c0 + c)] = 1 + (r + c) % 3
    for rc in ((1, 1), (1, 4), (3, 2), (3, 3), (3, 4)):
        del cells[(r0 + rc[0], c0 + rc[1])]
    cells[(r0 + 6, c0 + 6)] = 2
    return cells


def _tail_cells():
    corner_a = lambda w, h: {(0, 0): 1, (h - 1, w - 1): 1}             # noqa: E731  rim points in the first and the last tile
    corner_b = lambda w, h: {(0, w - 1): 1, (h - 1, 0): 1}             # noqa: E731  ... in the two other corners
    cases = {}
    cases["64x32_blob"] = (64, 32, {**corner_a(64, 32), **_blob(12, 28), (31, 0): 2, (0, 63): 3}, 1)
    cases["65x33_diagonal"] = (65, 33, {**corner_a(65, 33), (31, 63): 2, (32, 64): 1, (20, 64): 2, (32, 10): 3}, 2)
    cases["63x31_edges"] = (63, 31, {**corner_b(63, 31), **_blob(24, 56), (0, 30): 2, (15, 62): 2, (30, 31): 1, (14, 0): 2}, 1)
    for row, col in ((31, 63), (31, 64), (32, 63), (32, 64)):          # one cell at the corner where four tiles meet
        cases[f"73x41_corner_r{row}c{col}_a"] = (73, 41, {**corner_a(73, 41), (row, col): 2}, 1)
    for row, col in ((31, 63), (31, 64), (32, 63), (32, 64)):          # ... with the diagonally opposite tile empty
        cases[f"73x41_corner_r{row}c{col}_b"] = (73, 41, {**corner_b(73, 41), (row, col): 2}, 1)
    reach = dict(corner_a(73, 41))
    for k, s in enumerate((1, 2, 7, 8)):                               # S and S + 1 cells from the tile edges (column 63 | 64, row 31 | 32)
        reach[(2 + 9 * k, 64 - s)] = 2
        reach[(6 + 9 * k, 64 - s - 1)] = 1
        reach[(32 - s, 66)] = 2
        reach[(32 - s - 1, 70)] = 1
        reach[(31 + s, 3 + 14 * k)] = 1
        reach[(31 + s + 1, 9 + 14 * k)] = 2
    cases["73x41_reach"] = (73, 41, reach, 1)
    ring = {(9 + r, 20 + c): 1 for r in range(3) for c in range(3) if (r, c) != (1, 1)}
    cases["64x32_sum_order"] = (64, 32, {**corner_a(64, 32), **ring, (20, 40): 2}, 1)
    cases["2x40_narrow"] = (2, 40, {(0, 0): 2, (39, 1): 1, (31, 1): 2, (32, 0): 1, (12, 0): 3}, 2)
    return cases


TAIL_CASES = _tail_cells()
# a ring whose 3 x 3 mean depends on the order of the sum at BYTE level: numpy's pairwise order (a block of eight, then the
# ninth) gives 160 / 8 = 20.0, left to right 158 / 8 = 19.75
_BIG = float(np.float32(1e16))
TAIL_EXPLICIT = {"64x32_sum_order": dict(zip([(9 + r, 20 + c) for r in range(3) for c in range(3) if (r, c) != (1, 1)],
                                             [_BIG, 53.0, 48.0, -_BIG, 25.0, _BIG, 34.0, -_BIG]))}


@functools.lru_cache(maxsize=None)
def tail_case(name):
    """-> (Table, values (n, bands)): quarter steps from -40 to 300 (non-integer means, values under 0 and over 255 for the
    clip), and in one two-point cell the pair 10, 13 (mean and median 11.5: the truncation shows)"""
    width, height, cells, nb = TAIL_CASES[name]
    lengths = np.zeros(width * height, dtype=np.int64)
    for (row, col), count in cells.items():
        assert 0 <= row < height and 0 <= col < width, (name, row, col)
        lengths[row * width + col] = count
    x, y, size = table_from_runs(lengths, width, seed=len(name))
    table = Table(name, x, y, size)
    rng = np.random.default_rng(len(name) + 100 * width)
    v = rng.integers(-160, 1201, (table.n, nb)) / 4.0
    pair = np.flatnonzero(table.lengths == 2)[0]
    others = np.setdiff1d(np.arange(table.n), [table.starts[pair], table.starts[pair] + 1])
    v[others[0]], v[others[-1]] = -12.25, 280.5
    v[table.starts[pair]], v[table.starts[pair] + 1] = 10.0, 13.0
    for (row, col), value in TAIL_EXPLICIT.get(name, {}).items():
        v[table.starts[np.flatnonzero(table.sorted_cells[table.starts] == row * width + col)[0]]] = value
    return table, np.ascontiguousarray(table.scatter(v))


def window_counts(table):
    """how many of the 3 x 3 neighbours of every EMPTY cell hold points (the first sweep's window counts)"""
    width, height = table.size
    used = np.zeros((height + 2, width + 2), dtype=np.int64)
    rows, cols = np.divmod(np.unique(table.cells), width)
    used[rows + 1, cols + 1] = 1
    total = sum(used[1 + dr:height + 1 + dr, 1 + dc:width + 1 + dc] for dr in (-1, 0, 1) for dc in (-1, 0, 1))
    return total[used[1:-1, 1:-1] == 0]


def sparse_tiles_table(tiles_x, tiles_y):
    """one point in every tile of a tiles_x x tiles_y raster, at a different in-tile position each (the first and the last
    tile: the raster's corners, which fix the extent)"""
    width, height = tiles_x * RZ_TW, tiles_y * RZ_TH
    t = np.arange(tiles_x * tiles_y)
    ty, tx = np.divmod(t, tiles_x)
    row = ty * RZ_TH + (7 * t + 3) % RZ_TH
    col = tx * RZ_TW + (11 * t + 5) % RZ_TW
    row[0], col[0], row[-1], col[-1] = 0, 0, height - 1, width - 1
    lengths = np.zeros(width * height, dtype=np.int64)
    lengths[row * width + col] = 1
    x, y, size = table_from_runs(lengths, width, seed=1)
    return Table("sparse_tiles", x, y, size)


def tail_index_split_mismatches(lw, extent):
    """the tail's division by a float multiply, in float32 numpy: idx / lw as int((idx + 0.5f) * (1.0f / lw)), idx < extent"""
    idx = np.arange(extent, dtype=np.int64)
    inv = np.float32(1.0) / np.float32(lw)
    got = ((idx.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)
    return int((got != idx // lw).sum())
