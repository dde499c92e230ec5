"""HIP-free: a plain float64 numpy statement of the mesh construction of the reference's get_colored_surface
(src/alproj/surface.py:175-193, 211-212 and _normalize_aerial, :44-66, then persp_proj's float32 cast, project.py:213-214),
the map of surface_zmin_kernel's launch (alp_mesh.hip) and the shapes, transforms and positions of the seam tests
(test_gpu_surface_seams.py).

The statement is pinned to what the REFERENCE returned (g11) by tests/test_surface_cases.py, which also holds the launch map
to an enumeration of the kernel's own loops, so the GPU tests compare the kernels with the reference project at sizes its
fixtures do not reach and name the slot of the launch that a case lands in."""
import numpy as np

WG_LANES = 256                       # surface_zmin_kernel: lanes per workgroup (four waves of 64)
WG_PER_CU = 4                        # alp_mesh_from_rasters: cu_count * 4 workgroups
PACK_BYTES = 16                      # one pack per lane and turn
TILE_W, TILE_H = 64, 16              # raster_plan.h: GT_W x GT_H grid cells per tile of the implicit-grid render


# ------------------------------------------------------------------ the operation
def clamped_z(dsm, z_max):
    """surface.py:175-176, in the DSM's own type as the reference does it, then the float64 of np.vstack (:189): a NaN and a
    -0.0 pass both assignments unchanged"""
    z = np.array(dsm, copy=True)
    z[z < 0] = 0
    z[z > z_max] = z_max
    return z.astype(np.float64)


def normalized(aerial, color_div):
    """_normalize_aerial (surface.py:44-66) on the three bands as (3, n): float64, one division by the divisor the reference
    would have chosen (``color_div`` 0: none, its "already normalized" branch), np.clip -- which keeps a NaN"""
    data = np.vstack((aerial[0], aerial[1], aerial[2])).reshape([3, -1]).astype(np.float64)      # :186-192
    if color_div > 0:
        data /= color_div
    np.clip(data, 0, 1, out=data)
    return data


def expected(dsm, transform, z_max, aerial, color_div, nodata=None):
    """-> (vert32 (n, 3) X Z Y, col32 (n, 3), valid (n,) bool, offsets (3,) float64) of rasters of any shape.  ``z_max`` is
    a value of the DSM's type, as surface.py:169 always passes.  One meshgrid, one (n, 3) float64 table."""
    dsm = np.asarray(dsm)
    rows, cols = dsm.shape
    zz = clamped_z(dsm, z_max)
    x = np.arange(0, cols) * transform[0] + transform[2]                   # :179
    y = np.arange(0, rows) * transform[4] + transform[5]                   # :180
    xx, yy = np.meshgrid(x, y)
    vert = np.vstack((xx, zz, yy)).reshape([3, -1])                        # :189
    offsets = vert.min(axis=1)                                             # :211 (on the table before its transpose)
    vert32 = np.transpose(vert - offsets[:, None]).astype(np.float32)      # :190, :212, project.py:213
    col32 = np.transpose(normalized(aerial, color_div)).astype(np.float32)  # :193, project.py:214
    valid = np.ones(rows * cols, dtype=bool) if nodata is None else ~np.asarray(nodata, dtype=bool).flatten()   # :203
    return np.ascontiguousarray(vert32), np.ascontiguousarray(col32), valid, offsets


# ------------------------------------------------------------------ the launch of surface_zmin_kernel
def pack_len(itemsize):
    return PACK_BYTES // itemsize


def turn_packs(cu_count):
    """T: the packs one turn of the grid-stride loop covers = gridDim.x * blockDim.x"""
    return cu_count * WG_PER_CU * WG_LANES


def zmin_slot(index, n, itemsize, cu_count):
    """(turn, workgroup, wave, in_tail) of the lane that reads element ``index`` of an n-element DSM.  The n % V elements
    after the last whole pack are read one per lane by the first lanes of workgroup 0 in the tail loop's only turn."""
    V = pack_len(itemsize)
    nv = n // V
    if not 0 <= index < n:
        raise IndexError(index)
    if index >= nv * V:
        return 0, 0, 0, True
    turn, g = divmod(index // V, turn_packs(cu_count))
    return turn, g // WG_LANES, (g % WG_LANES) // 64, False


def launch_enumeration(n, itemsize, cu_count):
    """the loops of surface_zmin_kernel as they are written, every lane of the grid at once: (n, 4) int64 rows
    (turn, workgroup, wave, in_tail) per element, -1 where no lane reads it"""
    V = pack_len(itemsize)
    nv = n // V
    gid = np.arange(turn_packs(cu_count), dtype=np.int64)          # blockIdx.x * blockDim.x + threadIdx.x
    wg, wave = gid // WG_LANES, (gid % WG_LANES) // 64
    stride = len(gid)
    out = np.full((n, 4), -1, dtype=np.int64)
    k, turn = gid.copy(), 0
    while (k < nv).any():                                          # for (k = gid; k < nv; k += stride)
        live = k < nv
        for j in range(V):
            out[k[live] * V + j] = np.stack([np.full(live.sum(), turn), wg[live], wave[live], np.zeros(live.sum(), np.int64)], 1)
        k, turn = k + stride, turn + 1
    i, turn = nv * V + gid, 0
    while (i < n).any():                                           # for (i = nv * V + gid; i < n; i += stride)
        live = i < n
        out[i[live]] = np.stack([np.full(live.sum(), turn), wg[live], wave[live], np.ones(live.sum(), np.int64)], 1)
        i, turn = i + stride, turn + 1
    return out


POSITIONS = ["first", "body_last", "tail_last", "wave1", "wave2", "wave3", "last_workgroup", "turn1", "turn2"]


def min_positions(n, itemsize, cu_count):
    """name -> element index for a single lowest elevation, one per slot of the launch that decides the result alone: the
    first element, the last of the vector body, the last of the scalar tail, one owned by each of waves 1, 2, 3 (in
    workgroups 5, 6, 7, which tiny rasters never fill), one in the last workgroup of the grid, one in the second and one in
    the third turn.  A name whose slot the raster does not have is left out."""
    V = pack_len(itemsize)
    nv, T = n // V, turn_packs(cu_count)
    packs = {"wave1": (5 * WG_LANES + 64 + 17, 1), "wave2": (6 * WG_LANES + 128 + 63, 2), "wave3": (7 * WG_LANES + 255, 3),
             "last_workgroup": (T - WG_LANES + 3, 0), "turn1": (T + 7 * WG_LANES + 70, 1), "turn2": (2 * T + 100, 0)}
    pos = {"first": 0}
    if nv:
        pos["body_last"] = nv * V - 1
    if n % V:
        pos["tail_last"] = n - 1
    for name, (k, j) in packs.items():
        if k < nv:
            pos[name] = k * V + j % V
    return pos


# ------------------------------------------------------------------ shapes
def seam_shape(itemsize, cu_count, turns=3, rem=1, cols=1021):
    """(rows, cols) with ``cols`` as given (odd) and the fewest rows for which the launch takes ``turns`` turns, the last
    with eight whole workgroups in it (the positions of ``min_positions`` reach into the eighth), and n % V == rem: n lies
    within 2048 * V + 4 * cols of (turns - 1) * T * V"""
    V = pack_len(itemsize)
    assert cols % 2 == 1 and 0 <= rem < V
    need = (turns - 1) * turn_packs(cu_count) * V + 8 * WG_LANES * V
    rows = -(-need // cols)
    while (rows * cols) % V != rem:          # cols is odd: four consecutive row counts take every remainder
        rows += 1
    return rows, cols


# (itemsize, n % V) -> the row width of that seam shape: odd, above 1000, one of them above 2048
SEAM_COLS = {(4, 1): 1021, (4, 2): 1531, (4, 3): 2049, (8, 1): 1023}
SMALL_SHAPES = [(2, 2), (2, 3), (3, 3)]      # n = 4, 6, 9: float32 n = V / a tail of 2 / two packs + 1; float64 no tail / a tail of 1


def seam_shapes(itemsize, cu_count, turns=3):
    """rem -> (rows, cols) for every remainder the type has a width for"""
    return {rem: seam_shape(itemsize, cu_count, turns, rem, cols) for (size, rem), cols in SEAM_COLS.items() if size == itemsize}


# ------------------------------------------------------------------ transforms (a, b, c, d, e, f) of a rows x cols raster
def transform(name, rows, cols):
    """north_up: e < 0 at UTM magnitude, 1 m; south_up: e > 0 (row 0 holds the y minimum); west_up: a < 0 (the LAST column
    holds the x minimum); half: 2.5 m cells from a fractional origin (products and sums still exact: 2.5 * c is a multiple of
    the origin's last bit); fine: 0.3 m cells, where (double)c * t0 and the sum with t2 both round in most columns"""
    x0, y0 = 732000.0, 4048000.0
    return {"north_up": (1.0, 0.0, x0, 0.0, -1.0, y0 + rows),
            "south_up": (2.0, 0.0, x0, 0.0, 2.0, y0),
            "west_up": (-1.0, 0.0, x0 + cols, 0.0, -1.0, y0 + rows),
            "half": (2.5, 0.0, x0 + 0.1, 0.0, -2.5, y0 + 0.7 + 2.5 * rows),
            "fine": (0.3, 0.0, x0 + 0.1, 0.0, -0.3, y0 + 0.7 + 0.3 * rows)}[name]


TRANSFORMS = ["north_up", "south_up", "west_up", "half", "fine"]


# ------------------------------------------------------------------ rasters
def terrain(rows, cols, dtype, seed, base=1500.0, noise=30.0):
    """base + uniform noise in [0, noise): every value strictly above ``base``"""
    rng = np.random.default_rng(seed)
    return (base + noise * rng.random((rows, cols))).astype(dtype)


def aerial_bands(rows, cols, dtype, seed, bands=3):
    rng = np.random.default_rng(seed + 1000)
    if np.dtype(dtype) == np.float32:
        return rng.random((bands, rows, cols), dtype=np.float32)
    return rng.integers(0, int(np.iinfo(dtype).max) + 1, (bands, rows, cols), dtype=dtype)


def tile_straddling_nodata(rows, cols):
    """(rows, cols) bool: blocks of nodata vertices across the 64-column and 16-row tile lines of the render, one across a
    tile corner, one on the raster's edge, and a sprinkle of single vertices"""
    m = np.zeros((rows, cols), dtype=bool)
    m[5:12, TILE_W - 6:TILE_W + 7] = True                          # across a column line, inside a tile row
    m[TILE_H - 3:TILE_H + 4, 20:40] = True                         # across a row line, inside a tile column
    m[3 * TILE_H - 5:3 * TILE_H + 6, 2 * TILE_W - 9:2 * TILE_W + 10] = True      # across a corner: four tiles
    m[7 * TILE_H - 1:7 * TILE_H + 1, :] |= np.arange(cols) % 7 == 0              # a dotted row line
    m[:, 3 * TILE_W - 1:3 * TILE_W + 1] |= (np.arange(rows) % 5 == 0)[:, None]   # a dotted column line
    m[rows - 9:, cols - 30:] = True                                # the last tile, partial in both directions
    m |= np.random.default_rng(17).random((rows, cols)) < 0.01
    return m
