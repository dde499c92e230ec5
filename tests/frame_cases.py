"""HIP-free: plain float64 numpy statements of what runs on a finished frame or around a mesh (raster_post.h), and the
frames, validity patterns and shapes of the seam tests (test_gpu_frame_seams.py, test_gpu_upload_seams.py).

The statements are pinned to what the REFERENCE produced (g12: reverse_proj's tables and sim_image's bytes) by
tests/test_frame_cases.py, so the GPU tests compare the kernels with the reference project and not with themselves."""
import numpy as np

COMPACT_CHUNK = 4096                 # raster_post.h: pixels per workgroup of valid_count_kernel / valid_write_kernel
SCAN_THREADS = 1024                  # scan_counts_kernel: one workgroup, per = ceil(chunks / 1024) chunks per thread
MAX_SIDE = 32768                     # alp_render_load: h, w <= 32768
UTM_OFFSETS = np.array([732000.0, 1655.0, 4048000.0])


# ------------------------------------------------------------------ the operations
def valid_table(raw, offsets=None, array=None):
    """reverse_proj's table (project.py:361-373) of the (h, w, 3) float32 frame ``raw``: -> idx (uint32, the row-major
    positions with channel 0 > 0), xyz (M, 3) float64 = channels (0, 2, 1) + offsets[[0, 2, 1]], u = idx % w and
    v = idx // w as int16 (numpy's wrapping cast), and the channels of ``array`` (h, w, C) there as float64 rows (C, M)."""
    h, w = raw.shape[:2]
    flat = raw.reshape(-1, 3)
    idx = np.flatnonzero(flat[:, 0] > 0).astype(np.uint32)
    off = np.zeros(3) if offsets is None else np.asarray(offsets, dtype=np.float64)
    xyz = flat[idx][:, [0, 2, 1]].astype(np.float64) + off[[0, 2, 1]]
    u = (idx % w).astype(np.int16)
    v = (idx // w).astype(np.int16)
    C = 0 if array is None else array.shape[-1]
    chan = np.empty((0, len(idx))) if C == 0 else array.reshape(-1, C)[idx].astype(np.float64).T
    return idx, xyz, u, v, chan


def valid_bounds(xyz):
    """(x_min, y_min, x_max, y_max) of the table as to_geotiff takes them (project.py:420-423: pandas' min / max skip NaN);
    four NaN for an empty table"""
    if len(xyz) == 0:
        return (np.nan,) * 4
    return (float(np.nanmin(xyz[:, 0])), float(np.nanmin(xyz[:, 1])), float(np.nanmax(xyz[:, 0])), float(np.nanmax(xyz[:, 1])))


def gather(raw, u, v, offsets=None):
    """set_gcp's lookup (gcp.py:644-648) in the frame: (n, 3) float64 x, y, z = channels (0, 2, 1) + offsets of the pixels
    (u[i], v[i]); NaN outside the image and where channel 0 is not > 0"""
    h, w = raw.shape[:2]
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    off = np.zeros(3) if offsets is None else np.asarray(offsets, dtype=np.float64)
    inside = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    px = raw[np.where(inside, v, 0), np.where(inside, u, 0)]
    ok = inside & (px[:, 0] > 0)
    out = np.full((len(u), 3), np.nan)
    out[ok] = px[ok][:, [0, 2, 1]].astype(np.float64) + off[[0, 2, 1]]
    return out


def image_u8(raw, scale=255.0, reverse=True):
    """sim_image's tail (project.py:322-324), (raw * scale).astype(uint8) as x86-64 numpy does it: the product in float32,
    truncated toward zero to int32 -- NaN and everything outside [-2^31, 2^31) give 0x80000000 -- and wrapped to 8 bits;
    ``reverse``: RGB -> BGR"""
    x = raw * np.float32(scale)
    assert x.dtype == np.float32
    with np.errstate(invalid="ignore"):
        ok = (x >= np.float32(-2147483648.0)) & (x < np.float32(2147483648.0))           # False for NaN
    q = np.where(ok, np.trunc(np.where(ok, x, 0)).astype(np.int64), -2147483648)
    out = (q & 0xFF).astype(np.uint8)
    return np.ascontiguousarray(out[:, :, ::-1] if reverse else out)


def distance_keep(xyz, cam, lo=None, hi=None):
    """filter_gcp_distance's mask (gcp.py:711-724) in numpy's evaluation order: rows with a NaN coordinate are dropped, the
    others kept when sqrt(dx^2 + dy^2 + dz^2) lies in [lo, hi] (None: no bound)"""
    with np.errstate(invalid="ignore"):
        d = np.sqrt((xyz[:, 0] - cam[0]) ** 2 + (xyz[:, 1] - cam[1]) ** 2 + (xyz[:, 2] - cam[2]) ** 2)
        keep = ~np.isnan(xyz).any(axis=1)
        if lo is not None:
            keep &= d >= lo
        if hi is not None:
            keep &= d <= hi
    return keep


def grid_triangles(gh, gw, dtype=np.int64):
    """the index array of the regular grid of gh rows and gw columns, surface.py:194-201: per cell a = row * gw + col the
    triangles (a, a + gw, a + gw + 1) and (a, a + gw + 1, a + 1), cells in row-major order"""
    a = (np.arange(gh - 1, dtype=dtype)[:, None] * dtype(gw) + np.arange(gw - 1, dtype=dtype)[None, :]).reshape(-1, 1)
    return (a + np.array([0, gw, gw + 1, 0, gw + 1, 1], dtype=dtype)[None, :]).reshape(-1, 3)


# ------------------------------------------------------------------ shapes
def chunks_of(npix):
    return (npix + COMPACT_CHUNK - 1) // COMPACT_CHUNK


def shape_of(npix):
    """(h, w) with h * w == npix and both sides within the frame limit, the most square one; None when npix has none"""
    for h in range(int(np.sqrt(npix)), 0, -1):
        if npix % h == 0:
            return (h, npix // h) if npix // h <= MAX_SIDE else None
    return None


def shape_at_least(npix):
    """the first pixel count >= npix that is a frame shape, and that shape (2^20 + 1 = 17 * 61681 is none, for one)"""
    while shape_of(npix) is None:
        npix += 1
    return shape_of(npix)


def shape_at_most(npix):
    while shape_of(npix) is None:
        npix -= 1
    return shape_of(npix)


# pixel counts around a wave (64), a pass of valid_write_kernel (256) and a chunk (4096)
SMALL_SHAPES = [(1, 1), (7, 9), (8, 8), (13, 5), (15, 17), (16, 16), (257, 1), (63, 65), (64, 64), (17, 241)]

# name -> (h, w).  Chunk counts 1023, 1024, 1025 (per = 1 -> 2 of scan_counts_kernel), 2048, 2049 (per = 2 -> 3), each
# with a full last chunk and with a last chunk of ONE pixel -- except 2049 chunks: 2048 * 4096 + 1 = 3 * 2796203 is no
# frame shape (2796203 is prime), its last chunk holds two pixels (3970 * 2113 = 2048 * 4096 + 2)
LARGE_SHAPES = {
    "c1023_full": (4092, 1024), "c1023_one": (1983, 2111),
    "c1024_full": (2048, 2048), "c1024_one": (2047, 2047),
    "c1025_full": (2050, 2048), "c1025_one": (2113, 1985),
    "c2048_full": (2048, 4096), "c2048_one": (277, 30269),
    "c2049_full": (4098, 2048), "c2049_two": (3970, 2113),
    "row_1x32768": (1, 32768), "column_32768x1": (32768, 1),
    "c1024_width_limit": (128, 32768),
}
LARGE_CHUNKS = {"c1023_full": (1023, 4096), "c1023_one": (1023, 1), "c1024_full": (1024, 4096), "c1024_one": (1024, 1),
                "c1025_full": (1025, 4096), "c1025_one": (1025, 1), "c2048_full": (2048, 4096), "c2048_one": (2048, 1),
                "c2049_full": (2049, 4096), "c2049_two": (2049, 2), "row_1x32768": (8, 4096), "column_32768x1": (8, 4096),
                "c1024_width_limit": (1024, 4096)}       # name -> (chunks, pixels of the last chunk)


# ------------------------------------------------------------------ frames
PATTERNS = ["none", "all", "first", "last", "first_of_last_chunk", "d0.001", "d0.5", "d0.999", "runs", "specials"]
# what sits in channel 0 of the `specials` frame at the borders of waves, passes and chunks: the reference keeps a pixel
# when numpy says x > 0 -- the subnormals and FLT_MIN are kept, the zeros, the negative subnormal, NaN and -inf are not
SPECIALS = np.array([0.0, -0.0, 1e-45, 1.17549435e-38, -1e-45, np.nan, np.inf, -np.inf], dtype=np.float32)


def validity(npix, pattern, rng):
    """bool (npix,): which pixels channel 0 makes valid under ``pattern`` (before the specials are placed)"""
    keep = np.zeros(npix, dtype=bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "first":
        keep[0] = True
    elif pattern == "last":
        keep[-1] = True
    elif pattern == "first_of_last_chunk":
        keep[(chunks_of(npix) - 1) * COMPACT_CHUNK] = True
    elif pattern.startswith("d"):
        keep = rng.random(npix, dtype=np.float32) < np.float32(pattern[1:])
    elif pattern == "runs":                       # 100 valid, 37 invalid: the runs straddle every power-of-two border
        keep = (np.arange(npix) % 137) < 100
    elif pattern == "specials":
        keep = rng.random(npix, dtype=np.float32) < np.float32(0.5)
    elif pattern != "none":
        raise ValueError(pattern)
    return keep


def special_positions(npix):
    """pixel positions on both sides of the first wave, pass and chunk borders and of the last chunk's start"""
    last = (chunks_of(npix) - 1) * COMPACT_CHUNK
    cand = [b + d for b in (0, 64, 128, 256, 512, COMPACT_CHUNK, 2 * COMPACT_CHUNK, last) for d in (-2, -1, 0, 1)]
    return np.array(sorted({p for p in cand if 0 <= p < npix}), dtype=np.int64)


def fill_channels(h, w, rng):
    """(h * w, 3) float32 frame body: channels 1 (elevation) and 2 (northing) random at UTM scale, channel 0 left to
    ``set_pattern``"""
    raw = np.empty((h * w, 3), dtype=np.float32)
    raw[:, 1] = rng.random(h * w, dtype=np.float32) * np.float32(3000.0)
    raw[:, 2] = rng.random(h * w, dtype=np.float32) * np.float32(4.1e6)
    return raw


def set_pattern(raw, pattern, rng):
    """writes channel 0 of the (npix, 3) frame body in place: valid pixels get a random positive easting, the others 0 or a
    negative one; with three survivors or more the first gets a NaN and the last a -inf in channel 2 and the middle one a NaN in channel 1 (what an
    earlier pattern planted there is made finite first)"""
    npix = len(raw)
    keep = validity(npix, pattern, rng)
    east = rng.random(npix, dtype=np.float32) * np.float32(7.4e5) + np.float32(0.25)
    raw[:, 0] = np.where(keep, east, np.where(np.arange(npix) % 3 == 0, np.float32(0.0), -east))
    if pattern == "specials":
        pos = special_positions(npix)
        raw[pos, 0] = SPECIALS[np.arange(len(pos)) % len(SPECIALS)]
    for c in (1, 2):
        raw[~np.isfinite(raw[:, c]), c] = np.float32(1234.5)
    alive = np.flatnonzero(raw[:, 0] > 0)
    if len(alive) >= 3:
        raw[alive[0], 2] = np.nan
        raw[alive[-1], 2] = -np.inf
        raw[alive[len(alive) // 2], 1] = np.nan
    return raw


def frame(h, w, pattern, seed=0):
    rng = np.random.default_rng([seed, h, w])
    return set_pattern(fill_channels(h, w, rng), pattern, rng).reshape(h, w, 3)
