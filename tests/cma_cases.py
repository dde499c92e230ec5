"""An independent restatement of the CMA-ES candidate draw (alproj_amd/csrc/alp_sampler.h) in numpy, shared by
tests/test_cma_sampler_reference.py and tests/test_gpu_cma_limits.py, and the grid rule of the population launch
(alproj_amd/csrc/host/alp_plan.h: pop_grid; tests/test_launch_plan.py holds the two to each other on the CPU).

The draw: philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011) with the counter
(j >> 1, try, candidate, generation as uint32) and the key (seed low, seed high); 53-bit uniforms and Box-Muller (z[j] from cos,
z[j + 1] from sin, 0 past D); x = mean + sigma * BD z; the first try inside the box, else try n_max clipped to it.  Everything
here is uint64 / float64 numpy with libm's log, sin and cos."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
TWO_PI = 6.283185307179586476925286766559
NEAR_FACE = 1e-12          # a coordinate this close to a box face at some try may be judged either way by the two libms


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """the 10-round Philox4x32 block of every (broadcast) counter under the key (k0, k1): four uint64 arrays of 32-bit words"""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3)]
    k0 = np.asarray(k0, dtype=np.uint64) & M32
    k1 = np.asarray(k1, dtype=np.uint64) & M32
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    for _ in range(10):
        p0 = PHILOX_M0 * c0                     # 32 x 32 -> 64 bits: exact in uint64
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def key_of(seed):
    s = int(seed) & (2 ** 64 - 1)
    return np.uint64(s & 0xFFFFFFFF), np.uint64(s >> 32)


def uniform53(hi, lo):
    """((hi << 21 | lo >> 11) + 0.5) / 2^53: never 0; the largest word pair rounds to exactly 1"""
    m = (hi << np.uint64(21)) | (lo >> np.uint64(11))
    return (m.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def normals(D, tries, cands, generation, seed):
    """(..., D) standard normal deviates of every (try, candidate) pair (broadcast shapes) of one generation and seed"""
    k0, k1 = key_of(seed)
    gen = np.uint64(int(generation) & 0xFFFFFFFF)          # the kernel's (unsigned) cast
    tries = np.asarray(tries, dtype=np.uint64)
    cands = np.asarray(cands, dtype=np.uint64)
    shape = np.broadcast_shapes(tries.shape, cands.shape)
    z = np.zeros(shape + (D,))
    for j in range(0, D, 2):
        w = philox4x32_10(np.uint64(j >> 1), tries, cands, gen, k0, k1)
        u1, u2 = uniform53(w[0], w[1]), uniform53(w[2], w[3])
        rad, ang = np.sqrt(-2.0 * np.log(u1)), TWO_PI * u2
        z[..., j] = rad * np.cos(ang)
        if j + 1 < D:
            z[..., j + 1] = rad * np.sin(ang)
    return z


def sample(mean, sigma, BD, bounds, P, n_max, seed, generation):
    """alp_cma_sample restated: (x (P, D), tries (P,), scale (P, D), near (P,)).  scale = |mean| + sigma |BD| |z| of the
    returned draw (what its rounding is relative to); near = some coordinate of a try that decided the candidate (every try
    up to the returned one) lies within NEAR_FACE of a box face"""
    mean = np.asarray(mean, dtype=np.float64)
    BD = np.asarray(BD, dtype=np.float64)
    D = len(mean)
    bounded = bounds is not None
    if bounded:
        b = np.asarray(bounds, dtype=np.float64)
        lo, hi = b[:, 0], b[:, 1]
    n_max = int(n_max) if bounded else 1
    x = np.empty((P, D))
    scale = np.empty((P, D))
    tries = np.full(P, -1, dtype=np.int64)
    near = np.zeros(P, dtype=bool)

    def draw(rows, ts):
        z = normals(D, ts[None, :], rows[:, None], generation, seed)          # (rows, T, D)
        return mean + sigma * (z @ BD.T), np.abs(mean) + sigma * (np.abs(z) @ np.abs(BD).T)

    def near_face(xs):
        return np.minimum(np.abs(xs - lo), np.abs(xs - hi)).min(axis=-1) < NEAR_FACE

    pending = np.arange(P)
    t0 = 0
    while t0 < n_max and len(pending):
        ts = np.arange(t0, min(t0 + (1 if t0 == 0 else 16), n_max))   # the first try alone: most candidates stop there
        xs, sc = draw(pending, ts)
        ok = np.all((xs >= lo) & (xs <= hi), axis=-1) if bounded else np.ones(xs.shape[:2], dtype=bool)
        hit = ok.any(axis=1)
        first = np.where(hit, ok.argmax(axis=1), len(ts) - 1)
        if bounded:                                       # the tries this chunk decided on: up to the first feasible one
            near[pending] |= (near_face(xs) & (np.arange(len(ts))[None, :] <= first[:, None])).any(axis=1)
        r = pending[hit]
        x[r] = xs[hit, first[hit]]
        scale[r] = sc[hit, first[hit]]
        tries[r] = t0 + first[hit]
        pending = pending[~hit]
        t0 = int(ts[-1]) + 1
    if len(pending):                                      # none feasible: try n_max, clipped
        xs, sc = draw(pending, np.array([n_max]))
        xs, sc = xs[:, 0], sc[:, 0]
        near[pending] |= near_face(xs)
        x[pending] = np.clip(xs, lo, hi)
        scale[pending] = sc
        tries[pending] = n_max
    return x, tries, scale, near


# ------------------------------------------------------------------ the grid of the batched population launch
POP_TC = 128
BATCHED_PARTIALS_BYTES = 128 << 20
# rows of one unmasked group by (precision, lens-free): PopCfg / PopCfgLF (tests/popeval_cases.py GROUP_ROWS)
GROUP_V = {("f32", False): 6, ("f32", True): 8, ("f64", False): 5, ("f64", True): 6}


def batched_grid(n, R, prec, lens_free, cu, batched=True):
    """(stripes, tile columns) that host::pop_grid picks for R candidates on n points with batched = true (no ALP_POP_GRID);
    batched=False: the grid of every other population launch (the rule without its last two steps)"""
    rows = -(-n // 256)
    V = GROUP_V[(prec, lens_free)]
    tiles = -(-R // POP_TC)
    ytiles = 1
    if prec == "f32":
        want = -(-rows // (4 * V))
        lo, hi = cu * 4, cu * 64
        rounded = -(-want // lo) * lo
        nblk = lo if want < lo else (hi if want > hi else (rounded if want < 4 * lo else want))
        if tiles >= 2:
            k = min(max(int(rows / (V * 2.12 * lo) + 0.5), 1), 16)
            stripes = -(-rows // (V * k))
            if stripes * tiles >= 4 * lo:
                nblk, ytiles = stripes, tiles
    else:
        nblk = cu * 24
        cap = (128 << 20) // (8 * R)
        if nblk > cap:
            nblk = max(cap, cu * 3)
    nblk = min(nblk, max(rows, 1))
    if not batched:
        return nblk, ytiles
    cap = BATCHED_PARTIALS_BYTES // (8 * R)
    if nblk > cap:
        nblk = max(cap, 1)
    fill = cu * 4
    if ytiles == 1 and tiles >= 2 and nblk < fill:
        ytiles = min(-(-fill // nblk), tiles)
    return nblk, ytiles
