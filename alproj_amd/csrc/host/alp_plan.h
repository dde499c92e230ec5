// Launch planning of the point-set kernels (alp_points.hip): the stripes x tile columns of a population evaluation, the points of
// one staged residual / Jacobian launch, the stripes of the normal-equations kernel, the grid of a streaming kernel, the
// magic-number division by a grid set's row length and the rows and columns of one vector of its points -- and of a render frame (alp_raster.hip): the grid of every kernel of the
// frame, the sizes of the once-per-mesh tile plan, the capacities of the device queues and which of them a finished frame's
// counters say must grow.
// Integer arithmetic on (n, P, precision, V, cu_count) resp. (mesh shape, frame size, tile size, cu_count, counters) alone; the
// caller allocates and launches.  Included by host/alp_host.h after host/alp_fold.h (ALP_HD); no HIP header.
// host/alp_host_selfcheck.cpp sweeps it (check_plan, check_frame_plan, check_row_div, check_row_walk) and prints it (--plan).
#pragma once

#include <cstdint>
#include <cstdlib>

namespace alp {

// Division by the row length W of a grid point set (alp_points.hip: points_grid_detect; K1's grid form: alp_point_kernels.h).
// q = (e * mul) >> shift equals e / W for every e < 2^31 when 1 <= W <= 2^16, with shift = 31 + ceil(log2 W) and
// mul = ceil(2^shift / W) < 2^32: mul exceeds 2^shift / W by less than 1, so e * mul / 2^shift exceeds e / W by less than
// e / 2^shift < 2^31 / 2^shift <= 1 / W, which never reaches the next integer (the fraction of e / W is at most (W - 1) / W).
struct RowDiv {
    uint32_t w = 0, shift = 0, mul = 0;          // w = 0: not a grid (K1 reads the x and y planes)
    ALP_HD uint32_t div(uint32_t e) const { return (uint32_t)(((uint64_t)e * mul) >> shift); }
};

// Row and column of the VEC consecutive points e0 .. e0 + VEC - 1 of a grid set, as K1's grid form reads them: point k has its x
// at index col(k) of the x plane (its column) and its y at index row0(k) of the y plane (the first point of its row).
// e0 <= last = n - 1; a point past `last` (padding of the final vector, which nothing reads) never leaves the planes.
// ONE division, for e0.  Then
//   one_row (c + VEC <= W: every vector when VEC divides W, all but about VEC in W of them otherwise): the points lie in e0's row
//     at the columns c, c + 1, ... < W -- K1 reads them as one vector at x + c and one y; padding follows in the same row;
//   else, W >= VEC: exactly one row end lies inside the vector -- an add and a compare per point; padding is clamped to `last`,
//     so a row that is not there is never addressed;
//   else (W < VEC: several row ends in one vector; such sets are tiny): a division per point, clamped to `last`.
template <int VEC>
struct RowWalk {
    RowDiv rd;
    uint32_t c, r0, room;          // e0's column, the first index of its row, last - e0
    bool one_row;
    ALP_HD RowWalk(const RowDiv &d, uint32_t e0, uint32_t last) : rd(d) {
        const uint32_t r = d.div(e0);
        r0 = r * d.w;
        c = e0 - r0;
        room = last - e0;
        one_row = d.w % VEC == 0 || c + VEC <= d.w;      // the first test is uniform and implies the second
    }
    ALP_HD void at(uint32_t k, uint32_t *col, uint32_t *row0) const {
        if (one_row) {
            *col = c + k;
            *row0 = r0;
        } else if (rd.w >= VEC) {
            const uint32_t ck = c + (k < room ? k : room);
            const bool next = ck >= rd.w;
            *col = next ? ck - rd.w : ck;
            *row0 = next ? r0 + rd.w : r0;
        } else {
            const uint32_t e = r0 + c + (k < room ? k : room), r = rd.div(e);
            *col = e - r * rd.w;
            *row0 = r * rd.w;
        }
    }
};

namespace host {

inline RowDiv row_div(uint32_t w) {
    RowDiv rd;
    uint32_t l = 0;
    while ((1u << l) < w) ++l;                    // ceil(log2 w)
    rd.w = w;
    rd.shift = 31 + l;
    rd.mul = (uint32_t)((((uint64_t)1 << rd.shift) + w - 1) / w);
    return rd;
}

// memory-bound streaming kernels: enough workgroups of 256 lanes to fill 256 CUs x 8, grid-stride beyond
inline int stream_grid(int64_t items, int cu_count) {
    const int64_t want = (items + 255) / 256;
    const int64_t cap = (int64_t)cu_count * 8;
    return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}

// device staging of the residual and Jacobian entry points: at most RES_CHUNK_BYTES of output per launch
constexpr int64_t RES_CHUNK_BYTES = (int64_t)256 << 20;
// points per launch when a point stages `pairs_per_point` double2 values (alp_residuals_batch: the B poses; alp_jacobian: the D
// targets): whole multiples of 1024 points, at least 1024, at most n
inline int64_t stage_chunk_points(int64_t n, int64_t pairs_per_point) {
    int64_t chunk = RES_CHUNK_BYTES / (pairs_per_point * 16) / 1024 * 1024;
    if (chunk < 1024) chunk = 1024;
    return chunk > n ? n : chunk;
}

// stripes of the float64 confirmation pass over a float32 set (alp_points.hip: confirm_losses): one tile column
inline int confirm_grid(int64_t n, int cu_count) {
    const int64_t rows = (n + 255) / 256, want = (int64_t)cu_count * 4;
    return (int)(rows < want ? (rows > 0 ? rows : 1) : want);
}

// the multi-start launch of the device loop (`batched`) keeps its partial sums (stripes x P doubles) within this
constexpr int64_t POP_BATCHED_PARTIALS_BYTES = (int64_t)128 << 20;

// The grid of popeval_kernel: `stripes` workgroups along x, each over a run of whole rows of 256 points, times `tile_cols`
// columns of TC candidates each along y (1: a workgroup walks every tile of its stripe).
struct PopGrid { int stripes, tile_cols; };

// n points x P candidates; V = rows of a full group of the kernel variant (PopCfg<T>::V or PopCfgLF<T>::V), TC = candidates
// per tile; (ov_stripes, ov_tile_cols) = the parsed ALP_POP_GRID pair, 0 when absent
inline PopGrid pop_grid(int64_t n, int64_t P, bool is_f64, int V, int TC, int cu_count, bool batched, int ov_stripes = 0,
                        int ov_tile_cols = 0) {
    // one workgroup per stripe of ~24 rows of 256 points (four groups of V = 6), between 4 and 64
    // workgroups per CU: a stripe is re-read once per tile of 128 candidates and a short one stays
    // in cache between those passes.  Measured, 100 M x 2048 float32: 4 workgroups per CU 244 ms,
    // 8: 229, 16: 224, 32: 221, 64: 219, 128: 219; 10 M x 256: 8 per CU (stripes of 19 rows) 3.31
    // ms, 16: 3.46, 32: 3.73.  float64 (three workgroups resident per CU): 24 per CU (round 5: 527 ms against 541 with 4).
    int nblk = cu_count * (is_f64 ? 24 : 4), ytiles = 1;
    const int64_t rows = (n + 255) / 256, tiles = (P + TC - 1) / TC;
    if (!is_f64) {
        const int64_t want = (rows + 4 * V - 1) / (4 * V);            // ~four full groups per stripe
        const int64_t lo = (int64_t)cu_count * 4, hi = (int64_t)cu_count * 64;
        // whole rounds of the 4 workgroups a CU holds at once while the grid is only a few rounds deep
        const int64_t rounded = (want + lo - 1) / lo * lo;
        nblk = (int)(want < lo ? lo : (want > hi ? hi : (want < 4 * lo ? rounded : want)));
        // Two candidate tiles or more: the grid is stripes x tiles -- a workgroup runs ONE tile of 128 candidates over a stripe of
        // whole groups of V rows.  Round 3 introduced it for populations of a few tiles whose one-column grid was only a few
        // rounds deep (10 M x 256: 1954 stripes of 20 rows = 1.9 rounds of the 1024 resident workgroups, 2 rows of every 20 in
        // the narrow groups; tools/sweep_popeval_grid.py, ms for P = 256 / 384 / 512 at 10 M points: one column of 2048 stripes
        // 3.15 / 4.64 / 6.14; stripes of 18 rows x tiles 2.90 / 4.33 / 5.61).  Round 6 measured it at every other shape as well
        // (profiles/r06_popeval_grid_sweep.txt, one column -> stripes x tiles, general | lens-free variant): 10 M x 1024 12.2 ->
        // 11.0 | 5.81 -> 4.91 ms; 10 M x 2048 24.6 -> 21.7 | 11.5 -> 9.64; 30 M x 1024 34.9 -> 32.5 | 15.8 -> 14.4; 100 M x 2048
        // 219.5 -> 215.2 | 95.7 -> 93.4 -- never slower, so it is the rule.  Stripes of k groups, k grown with the point count
        // (about two stripes per resident slot and tile column for small sets, up to 16 groups = ~25 000 points for large ones:
        // the timings are flat from 4 to 16 groups and the partial-sum buffer shrinks with the stripe count).
        // The sums depend on the shape in the last bits only (up to ~3e-8 relative between shapes: other group boundaries).
        if (tiles >= 2) {
            int64_t k = (int64_t)((double)rows / ((double)V * 2.12 * (double)lo) + 0.5);      // groups of V rows per stripe
            k = k < 1 ? 1 : (k > 16 ? 16 : k);
            const int64_t stripes = (rows + V * k - 1) / (V * k);
            if (stripes * tiles >= 4 * lo) { nblk = (int)stripes; ytiles = (int)tiles; }
        }
    } else {
        // the per-stripe partial sums (nblk x P doubles, read once per generation by reduce_partials_kernel) stay below 128 MB:
        // 24 stripes per CU at P = 2048 are 100 MB (kept: 527 ms against 533 with 8 per CU); a population of 8192 gets 2048 stripes
        const int64_t cap = ((int64_t)128 << 20) / (8 * P);
        const int64_t lo = (int64_t)cu_count * 3;                  // one round of the three resident workgroups per CU
        if (nblk > cap) nblk = (int)(cap > lo ? cap : lo);
    }
    // tuning hook ALP_POP_GRID="stripes,ytiles".  The stripe count moves the last bits of the losses in either precision: it decides which
    // rows go through the V-wide, the 2-wide and the masked single-row groups (float32: other group sums, up to ~3e-8 relative) and sets the
    // ORDER of the float64 additions.  Same grid, same bits (tests/test_gpu_popeval_grid.py) -- a development switch, not a setting
    if (ov_stripes >= 1 && ov_tile_cols >= 1 && ov_tile_cols <= tiles) { nblk = ov_stripes; ytiles = ov_tile_cols; }
    if (rows < nblk) nblk = (int)(rows > 0 ? rows : 1);
    if (batched) {
        const int64_t cap = POP_BATCHED_PARTIALS_BYTES / (8 * P);
        if (nblk > cap) nblk = (int)(cap > 1 ? cap : 1);
        const int64_t fill = (int64_t)cu_count * 4;
        if (ytiles == 1 && tiles >= 2 && nblk < fill) {
            const int64_t cols = (fill + nblk - 1) / nblk;
            ytiles = (int)(cols < tiles ? cols : tiles);
        }
    }
    return {nblk, ytiles};
}

// The grid of the mend pass over a float32 set (alp_points_set_mend; alp_points.hip: mend_launch): popeval_counted_kernel,
// float64 arithmetic with V = PopCfg<double>::V rows per group.  The number of candidates it evaluates is known on the device
// only, so the grid is planned for the worst case, all P of them: one column per tile of TC candidates (tile_cols x TC >= P; a
// workgroup whose tile lies beyond the count returns at once, so the columns in use are ceil(count / TC)) times `stripes`
// stripes of whole rows.  The stripes follow the float64 rule of pop_grid -- at least one round of the three resident
// workgroups per CU, at most 24 per CU, never more than rows, partial sums (stripes x P doubles) within 128 MB -- and between
// those bounds aim at four groups of V rows each: a column's workgroup stages its 128 records (32 KB) once per stripe, and a
// stripe of one or two groups would read about as many bytes of records as of points.
inline PopGrid mend_grid(int64_t n, int64_t P, int V, int TC, int cu_count) {
    const int64_t rows = (n + 255) / 256, tiles = (P + TC - 1) / TC;
    const int64_t lo = (int64_t)cu_count * 3, hi = (int64_t)cu_count * 24;
    int64_t nblk = (rows + 4 * V - 1) / (4 * V);
    nblk = nblk < lo ? lo : (nblk > hi ? hi : nblk);
    const int64_t cap = POP_BATCHED_PARTIALS_BYTES / (8 * (P > 0 ? P : 1));
    if (nblk > cap) nblk = cap;
    if (nblk > rows) nblk = rows;
    if (nblk < 1) nblk = 1;
    return {(int)nblk, (int)(tiles > 0 ? tiles : 1)};
}

// The grid of normal_poses_kernel (alp_normal_equations -- B = 1 --, alp_normal_equations_batch, its _rows form and the rounds
// of alp_lm.hip): B poses over the same points, one workgroup per (stripe, pose) pair, `blocks` stripes per pose -- blocks x B
// workgroups.  A stripe is `groups_per` whole groups of 256 points (a pose's last stripe may be shorter and its last group
// ragged); every workgroup writes ONE row of partial sums.
// Workgroups aimed at: NORMAL_WG_PER_CU per CU -- two rounds of the three a CU holds at once (50 KB of LDS each) -- and never
// more than NORMAL_MAX_BLOCKS, which keeps the partial rows (at most 300 doubles each) of one pose below 5 MB whatever the
// device.  They are shared out among the poses: a pose gets ceil(want / B) stripes, at least one, at most one per group; the
// stripes are then made as long as they must be and those that would be left without a group are not launched.
// blocks x B < want + B, so the partial rows stay below 7.4 MB up to NORMAL_BATCH_MAX poses.  n = 0 or B < 1: no launch.
constexpr int NORMAL_WG_PER_CU = 6;
constexpr int NORMAL_MAX_BLOCKS = 2048;
struct NormalGrid { int blocks; int64_t groups_per; };
constexpr int NORMAL_BATCH_MAX = 1024;

inline NormalGrid normal_batch_grid(int64_t n, int64_t B, int cu_count) {
    const int64_t groups = (n + 255) / 256;
    if (groups <= 0 || B < 1) return {0, 0};
    int64_t want = (int64_t)cu_count * NORMAL_WG_PER_CU;
    if (want > NORMAL_MAX_BLOCKS) want = NORMAL_MAX_BLOCKS;
    int64_t stripes = (want + B - 1) / B;
    if (stripes < 1) stripes = 1;
    if (stripes > groups) stripes = groups;
    const int64_t per = (groups + stripes - 1) / stripes;
    return {(int)((groups + per - 1) / per), per};
}

// ------------------------------------------------------------------ the render frame (alp_raster.hip)
// The launch shapes of one frame.  (tile_w, tile_h) = the cells of a raster_grid_kernel tile (GT_W x GT_H); the two
// blocks-per-CU figures are the tunables next to raster_kernel and resolve_kernel.
struct FramePlan {
    // regular-grid meshes
    int tiles_x = 0;
    int64_t tiles = 0;                          // tiles_x x tile rows: one raster_grid_kernel workgroup each
    unsigned plan_grid = 0;                     // tile_plan_kernel, tile_occlusion_kernel: one thread per tile
    unsigned grid_wgs = 0;                      // raster_grid_kernel: whole turns of the 8 XCDs (see the kernel's phase 0)
    int parked_wgs[2] = {0, 0};                 // raster_parked_kernel, first / second round
    int64_t tile_bounds_bytes = 0;              // once per mesh: six floats per tile ...
    int64_t tile_lists_bytes = 0;               // ... and three tile lists (near, far, far survivors)
    // index arrays
    int index_grid = 0;                         // raster_kernel (0 for a mesh without triangles: not launched)
    // both
    int general_wgs = 0, large_wgs = 0;         // raster_general_kernel, raster_large_kernel
    int resolve_grid = 0;                       // resolve_kernel
};

// min(ceil(items / 256), cu_count * blocks_per_cu): grid-stride kernels with one thread per item
inline int capped_grid(int64_t items, int cu_count, int blocks_per_cu) {
    const int64_t want = (items + 255) / 256, cap = (int64_t)cu_count * blocks_per_cu;
    return (int)(want < cap ? want : cap);
}

inline FramePlan frame_plan(bool implicit, int64_t grid_h, int64_t grid_w, int64_t n_tri, int w, int h, int cu_count, int tile_w,
                            int tile_h, int raster_blocks_per_cu = 64, int resolve_blocks_per_cu = 64) {
    FramePlan p;
    if (implicit) {
        p.tiles_x = (int)((grid_w - 1 + tile_w - 1) / tile_w);
        p.tiles = (int64_t)p.tiles_x * ((grid_h - 1 + tile_h - 1) / tile_h);
        p.plan_grid = (unsigned)((p.tiles + 255) / 256);
        p.grid_wgs = (unsigned)((p.tiles + 7) / 8 * 8);
        p.parked_wgs[0] = cu_count * 8;
        p.parked_wgs[1] = cu_count * 2;
        p.tile_bounds_bytes = p.tiles * 6 * (int64_t)sizeof(float);
        p.tile_lists_bytes = 3 * p.tiles * (int64_t)sizeof(unsigned);
    } else {
        p.index_grid = capped_grid(n_tri, cu_count, raster_blocks_per_cu);
    }
    p.general_wgs = cu_count * 2;
    p.large_wgs = cu_count * 8;
    p.resolve_grid = capped_grid((int64_t)w * h, cu_count, resolve_blocks_per_cu);
    return p;
}

// The device queues of a mesh, in entries: work items (raster_large_kernel), general entries (raster_general_kernel) and the
// parked work of the grid kernel -- small triangles, large triangles, cells -- of the first and of the second round.
struct FrameQueues {
    unsigned items = 0, general = 0;
    unsigned park[3] = {0, 0, 0}, park_b[3] = {0, 0, 0};
};

// The queues start at 2^20 entries and grow on demand; ALP_QUEUE_CAP (`env`: its text, or NULL) lowers the start so that tests
// can exercise the growth.
constexpr unsigned QUEUE_CAP_DEFAULT = 1u << 20;
inline unsigned initial_queue_cap(const char *env) {
    if (env) {
        const long v = atol(env);
        if (v >= 1 && v < (1l << 30)) return (unsigned)v;
    }
    return QUEUE_CAP_DEFAULT;
}
// a queue that held `n` entries too few is grown to a quarter more than was asked for
inline unsigned grown_cap(unsigned n) { return n + n / 4 + 1024; }
// The second round (far tiles: hardly anything to park) gets an eighth of the first round's capacity, and never less than it had.
inline unsigned second_round_cap(unsigned previous, unsigned first_round) {
    const unsigned c = first_round / 8 + 64;
    return previous > c ? previous : c;
}
// the parked queues of the first grid frame: ~0.7 M parked cells and a few 100 k parked triangles per 5616 x 3744 frame of the
// 100 M-vertex DSM, so the cells start at twice the default; an overridden start is taken for all three
inline void initial_park_caps(unsigned cap, FrameQueues *q) {
    q->park[0] = q->park[1] = cap;
    q->park[2] = cap == QUEUE_CAP_DEFAULT ? 2u << 20 : cap;
    for (int k = 0; k < 3; ++k) q->park_b[k] = second_round_cap(q->park_b[k], q->park[k]);
}

// What a finished frame says about its queues.  `counters`: the frame's pinned counters, per round (stride `stride`) [0] work
// items, [1] general entries, [2] small parked, [3] large parked, [4] parked cells -- what the kernels ASKED for, whether it
// fitted or not.  `have`: the capacities the frame ran with; `has_park`: the parked queues exist (a grid mesh that has drawn).
// Work items and general entries of both rounds share one queue each and the second round's counters continue the first's, so
// the larger one decides.  caps = `have` with every overflowed queue grown; a grown first-round parked queue takes its second
// round along (second_round_cap).  Asked again with the same counters and `caps`, the answer is none(): the frame is redone
// once per overflow, not for ever.
struct QueueVerdict {
    bool items = false, general = false, park = false;      // which allocations must be made anew
    FrameQueues caps;
    bool none() const { return !items && !general && !park; }
};

inline QueueVerdict frame_verdict(const unsigned *counters, int stride, bool has_park, const FrameQueues &have) {
    QueueVerdict v;
    v.caps = have;
    const unsigned *a = counters, *b = counters + stride;
    const unsigned items = a[0] > b[0] ? a[0] : b[0], general = a[1] > b[1] ? a[1] : b[1];
    if (items > have.items) { v.items = true; v.caps.items = grown_cap(items); }
    if (general > have.general) { v.general = true; v.caps.general = grown_cap(general); }
    if (!has_park) return v;
    for (int k = 0; k < 3; ++k) {
        if (a[2 + k] > have.park[k]) { v.park = true; v.caps.park[k] = grown_cap(a[2 + k]); }
        if (b[2 + k] > have.park_b[k]) { v.park = true; v.caps.park_b[k] = grown_cap(b[2 + k]); }
    }
    if (v.park)
        for (int k = 0; k < 3; ++k) v.caps.park_b[k] = second_round_cap(v.caps.park_b[k], v.caps.park[k]);
    return v;
}

}  // namespace host
}  // namespace alp
