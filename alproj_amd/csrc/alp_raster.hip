// libalproj_hip.so -- depth-buffered mesh render + lens-distortion remap: the OpenGL
// replacement for persp_proj(), src/alproj/project.py:145-294 (call stack in SURVEY.md 3.2).
//
// What the reference makes OpenGL do, and where it is restated here:
//   project.py:203-207  camera position minus offsets (X,Z,Y order)        -> make_view()
//   project.py:13-54    projection_mat, used WITHOUT cx,cy (:257) and untransposed (:262):
//                       clip = (fx vx, fy vy, -1, vz) => near plane at view depth 1, no far
//                       plane, principal point ignored (quirks Q10, Q11)      -> to_window()
//   project.py:56-109   modelview_mat R = Rz(roll) Rx(tilt) Ry(360-pan)      -> make_view()
//   project.py:211-212  depth test GL_LESS + back-face culling (CCW front)   -> raster_tri()
//   project.py:217-253  varyings value, |view_pos|; min_dist mask            -> shade()
//   project.py:269-281  clear to 0, one indexed TRIANGLES draw, readback, flipud
//   project.py:111-143  distort(): inverted-coefficient source map, nearest gather, 0 border
//                                                                         -> remap_source()
//
// Pipeline (all on the library stream, no host round trip; DESIGN.md section 5 has the launch table):
//   1. clear the 64-bit visibility buffer (one word per pixel: float32 1/vz << 32 | ~triangle id) and the
//      frame's queue / list counters behind it
//   2. coverage, one of
//      regular-grid meshes (no index array, or an index array recognised at mesh creation as the grid or
//      as the grid minus the triangles of masked vertices):
//        tile_plan_kernel        tiles of 64x16 cells: frustum culling, NEAR / FAR lists
//        raster_grid_kernel      first round, NEAR tiles: one workgroup per tile, vertices transformed /
//                                projected / snapped once into LDS, one lane per cell = two triangles;
//                                fragments of small cells through an LDS depth patch where the tile's
//                                footprint fits one, larger cells and triangles parked in device queues
//        raster_parked_kernel    the parked cells (a wave per cell) and triangles (a wave per triangle)
//        hiz_build / hiz_top / tile_occlusion_kernel   depth pyramid, occlusion test of the FAR tiles
//        raster_grid_kernel, raster_parked_kernel      second round: the surviving FAR tiles
//      any other index array:
//        raster_kernel           one thread per triangle, three gathered vertices
//      all of them use emit_small(): 32-bit bounding-box rejection and back-face test, then an inline walk of
//      the bounding box with exact integer edge functions (64-bit atomicMax per covered pixel centre) for
//      triangles under 64 px; near-plane crossings and larger triangles go to raster_general_kernel, which
//      splits them into 64x64-pixel work items
//   3. raster_large_kernel: one wave per work item, one lane per pixel column
//   4. resolve_kernel: one thread per OUTPUT pixel: distortion source map (float64), fetch the
//      winning triangle, perspective-correct interpolation by ray/triangle intersection in view
//      space, min_distance mask, write h x w x 3 float32 (row 0 = top)
// On the host a frame is render_impl: clear, ensure_grid_plan (once per grid mesh: parked queues, tile boxes), draw_grid_mesh
// or draw_indexed_mesh (step 2 and 3), resolve_frame.  Every grid size and queue capacity, and the verdict of finish_frame on
// a finished frame's queue counters, is integer arithmetic in host/alp_plan.h (frame_plan, initial_park_caps, frame_verdict),
// HIP-free and swept on the CPU; this file allocates and launches.  The development builds' reports hang on three hooks
// (raster_dev.h), empty in a release build.
//
// Preprocessor switches of this translation unit; a build with any of them set needs -DALP_DEV (the guards at the head of
// raster_dev.h stop it otherwise) and says so through alp_build_flags().  tests/test_abi_symbols.py holds this list and the
// guards to every #if of the unit.
//   development switches: ALP_WG_TIMING ALP_RASTER_STATS VIS_PLAIN_STORE VIS_NEVER PARK_NOATOMIC PARKED_SKIP_CELLS
//                         PARKED_SKIP_COOP PARKED_SKIP_COOP4 GRID_STOP_AFTER GRID_NO_XCD_SWIZZLE
//   tunables:             INLINE_LOG2 FAST_MAX COOP_MIN_W COOP_MIN_PIX GT_W_LOG2 GT_H_LOG2 HIZ_SPAN GRID_WAVES_PER_EU
//                         PATCH_MIN_FAST PATCH_WORDS_NEAR PATCH_WORDS_FAR RASTER_BLOCKS_PER_CU RESOLVE_BLOCKS_PER_CU
// The arithmetic that decides coverage and visibility is specified step by step in DESIGN.md
// section 5 and compiled with -ffp-contract=off so that it is reproducible bit for bit.
//
// Pinned by a real OpenGL: the reference's own persp_proj, run unmodified on Mesa llvmpipe in the
// build container, shows the same triangle and value on every pixel where a conformant GL has no freedom
// (tests/golden/g15_gl_render.npz, tests/test_gpu_gl.py).  The rules OpenGL leaves to the implementation
// (sub-pixel snapping, tie-break on shared edges, depth-buffer precision) are fixed here watertight and
// deterministic; how often they make a pixel differ from llvmpipe's is measured there too (0-2 pixels per frame).
#include "alp_raster_internal.h"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <thread>
#include <type_traits>
#include <vector>

namespace alp {

// the development switches' guards, alp_build_flags() and report hooks (before the kernels: the guards must see which
// tunables the command line set)
#include "raster_dev.h"
// The stages, in dependency order (one translation unit: the kernels inline each other's device functions):
#include "raster_common.h"
#include "raster_parked.h"
#include "raster_index.h"
#include "raster_plan.h"
#include "raster_grid.h"
#include "raster_large.h"
#include "raster_resolve.h"
#include "raster_post.h"

}  // namespace alp

using namespace alp;

namespace alp {

int upload_chunked(void *dst, const void *src, size_t bytes) {
    const size_t CH = (size_t)256 << 20;
    for (size_t off = 0; off < bytes; off += CH) {
        const size_t n = bytes - off < CH ? bytes - off : CH;
        ALP_HIP(hipMemcpyAsync((char *)dst + off, (const char *)src + off, n, hipMemcpyHostToDevice, ctx().stream));
    }
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    return ALP_OK;
}

// A host array of `total` elements of `esize` bytes through the staging buffer `stage` in chunks of `chunk` elements, one
// kernel per chunk: launch(off, cnt).  Nothing waits in between (tools/h2d_rate.hip: large chunks, no sync) -- the stream
// orders a chunk's kernel before the next chunk's copy.  Ends at the first HIP error; the caller synchronises.
template <typename Launch>
static hipError_t staged_upload(const void *src, size_t esize, int64_t total, int64_t chunk, void *stage, Launch launch) {
    for (int64_t off = 0; off < total; off += chunk) {
        const int64_t cnt = total - off < chunk ? total - off : chunk;
        hipError_t e = hipMemcpyAsync(stage, (const char *)src + (size_t)off * esize, (size_t)cnt * esize, hipMemcpyHostToDevice, ctx().stream);
        if (e != hipSuccess) return e;
        launch(off, cnt);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

int ensure_queue(alp_mesh *m, unsigned cap) {
    if (m->queue && m->qcap >= cap) return ALP_OK;
    m->qcap = 0;
    if (int rc = m->queue.reserve((size_t)cap * sizeof(WorkItem))) return rc;
    m->qcap = cap;
    return ALP_OK;
}

// both device queues start at 2^20 entries and grow on demand (finish_frame); ALP_QUEUE_CAP
// lowers the start so that tests can exercise the growth path
unsigned initial_queue_cap() { return host::initial_queue_cap(getenv("ALP_QUEUE_CAP")); }

// Queues of parked work: [first round | second round] per kind (small triangles, large triangles, cells), `cap` and `cap_b`
// entries; the capacities are host::initial_park_caps' at the first grid frame and host::frame_verdict's after an overflow.
static int alloc_park(alp_mesh *m, const unsigned cap[3], const unsigned cap_b[3]) {
    for (int k = 0; k < 3; ++k) m->park_cap[k] = m->park_cap_b[k] = 0;
    m->park_large = nullptr;
    reset_all(m->park_small, m->park_cell);
    const size_t triangles = ((size_t)cap[0] + cap_b[0] + cap[1] + cap_b[1]) * sizeof(Deferred);
    const size_t cells = ((size_t)cap[2] + cap_b[2]) * sizeof(ParkedCell);
    if (int rc = reserve_all({triangles, cells}, m->park_small, m->park_cell)) return rc;
    m->park_large = m->park_small + cap[0] + cap_b[0];
    for (int k = 0; k < 3; ++k) {
        m->park_cap[k] = cap[k];
        m->park_cap_b[k] = cap_b[k];
    }
    return ALP_OK;
}

int apply_derived_mask(alp_mesh *m, const unsigned char *user) {
    hipStream_t st = ctx().stream;
    unsigned char *user_dev = nullptr;
    if (user) {
        if (int rc = scratch_reserve((size_t)m->n_vert, (void **)&user_dev)) return rc;
        if (int rc = upload_chunked(user_dev, user, (size_t)m->n_vert)) return rc;
    }
    if (int rc = m->valid.reserve((size_t)m->n_vert)) return rc;
    hipLaunchKernelGGL(mask_and_kernel, dim3((unsigned)((m->n_vert + 255) / 256)), dim3(256), 0, st, m->valid_derived, user_dev,
                       (long long)m->n_vert, m->valid);
    ALP_HIP(hipGetLastError());
    ALP_HIP(hipStreamSynchronize(st));
    return ALP_OK;
}

// alp_mesh_create, explicit index array that is not the full grid: is it the grid with triangles removed
// such that a vertex mask says which (see subgrid_mark_kernel)?  On success the mesh becomes an implicit
// grid with that mask; on any mismatch it stays what it was.  `first` = the array's first triangle.
int try_subgrid(alp_mesh *m, const long long first[3]) {
    const long long a = first[0], b = first[1], c = first[2];
    const long long gw = c == a + 1 ? b - a - 1 : b - a;
    if (a < 0 || gw < 2 || m->n_vert % gw) return ALP_OK;
    const long long gh = m->n_vert / gw;
    if (gh < 2) return ALP_OK;
    const long long full = 2 * (gh - 1) * (gw - 1);
    // a small part of a large grid is cheaper as the index array it is
    if (m->n_tri >= full || m->n_tri * 4 < full) return ALP_OK;
    hipStream_t st = ctx().stream;
    const long long words = (full + 31) / 32, blocks = (words + 255) / 256;
    // the mask, the triangle bits and their ranks stay this function's own until every check has passed
    DeviceBuffer<unsigned char> derived;
    DeviceBuffer<unsigned> present, rank, block_dev;
    if (int rc = reserve_all({(size_t)m->n_vert, (size_t)words * 4, (size_t)words * 4, (size_t)blocks * 4},
                             derived, present, rank, block_dev))
        return rc;
    hipError_t e = hipMemsetAsync(derived, 0, (size_t)m->n_vert, st);
    if (e == hipSuccess) e = hipMemsetAsync(present, 0, (size_t)words * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(m->qcount_dev, 0, sizeof(unsigned), st);
    if (e != hipSuccess) return fail(ALP_EHIP, "sub-grid check: memset");
    hipLaunchKernelGGL(subgrid_mark_kernel, dim3(ctx().cu_count * 8), dim3(256), 0, st, m->ind, (long long)m->n_tri, gw, gh,
                       present, derived, m->qcount_dev);
    hipLaunchKernelGGL(subgrid_absent_kernel, dim3(ctx().cu_count * 8), dim3(256), 0, st, full, gw, present,
                       derived, m->qcount_dev);
    hipLaunchKernelGGL(subgrid_blocksum_kernel, dim3((unsigned)blocks), dim3(256), 0, st, present, words, block_dev);
    std::vector<unsigned> sums((size_t)blocks);
    e = hipMemcpyAsync(m->qcount_host, m->qcount_dev, sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(sums.data(), block_dev, (size_t)blocks * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ALP_EHIP, "sub-grid check: %s", hipGetErrorString(e));
    if (*m->qcount_host != 0) return ALP_OK;                               // not a filtered grid: keep the index array
    unsigned long long run = 0;
    for (auto &s : sums) {
        const unsigned here = s;
        s = (unsigned)run;
        run += here;
    }
    if ((long long)run != m->n_tri) return ALP_OK;                          // cannot happen after the order check; be safe
    e = hipMemcpyAsync(block_dev, sums.data(), (size_t)blocks * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(subgrid_rank_kernel, dim3((unsigned)blocks), dim3(256), 0, st, present, words, block_dev, rank);
        e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) return fail(ALP_EHIP, "sub-grid ranks: %s", hipGetErrorString(e));
    block_dev.reset();
    m->valid_derived = std::move(derived);
    if (int rc = apply_derived_mask(m, nullptr)) {
        // (m->valid: the mesh is being created, a mask can only be this function's own, half-made one)
        reset_all(m->valid_derived, m->valid);
        return rc;
    }
    m->tri_present = std::move(present);
    m->tri_rank = std::move(rank);
    m->ind.reset();
    m->implicit = true;
    m->grid_h = gh;
    m->grid_w = gw;
    m->n_tri = full;
    return ALP_OK;
}

int ensure_gqueue(alp_mesh *m, unsigned cap) {
    if (m->gqueue && m->gcap >= cap) return ALP_OK;
    m->gcap = 0;
    if (int rc = m->gqueue.reserve((size_t)cap * sizeof(unsigned))) return rc;
    m->gcap = cap;
    return ALP_OK;
}

int finish_frame_of(alp_mesh *m);      // = finish_frame below (anonymous namespace)

// The x > 0 selection of reverse_proj (project.py:369) on the resident frame, in two steps: count + exclusive scan
// per chunk of the image (frame_valid_count, also waits for the frame and checks its queues), then the order-
// preserving write of the survivors' pixel index and (x, y, z) = channels (0, 2, 1) + offsets as float64
// (frame_valid_write; device pointers).  Shared by alp_render_fetch_valid and alp_render_rasterize_*.
int frame_valid_count(alp_mesh *m, int64_t *count) {
    if (int e = finish_frame_of(m)) return e;
    const long long npix = (long long)m->w * m->h;
    const int chunks = (int)((npix + COMPACT_CHUNK - 1) / COMPACT_CHUNK);
    if (chunks > m->compact_cap) {
        m->compact_cap = 0;
        reset_all(m->compact_counts, m->compact_offsets);
        // counts | the chunks' extents (four floats each);  offsets | the total | the frame's extent (four floats)
        const size_t counts = (size_t)chunks * (sizeof(unsigned) + 4 * sizeof(float)) + 16;
        const size_t offsets = (size_t)(chunks + 3) * sizeof(unsigned long long);
        if (int rc = reserve_all({counts, offsets}, m->compact_counts, m->compact_offsets)) return rc;
        m->compact_cap = chunks;
    }
    hipStream_t st = ctx().stream;
    ktime_begin();
    float *span = (float *)(((uintptr_t)(m->compact_counts + chunks) + 15) & ~(uintptr_t)15);
    hipLaunchKernelGGL(valid_count_kernel, dim3(chunks), dim3(256), 0, st, m->image, npix, m->compact_counts, span);
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(1024), 0, st, m->compact_counts, chunks, m->compact_offsets, span);
    ktime_end();
    ALP_HIP(hipGetLastError());
    unsigned long long tail[3] = {0, 0, 0};      // the total, then the extent of channels 0 and 2 over the survivors
    ALP_HIP(hipMemcpyAsync(tail, m->compact_offsets + chunks, sizeof(tail), hipMemcpyDeviceToHost, st));
    ALP_HIP(hipStreamSynchronize(st));
    const unsigned long long total = tail[0];
    memcpy(m->valid_span, tail + 1, sizeof(m->valid_span));
    m->valid_total = (int64_t)total;
    *count = m->valid_total;
    return ALP_OK;
}

int frame_valid_write(alp_mesh *m, const double *offsets, unsigned *idx_dev, double *xyz_dev, bool planar) {
    const long long npix = (long long)m->w * m->h;
    const int chunks = (int)((npix + COMPACT_CHUNK - 1) / COMPACT_CHUNK);
    const double o0 = offsets ? offsets[0] : 0.0, o1 = offsets ? offsets[1] : 0.0, o2 = offsets ? offsets[2] : 0.0;
    ktime_begin();
    hipLaunchKernelGGL(valid_write_kernel, dim3(chunks), dim3(256), 0, ctx().stream, m->image, npix, m->compact_offsets, o0, o1,
                       o2, idx_dev, xyz_dev, planar ? 1ll : 3ll, planar ? (long long)m->valid_total_planes : 1ll);
    ktime_end();
    ALP_HIP(hipGetLastError());
    return ALP_OK;
}

}  // namespace alp

namespace {

int ensure_frame(alp_mesh *m, int w, int h) {
    if (m->w == w && m->h == h && m->vis) return ALP_OK;
    m->w = m->h = 0;             // the new size is published last: a frame whose buffers are not all there has no pixels
    m->vis_current = false;
    reset_all(m->vis, m->image);
    if (int rc = reserve_all({(size_t)w * h * sizeof(unsigned long long) + QC_TOTAL * sizeof(unsigned),      // + the frame's counters
                              (size_t)w * h * 3 * sizeof(float)}, m->vis, m->image))
        return rc;
    m->hiz.reset();
    if (int rc = m->hiz.reserve((size_t)hiz_total(w, h) * sizeof(unsigned))) return rc;
    m->w = w;
    m->h = h;
    return ALP_OK;
}

// ---- one frame, step by step.  Every grid size comes from host::frame_plan (host/alp_plan.h); the steps allocate and launch.
// The frame's counters live right behind the visibility buffer (one fill clears both).  Queue counters, QC_STRIDE per round:
// [0] work items, [1] general entries, [2] small parked, [3] large parked, [4] parked cells; then (+ 2 * QC_STRIDE) the
// lengths of the three tile lists and the FAR tiles' screen region.
unsigned *frame_counters(const alp_mesh *m, const View &v) { return (unsigned *)(m->vis + (size_t)v.w * v.h); }

host::FramePlan frame_plan_of(const alp_mesh *m, const View &v) {
    return host::frame_plan(m->implicit, m->grid_h, m->grid_w, m->n_tri, v.w, v.h, ctx().cu_count, GT_W, GT_H, RASTER_BLOCKS_PER_CU,
                            RESOLVE_BLOCKS_PER_CU);
}

// the rare cases of one round (near-plane crossings, 64 px and more): general entries into work items, then the work items
template <bool IMPLICIT>
int drain_rare(alp_mesh *m, const View &v, const host::FramePlan &p, int round) {
    hipStream_t st = ctx().stream;
    unsigned *items = frame_counters(m, v) + QC_STRIDE * round, *general = items + 1;
    hipLaunchKernelGGL((raster_general_kernel<IMPLICIT>), dim3(p.general_wgs), dim3(256), 0, st, m->vert, m->ind,
                       (long long)m->grid_w, v, m->vis, m->gqueue, general, m->gcap, m->queue, items, m->qcap);
    ALP_HIP(hipGetLastError());
    hipLaunchKernelGGL((raster_large_kernel<IMPLICIT>), dim3(p.large_wgs), dim3(256), 0, st, m->vert, m->ind,
                       (long long)m->grid_w, v, m->vis, m->queue, items, m->qcap);
    ALP_HIP(hipGetLastError());
    return ALP_OK;
}

// what raster_grid_kernel parked in one round; the second round's entries follow the first round's in the queues
int drain_parked(alp_mesh *m, const View &v, const host::FramePlan &p, int round) {
    const unsigned *cap = round ? m->park_cap_b : m->park_cap;
    hipLaunchKernelGGL(raster_parked_kernel, dim3(p.parked_wgs[round]), dim3(256), 0, ctx().stream, v, m->vis,
                       m->park_small + (round ? m->park_cap[0] : 0), m->park_large + (round ? m->park_cap[1] : 0),
                       m->park_cell + (round ? m->park_cap[2] : 0), frame_counters(m, v) + QC_STRIDE * round + 2, cap[0], cap[1], cap[2]);
    ALP_HIP(hipGetLastError());
    return ALP_OK;
}

// Once per grid mesh, at its first frame: the parked queues and the tile plan (the vertices never change).
int ensure_grid_plan(alp_mesh *m, const host::FramePlan &p) {
    if (!m->park_small) {
        host::FrameQueues q;
        for (int k = 0; k < 3; ++k) q.park_b[k] = m->park_cap_b[k];
        host::initial_park_caps(initial_queue_cap(), &q);
        if (int e = alloc_park(m, q.park, q.park_b)) return e;
    }
    if (m->tile_bounds) return ALP_OK;
    // published only when both allocations and the launch succeeded: a half-made plan must not
    // make the next frame skip this block and read uninitialised boxes
    DeviceBuffer<float> tb;
    DeviceBuffer<unsigned> tl;
    if (int rc = reserve_all({(size_t)p.tile_bounds_bytes, (size_t)p.tile_lists_bytes}, tb, tl)) return rc;
    hipLaunchKernelGGL(tile_bounds_kernel, dim3((unsigned)p.tiles), dim3(256), 0, ctx().stream, m->vert, (int)m->grid_h,
                       (int)m->grid_w, p.tiles_x, tb);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ALP_EHIP, "frame plan of the mesh: %s", hipGetErrorString(e));
    m->tile_bounds = std::move(tb);
    m->tile_lists = std::move(tl);
    return ALP_OK;
}

// one round of raster_grid_kernel over a tile list: one workgroup per possible list entry, the ones beyond the list's length
// leave at once.  patch_words: the LDS depth patch (words of 8 bytes; 0 = none) -- the kernel's static LDS is 19 KB, 64 KB per
// workgroup in all.
int grid_round(alp_mesh *m, const View &v, const host::FramePlan &p, int round, int along_rows, const unsigned *list,
               const unsigned *list_count, int patch_words) {
    unsigned *fcount = frame_counters(m, v);
    const unsigned *cap = round ? m->park_cap_b : m->park_cap;
    hipLaunchKernelGGL(raster_grid_kernel, dim3(p.grid_wgs), dim3(256), (size_t)patch_words * 8, ctx().stream, m->vert, m->valid,
                       (int)m->grid_h, (int)m->grid_w, v, m->vis, m->gqueue, fcount + 1, m->gcap, along_rows, list, list_count,
                       m->park_small + (round ? m->park_cap[0] : 0), m->park_large + (round ? m->park_cap[1] : 0),
                       m->park_cell + (round ? m->park_cap[2] : 0), fcount + QC_STRIDE * round + 2, cap[0], cap[1], cap[2], patch_words);
    ALP_HIP(hipGetLastError());
    return ALP_OK;
}

// Coverage of a regular-grid mesh: tile plan, first round (the NEAR tiles: the occluders), depth pyramid and occlusion test of
// the FAR tiles, second round (the survivors), and the consumers of what the rounds set aside.
int draw_grid_mesh(alp_mesh *m, const View &v, const host::FramePlan &p) {
    hipStream_t st = ctx().stream;
    unsigned *near_list = m->tile_lists, *far_list = near_list + p.tiles, *second_list = far_list + p.tiles,
             *counts = frame_counters(m, v) + 2 * QC_STRIDE;   // [0] near, [1] far, [2] far survivors (cleared with the queue counters)
    TileCull cull;
    make_tile_cull(v, &cull);
    if (getenv("ALP_NO_TILE_CULL")) cull.enabled = 0;     // development: measure / cross-check the exact path alone
    if (getenv("ALP_NO_OCCLUSION")) cull.occlusion = 0;   // development: frustum culling only, one round
    // vertices are X, Z, Y: columns step X (R[0][0] on screen x), rows step Y (R[0][2])
    int along_rows = std::fabs(v.R[0][2]) > std::fabs(v.R[0][0]);
    if (const char *e = dev_getenv("ALP_GRID_LANES")) along_rows = e[0] == 'r';   // development override
    hipLaunchKernelGGL(tile_plan_kernel, dim3(p.plan_grid), dim3(256), 0, st, m->tile_bounds, (unsigned)p.tiles, cull, near_list,
                       far_list, counts, counts + 4);
    ALP_HIP(hipGetLastError());
    static const int patch_near = patch_words_env("ALP_PATCH_NEAR", PATCH_WORDS_NEAR),
                     patch_far = patch_words_env("ALP_PATCH_FAR", PATCH_WORDS_FAR);
    if (int e = grid_round(m, v, p, 0, along_rows, near_list, counts + 0, patch_near)) return e;
    if (int e = dev_report_first_round(st, counts)) return e;
    // The rare cases (near-plane crossings, triangles of 64 px and more) of BOTH rounds are drawn once, after
    // the second round's grid kernel: its general entries follow the first round's in the same queue.  The
    // pyramid then lacks those few triangles as occluders -- it stays conservative -- and a frame has two
    // launches fewer.
    const bool two_rounds = cull.enabled && cull.occlusion;
    if (!two_rounds)
        if (int e = drain_rare<true>(m, v, p, 0)) return e;
    if (int e = drain_parked(m, v, p, 0)) return e;
    if (two_rounds) {
        // depth pyramid of everything the first round drew, occlusion test of the far tiles, second round.
        // (Measured and not kept: building the pyramid BEFORE the first round's parked cells / triangles
        // are drawn and running the second round on a second stream next to them -- the parked geometry
        // is the main occluder, three times as many far tiles survive, 1.23 instead of 1.06 ms.)
        const HizDims dm = hiz_dims(v.w, v.h);
        hipLaunchKernelGGL(hiz_build_kernel, dim3((unsigned)dm.w[3], (unsigned)dm.h[3]), dim3(256), 0, st, m->vis, v.w, v.h, dm,
                           m->hiz, counts + 4);
        ALP_HIP(hipGetLastError());
        hipLaunchKernelGGL(tile_occlusion_kernel, dim3(p.plan_grid), dim3(256), 0, st, m->tile_bounds, cull, far_list, counts, dm,
                           m->hiz, second_list, counts + 2);
        ALP_HIP(hipGetLastError());
        if (int e = grid_round(m, v, p, 1, along_rows, second_list, counts + 2, patch_far)) return e;
        if (int e = drain_rare<true>(m, v, p, 0)) return e;      // round 0's counters: both rounds' entries
        if (int e = drain_parked(m, v, p, 1)) return e;
    }
    return dev_report_tiles(m, v, cull, p.tiles, p.plan_grid, two_rounds, counts);
}

// coverage of any other index array: one thread per triangle, then the rare cases
int draw_indexed_mesh(alp_mesh *m, const View &v, const host::FramePlan &p) {
    hipLaunchKernelGGL((raster_kernel<false>), dim3(p.index_grid), dim3(256), 0, ctx().stream, m->vert, m->ind, m->valid,
                       (long long)m->n_tri, (long long)m->grid_w, v, m->vis, m->gqueue, frame_counters(m, v) + 1, m->gcap);
    ALP_HIP(hipGetLastError());
    return drain_rare<false>(m, v, p, 0);
}

template <bool IMPLICIT>
int resolve_frame(alp_mesh *m, const View &v, const RemapCoef &rc, double min_distance, const host::FramePlan &p) {
    const int identity = rc.a1 == 1 && rc.a2 == 1 && rc.k1 == 0 && rc.k2 == 0 && rc.k3 == 0 && rc.k4 == 0 && rc.k5 == 0 &&
                         rc.k6 == 0 && rc.p1 == 0 && rc.p2 == 0 && rc.s1 == 0 && rc.s2 == 0 && rc.s3 == 0 && rc.s4 == 0 &&
                         rc.c0 > 0 && rc.c1 > 0;
    hipLaunchKernelGGL((resolve_kernel<IMPLICIT>), dim3(p.resolve_grid), dim3(256), 0, ctx().stream, m->vert,
                       m->coords_as_value ? nullptr : m->value, m->ind, (long long)m->grid_w, v, rc, identity, min_distance, m->vis,
                       m->image, frame_counters(m, v), m->n_tri > 0 ? m->qcount_host : nullptr);
    ALP_HIP(hipGetLastError());
    return ALP_OK;
}

// Enqueue one whole frame on the library stream, no host round trip: clear, raster passes (the
// queue lengths stay on the device), resolve.  The queue counters are copied to pinned host
// memory at the end (by the resolve); finish_frame() checks them before anything reads the frame.
// `resolve_only`: the visibility buffer (and the frame's counters behind it) already hold this view's finished
// raster passes -- only the resolve runs (the visibility cache, see alp_mesh::vis_current).
int render_impl(alp_mesh *m, const View &v, const RemapCoef &rc, double min_distance, bool resolve_only = false) {
    hipStream_t st = ctx().stream;
    const host::FramePlan p = frame_plan_of(m, v);
    m->vis_current = false;          // until every launch below has been accepted
    // one fill clears the visibility buffer AND the frame's queue / list counters, which live right behind it
    if (!resolve_only)
        ALP_HIP(hipMemsetAsync(m->vis, 0, (size_t)v.w * v.h * sizeof(unsigned long long) + QC_TOTAL * sizeof(unsigned), st));
    if (m->n_tri > 0 && !resolve_only) {
        if (m->implicit)
            if (int e = ensure_grid_plan(m, p)) return e;
        if (int e = m->implicit ? draw_grid_mesh(m, v, p) : draw_indexed_mesh(m, v, p)) return e;
    }
    if (int e = m->implicit ? resolve_frame<true>(m, v, rc, min_distance, p) : resolve_frame<false>(m, v, rc, min_distance, p)) return e;
    m->last_v = v;
    m->last_rc = rc;
    m->last_min_distance = min_distance;
    m->unchecked = m->n_tri > 0;
    m->vis_current = true;
    m->rz_n = -1;                    // a rasterisation plan belongs to the frame it was made for
    ++(resolve_only ? m->frames_resolve_only : m->frames_full);
    if (int e = dev_report_frame(st)) return e;
    m->rendered = true;
    return ALP_OK;
}

// everything of a View the raster passes read (the resolve's float64 members follow from the same parameters)
static bool same_view(const View &a, const View &b) {
    return a.w == b.w && a.h == b.h && a.fx == b.fx && a.fy == b.fy && a.sx == b.sx && a.sy == b.sy && a.fxd == b.fxd && a.fyd == b.fyd &&
           !memcmp(a.R, b.R, sizeof(a.R)) && !memcmp(a.camf, b.camf, sizeof(a.camf)) && !memcmp(a.caml, b.caml, sizeof(a.caml)) &&
           !memcmp(a.Rd, b.Rd, sizeof(a.Rd)) && !memcmp(a.camd, b.camd, sizeof(a.camd));
}

// Before anything reads the last frame: wait for it and make sure no queue overflowed (host::frame_verdict).  A
// queue that was too small is grown and the frame rendered again (max is idempotent, but the
// dropped entries were never drawn); the verdict on the grown queues with the same counters is "none", so a frame is
// redone only for entries that the redone frame itself newly asks for.
int finish_frame(alp_mesh *m) {
    while (m->unchecked) {
        ALP_HIP(hipStreamSynchronize(ctx().stream));
        m->unchecked = false;
        host::FrameQueues have;
        have.items = m->qcap;
        have.general = m->gcap;
        for (int k = 0; k < 3; ++k) {
            have.park[k] = m->park_cap[k];
            have.park_b[k] = m->park_cap_b[k];
        }
        const host::QueueVerdict want = host::frame_verdict(m->qcount_host, QC_STRIDE, m->park_small != nullptr, have);
        if (want.none()) break;
        if (want.park)
            if (int e = alloc_park(m, want.caps.park, want.caps.park_b)) return e;
        if (want.items)
            if (int e = ensure_queue(m, want.caps.items)) return e;
        if (want.general)
            if (int e = ensure_gqueue(m, want.caps.general)) return e;
        if (int e = render_impl(m, m->last_v, m->last_rc, m->last_min_distance)) return e;
    }
    return ALP_OK;
}

}  // namespace

int alp::finish_frame_of(alp_mesh *m) { return finish_frame(m); }

// n x 3 float32 or float64 host array -> n x 3 float32 on the device; float64 is staged through the library
// scratch in chunks and cast there (no host pass over the array, no float32 copy on the host)
int alp::upload_f32(float *dst, const void *src, int dtype, int64_t n_vert) {
    const size_t count = (size_t)n_vert * 3;
    if (dtype == ALP_F32) return upload_chunked(dst, src, count * 4);
    const size_t CH = (size_t)24 << 20;                 // doubles per chunk: 192 MB
    const size_t ch = count < CH ? count : CH;
    double *stage = nullptr;
    if (int rc = scratch_reserve(ch * 8, (void **)&stage)) return rc;
    hipStream_t st = ctx().stream;
    const hipError_t e = staged_upload(src, 8, (int64_t)count, (int64_t)ch, stage, [&](int64_t off, int64_t cnt) {
        hipLaunchKernelGGL(cast_f64_f32_kernel, dim3(4096), dim3(256), 0, st, stage, (long long)cnt, (long long)off, dst);
    });
    if (e != hipSuccess) return fail(ALP_EHIP, "float64 upload: %s", hipGetErrorString(e));
    ALP_HIP(hipStreamSynchronize(st));
    return ALP_OK;
}

// alp_mesh_create: is the host index array the full regular grid of row length gw?  Checked WHILE IT STREAMS through the
// staging buffer, chunks of whole triangles; nothing is stored.
static int streamed_grid_check(alp_mesh *m, const void *ind, int ind_dtype, int64_t n_tri, long long gw, bool *is_grid) {
    hipStream_t st = ctx().stream;
    const size_t esize = ind_dtype == ALP_I32 ? 4 : 8;
    const int64_t total = n_tri * 3;
    const int64_t CH = (int64_t)(((size_t)192 << 20) / esize) / 3 * 3;      // whole triangles per chunk
    const int64_t ch = total < CH ? total : CH;
    void *stage = nullptr;
    if (int rc = scratch_reserve((size_t)ch * esize, &stage)) return rc;
    hipError_t e = hipMemsetAsync(m->qcount_dev, 0, sizeof(unsigned), st);
    if (e == hipSuccess)
        e = staged_upload(ind, esize, total, ch, stage, [&](int64_t off, int64_t cnt) {
            if (ind_dtype == ALP_I32)
                hipLaunchKernelGGL(check_grid_chunk_kernel<int>, dim3(4096), dim3(256), 0, st, (const int *)stage, cnt / 3, off / 3, gw, m->qcount_dev);
            else
                hipLaunchKernelGGL(check_grid_chunk_kernel<long long>, dim3(4096), dim3(256), 0, st, (const long long *)stage, cnt / 3, off / 3, gw,
                                   m->qcount_dev);
        });
    if (e == hipSuccess) e = hipMemcpyAsync(m->qcount_host, m->qcount_dev, sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ALP_EHIP, "grid check: %s", hipGetErrorString(e));
    *is_grid = *m->qcount_host == 0;
    return ALP_OK;
}

// alp_mesh_create: the index array of m->n_tri triangles as int32 on the device, every index checked against the vertex count
static int upload_indices(alp_mesh *m, const void *ind, int ind_dtype) {
    hipStream_t st = ctx().stream;
    const long long n_vert = m->n_vert;
    if (int rc = m->ind.reserve((size_t)m->n_tri * 12)) return rc;
    if (hipMemsetAsync(m->qcount_dev, 0, sizeof(unsigned), st) != hipSuccess) return fail(ALP_EHIP, "index check: memset");
    const int64_t total = m->n_tri * 3;
    hipError_t e = hipSuccess;
    if (ind_dtype == ALP_I32) {
        if (int rc = upload_chunked(m->ind, ind, (size_t)total * 4)) return rc;
        hipLaunchKernelGGL(check_index_range_kernel, dim3(4096), dim3(256), 0, st, m->ind, (long long)total, n_vert, m->qcount_dev);
    } else {
        // int64 (what numpy builds, surface.py:194-201; project.py:215 casts with astype("i4")): narrowed on the
        // device, staged through the library scratch in chunks of 192 MB
        const int64_t CH = 24 << 20;
        const int64_t ch = total < CH ? total : CH;
        long long *stage = nullptr;
        if (int rc = scratch_reserve((size_t)ch * 8, (void **)&stage)) return rc;
        e = staged_upload(ind, 8, total, ch, stage, [&](int64_t off, int64_t cnt) {
            hipLaunchKernelGGL(narrow_indices_kernel, dim3(4096), dim3(256), 0, st, stage, (long long)cnt, (long long)off, m->ind, n_vert,
                               m->qcount_dev);
        });
    }
    // range check (an out-of-range index would fault in the kernels): counted by the kernels above
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(m->qcount_host, m->qcount_dev, sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ALP_EHIP, "index upload: %s", hipGetErrorString(e));
    if (*m->qcount_host == 0) return ALP_OK;
    // name the first offender like the host check did (cold path: a scan of the caller's array)
    for (int64_t i = 0; i < total; ++i) {
        const long long v = ind_dtype == ALP_I32 ? (long long)((const int *)ind)[i] : ((const long long *)ind)[i];
        if (v < 0 || v >= n_vert) return fail(ALP_EINVAL, "index %lld out of range at %lld", v, (long long)i);
    }
    return fail(ALP_EINVAL, "%u indices out of range", *m->qcount_host);
}

// Regular-grid recognition in a host index array (HostGridCheck, host_check_threads, grid_candidate): host/alp_host.h --
// HIP-free, so that its threads run under the sanitizers on the CPU build.
using alp::host::HostGridCheck;
using alp::host::host_check_threads;

extern "C" {

int alp_mesh_create(const void *vert, int vert_dtype, const void *value, int value_dtype, int64_t n_vert, const void *ind,
                    int ind_dtype, int64_t n_tri, int64_t grid_h, int64_t grid_w, alp_mesh_t **out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(out, "out is NULL");
    *out = nullptr;
    ALP_REQUIRE(vert && n_vert > 0, "vert is NULL or empty");
    ALP_REQUIRE(vert_dtype == ALP_F32 || vert_dtype == ALP_F64, "vert_dtype must be ALP_F32 or ALP_F64");
    ALP_REQUIRE(!value || value_dtype == ALP_F32 || value_dtype == ALP_F64, "value_dtype must be ALP_F32 or ALP_F64");
    ALP_REQUIRE(n_vert < ((int64_t)1 << 31), "more than 2^31 vertices");
    const bool implicit = ind == nullptr;
    if (implicit) {
        ALP_REQUIRE(grid_h >= 2 && grid_w >= 2 && grid_h * grid_w == n_vert, "implicit grid: grid_h*grid_w != n_vert");
        n_tri = 2 * (grid_h - 1) * (grid_w - 1);
    } else {
        ALP_REQUIRE(ind_dtype == ALP_I32 || ind_dtype == ALP_I64, "ind_dtype must be ALP_I32 or ALP_I64");
        ALP_REQUIRE(n_tri >= 0, "n_tri is negative");
    }
    ALP_REQUIRE(n_tri < ((int64_t)1 << 32) - 1, "more than 2^32-2 triangles");
    alp_mesh *m = new alp_mesh();
    m->n_vert = n_vert;
    m->n_tri = n_tri;
    m->grid_h = grid_h;
    m->grid_w = grid_w;
    m->implicit = implicit;
    int rc = ALP_OK;
    auto bail = [&](int code) { alp_mesh_destroy(m); return code; };
    // The index array the reference builds (surface.py:194-201) is the full regular grid unless nodata triangles were
    // filtered out: an array with the grid's first triangle and exactly its triangle count is a candidate
    const bool detect = !getenv("ALP_NO_GRID_DETECT");       // env: keep the index path (tests, benchmarks)
    long long cand_gh = 0, cand_gw = 0;
    if (!implicit && detect) host::grid_candidate(ind, ind_dtype, n_tri, n_vert, &cand_gh, &cand_gw);
    HostGridCheck host_check;                 // its destructor joins on every way out of this function
    if (cand_gw) {
        const int T = host_check_threads(n_tri);
        if (T > 0) host_check.start(ind, ind_dtype, cand_gh, cand_gw, T);
    }
    if ((rc = m->vert.reserve((size_t)n_vert * 12))) return bail(rc);
    if ((rc = upload_f32(m->vert, vert, vert_dtype, n_vert))) return bail(rc);
    if (value) {
        if ((rc = m->value.reserve((size_t)n_vert * 12))) return bail(rc);
        if ((rc = upload_f32(m->value, value, value_dtype, n_vert))) return bail(rc);
    }
    const size_t counters = QC_TOTAL * sizeof(unsigned);
    if ((rc = reserve_all({counters, counters}, m->qcount_dev, m->qcount_host))) return bail(rc);
    // ... checked by the host threads started above while the vertices were uploaded -- then the array never crosses
    // PCIe -- or, where there are no threads to spare, WHILE IT STREAMS through the staging buffer; either way a full
    // grid is never stored: no 12 B/triangle buffer is allocated, nothing is narrowed or written, and the mesh is
    // rendered by the LDS-tiled grid kernels (same triangle ids, same result, no index traffic).  An array that only
    // starts like the grid takes the general path below.
    bool streamed_grid = false;
    if (cand_gw) {
        const long long gh = cand_gh, gw = cand_gw;
        if (host_check.started) streamed_grid = host_check.is_grid();
        else if ((rc = streamed_grid_check(m, ind, ind_dtype, n_tri, gw, &streamed_grid))) return bail(rc);
        if (streamed_grid) {
            m->implicit = true;
            m->grid_h = gh;
            m->grid_w = gw;
        }
    }
    const bool want_ind = !implicit && n_tri > 0 && !streamed_grid;
    if (want_ind)
        if ((rc = upload_indices(m, ind, ind_dtype))) return bail(rc);
    if ((rc = ensure_queue(m, initial_queue_cap()))) return bail(rc);
    if ((rc = ensure_gqueue(m, initial_queue_cap()))) return bail(rc);
    // ... and when they were (surface.py:203-205), the grid with a vertex mask
    if (!implicit && !m->implicit && n_tri >= 1 && detect) {
        long long first[3];
        for (int k = 0; k < 3; ++k)
            first[k] = ind_dtype == ALP_I32 ? (long long)((const int *)ind)[k] : ((const long long *)ind)[k];
        if ((rc = try_subgrid(m, first))) return bail(rc);
    }
    *out = m;
    return ALP_OK;
}

int alp_mesh_info(alp_mesh_t *m, int64_t info[4]) {
    ALP_REQUIRE(m && info, "NULL argument");
    info[0] = m->implicit ? 1 : 0;
    info[1] = m->grid_h;
    info[2] = m->grid_w;
    info[3] = m->n_tri;
    return ALP_OK;
}

int alp_mesh_destroy(alp_mesh_t *m) {
    if (!m) return ALP_OK;
    if (ctx().ready) hipStreamSynchronize(ctx().stream);
    delete m;
    return ALP_OK;
}

int alp_render_enqueue(alp_mesh_t *m, const double params[ALP_NPARAM], const double *offsets, double min_distance) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(m && params, "NULL argument");
    ALP_REQUIRE(params[21] >= 1 && params[22] >= 1 && params[21] <= 32768 && params[22] <= 32768,
                "image size w,h must be in [1, 32768]");
    View v;
    RemapCoef rc;
    make_view(params, offsets, &v, &rc);
    if (int e = ensure_frame(m, v.w, v.h)) return e;
    // same view as the frame whose visibility buffer is still there: the raster passes would rebuild it bit for bit
    const bool no_cache = getenv("ALP_NO_VIS_CACHE") != nullptr;      // tests, benchmarks: force the full frame
    const bool cached = m->vis_current && !no_cache && same_view(v, m->last_v);
    if (!m->ev_frame[0]) {       // both or neither
        Event a, b;
        if (int e = a.ensure()) return e;
        if (int e = b.ensure()) return e;
        m->ev_frame[0] = std::move(a);
        m->ev_frame[1] = std::move(b);
    }
    ALP_HIP(hipEventRecord(m->ev_frame[0], ctx().stream));
    const int e = render_impl(m, v, rc, min_distance, cached);
    if (e) return e;
    ALP_HIP(hipEventRecord(m->ev_frame[1], ctx().stream));
    return ALP_OK;
}

int alp_mesh_frame_ms(alp_mesh_t *m, float *ms) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(m && ms, "NULL argument");
    if (!m->rendered || !m->ev_frame[1]) return fail(ALP_ESTATE, "alp_mesh_frame_ms: nothing rendered yet");
    ALP_HIP(hipEventSynchronize(m->ev_frame[1]));
    ALP_HIP(hipEventElapsedTime(ms, m->ev_frame[0], m->ev_frame[1]));
    return ALP_OK;
}

int alp_mesh_trim(alp_mesh_t *m) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(m, "mesh handle is NULL");
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    m->rz_work.reset();
    m->rz_points.reset();
    m->rz_n = -1;
    return ALP_OK;
}

int alp_render_fetch(alp_mesh_t *m, float *out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(m && out, "NULL argument");
    if (!m->rendered) return fail(ALP_ESTATE, "alp_render_fetch: nothing rendered yet");
    if (int e = finish_frame(m)) return e;
    ALP_HIP(hipMemcpyAsync(out, m->image, (size_t)m->w * m->h * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx().stream));
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    return ALP_OK;
}

int alp_render_fetch_u8(alp_mesh_t *m, float scale, int reverse_channels, uint8_t *out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(m && out, "NULL argument");
    if (!m->rendered) return fail(ALP_ESTATE, "alp_render_fetch_u8: nothing rendered yet");
    if (int e = finish_frame(m)) return e;
    const long long npix = (long long)m->w * m->h;
    unsigned char *dev = nullptr;
    if (int rc = scratch_reserve((size_t)npix * 3, (void **)&dev)) return rc;
    hipLaunchKernelGGL(image_u8_kernel, dim3(ctx().cu_count * 16), dim3(256), 0, ctx().stream, m->image, npix, scale,
                       reverse_channels, dev);
    ALP_HIP(hipGetLastError());
    ALP_HIP(hipMemcpyAsync(out, dev, (size_t)npix * 3, hipMemcpyDeviceToHost, ctx().stream));
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    return ALP_OK;
}

int alp_render_fetch_visibility(alp_mesh_t *m, uint64_t *out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(m && out, "NULL argument");
    if (!m->rendered) return fail(ALP_ESTATE, "alp_render_fetch_visibility: nothing rendered yet");
    if (int e = finish_frame(m)) return e;
    const unsigned long long *src = m->vis;
    if (m->tri_present) {                    // filtered grid: the caller's triangle numbering
        const long long npix = (long long)m->w * m->h;
        unsigned long long *tr = nullptr;
        if (int rc = scratch_reserve((size_t)npix * sizeof(uint64_t), (void **)&tr)) return rc;
        hipLaunchKernelGGL(vis_translate_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, ctx().stream, m->vis, npix,
                           m->tri_present, m->tri_rank, tr);
        ALP_HIP(hipGetLastError());
        src = tr;
    }
    ALP_HIP(hipMemcpyAsync(out, src, (size_t)m->w * m->h * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx().stream));
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    return ALP_OK;
}

int alp_render_gather(alp_mesh_t *m, const int32_t *u, const int32_t *v, int64_t n, const double *offsets,
                      double *xyz_out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(m, "mesh handle is NULL");
    ALP_REQUIRE(n >= 0, "n is negative");
    if (!m->rendered) return fail(ALP_ESTATE, "alp_render_gather: nothing rendered yet");
    if (int e = finish_frame(m)) return e;
    if (n == 0) return ALP_OK;
    ALP_REQUIRE(u && v && xyz_out, "NULL argument");
    char *dev = nullptr;
    const size_t uv_bytes = (size_t)n * sizeof(int32_t), xyz_bytes = (size_t)n * 3 * sizeof(double);
    if (int rc = scratch_reserve(xyz_bytes + 2 * uv_bytes, (void **)&dev)) return rc;
    double *xyz_dev = (double *)dev;
    int32_t *u_dev = (int32_t *)(dev + xyz_bytes), *v_dev = u_dev + n;
    hipStream_t st = ctx().stream;
    const double o0 = offsets ? offsets[0] : 0.0, o1 = offsets ? offsets[1] : 0.0, o2 = offsets ? offsets[2] : 0.0;
    hipError_t e = hipMemcpyAsync(u_dev, u, uv_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(v_dev, v, uv_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        hipLaunchKernelGGL(gather_pixels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, m->image, m->w,
                           m->h, u_dev, v_dev, n, o0, o1, o2, xyz_dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(xyz_out, xyz_dev, xyz_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ALP_EHIP, "alp_render_gather: %s", hipGetErrorString(e));
    return ALP_OK;
}

int alp_distance_mask(const double *xyz, int64_t n, const double camera[3], double min_distance, double max_distance,
                      uint8_t *keep) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(n >= 0, "n is negative");
    if (n == 0) return ALP_OK;
    ALP_REQUIRE(xyz && camera && keep, "NULL argument");
    ALP_REQUIRE(!(min_distance < 0), "min_distance must be non-negative");
    ALP_REQUIRE(!(max_distance < min_distance), "max_distance must be >= min_distance");
    char *dev = nullptr;
    const size_t xyz_bytes = (size_t)n * 3 * sizeof(double);
    if (int rc = scratch_reserve(xyz_bytes + (size_t)n, (void **)&dev)) return rc;
    unsigned char *keep_dev = (unsigned char *)(dev + xyz_bytes);
    hipStream_t st = ctx().stream;
    hipError_t e = hipMemcpyAsync(dev, xyz, xyz_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        KTimeScope kt;
        hipLaunchKernelGGL(distance_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double *)dev,
                           (long long)n, camera[0], camera[1], camera[2], min_distance, max_distance, keep_dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(keep, keep_dev, (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ALP_EHIP, "alp_distance_mask: %s", hipGetErrorString(e));
    return ALP_OK;
}

int alp_render_valid_count(alp_mesh_t *m, int64_t *count) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(m && count, "NULL argument");
    if (!m->rendered) return fail(ALP_ESTATE, "alp_render_valid_count: nothing rendered yet");
    return frame_valid_count(m, count);
}

// prologue of the three alp_render_fetch_valid*: the count alp_render_valid_count left, taken (it serves one fetch)
static int take_valid_total(alp_mesh_t *m, const char *who, int64_t *M) {
    if (int rc = require_init()) return rc;
    if (!m) return fail(ALP_EINVAL, "%s: mesh handle is NULL", who);
    if (m->valid_total < 0) return fail(ALP_ESTATE, "%s: call alp_render_valid_count first", who);
    *M = m->valid_total;
    m->valid_total = -1;
    return ALP_OK;
}

int alp_render_fetch_valid(alp_mesh_t *m, const double *offsets, uint32_t *idx_out, double *xyz_out) {
    int64_t M = 0;
    if (int rc = take_valid_total(m, __func__, &M)) return rc;
    if (M == 0) return ALP_OK;
    ALP_REQUIRE(idx_out && xyz_out, "output is NULL");
    char *dev = nullptr;
    const size_t xyz_bytes = (size_t)M * 3 * sizeof(double), idx_bytes = (size_t)M * sizeof(unsigned);
    if (int rc = scratch_reserve(xyz_bytes + idx_bytes, (void **)&dev)) return rc;
    double *xyz_dev = (double *)dev;
    unsigned *idx_dev = (unsigned *)(dev + xyz_bytes);
    hipStream_t st = ctx().stream;
    if (int rc = frame_valid_write(m, offsets, idx_dev, xyz_dev, false)) return rc;
    hipError_t e = hipMemcpyAsync(xyz_out, xyz_dev, xyz_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(idx_out, idx_dev, idx_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ALP_EHIP, "alp_render_fetch_valid: %s", hipGetErrorString(e));
    return ALP_OK;
}

int alp_render_fetch_valid_planes(alp_mesh_t *m, const double *offsets, uint32_t *idx_out, double *x_out, double *y_out, double *z_out) {
    int64_t M = 0;
    if (int rc = take_valid_total(m, __func__, &M)) return rc;
    if (M == 0) return ALP_OK;
    ALP_REQUIRE(idx_out && x_out && y_out && z_out, "output is NULL");
    char *dev = nullptr;
    const size_t plane = (size_t)M * sizeof(double), idx_bytes = (size_t)M * sizeof(unsigned);
    if (int rc = scratch_reserve(3 * plane + idx_bytes, (void **)&dev)) return rc;
    double *xyz_dev = (double *)dev;
    unsigned *idx_dev = (unsigned *)(dev + 3 * plane);
    hipStream_t st = ctx().stream;
    m->valid_total_planes = M;
    if (int rc = frame_valid_write(m, offsets, idx_dev, xyz_dev, true)) return rc;
    hipError_t e = hipMemcpyAsync(x_out, xyz_dev, plane, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(y_out, xyz_dev + M, plane, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(z_out, xyz_dev + 2 * M, plane, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(idx_out, idx_dev, idx_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ALP_EHIP, "alp_render_fetch_valid_planes: %s", hipGetErrorString(e));
    return ALP_OK;
}

int alp_render_fetch_valid_table(alp_mesh_t *m, const double *offsets, const void *array, int array_dtype, int64_t channels,
                                 int64_t *index_out, int16_t *u_out, int16_t *v_out, double *block_out) {
    int64_t M = 0;
    if (int rc = take_valid_total(m, __func__, &M)) return rc;
    if (M == 0) return ALP_OK;
    ALP_REQUIRE(index_out && u_out && v_out && block_out, "output is NULL");
    ALP_REQUIRE(channels >= 0 && channels <= 64, "channel count out of range");
    ALP_REQUIRE(channels == 0 || array, "array is NULL");
    ALP_REQUIRE(array_dtype == ALP_U8 || array_dtype == ALP_U16 || array_dtype == ALP_F32 || array_dtype == ALP_F64,
                "array_dtype must be ALP_U8, ALP_U16, ALP_F32 or ALP_F64");
    const size_t esize = array_dtype == ALP_U8 ? 1 : array_dtype == ALP_U16 ? 2 : array_dtype == ALP_F32 ? 4 : 8;
    const size_t npix = (size_t)m->w * m->h, arr_bytes = npix * (size_t)channels * esize;
    // block (x | y | z | channels: float64 rows of M) | labels (int64) | pixel index (u32) | u | v (int16) | the caller's array
    const size_t plane = (size_t)M * sizeof(double);
    const size_t block_bytes = (3 + (size_t)channels) * plane;
    const size_t small = (size_t)M * (8 + 4 + 2 + 2);
    char *dev = nullptr;
    if (int rc = scratch_reserve(block_bytes + small + 256 + arr_bytes + 256, (void **)&dev)) return rc;
    double *block_dev = (double *)dev;
    long long *index_dev = (long long *)(dev + block_bytes);
    unsigned *idx_dev = (unsigned *)(index_dev + M);
    short *u_dev = (short *)(idx_dev + M), *v_dev = u_dev + M;
    char *arr_dev = (char *)(((uintptr_t)(v_dev + M) + 255) & ~(uintptr_t)255);
    hipStream_t st = ctx().stream;
    if (arr_bytes)
        if (int rc = upload_chunked(arr_dev, array, arr_bytes)) return rc;
    m->valid_total_planes = M;
    if (int rc = frame_valid_write(m, offsets, idx_dev, block_dev, true)) return rc;
    {
        KTimeScope kt;
        const dim3 grid((unsigned)((M + 255) / 256));
#define ALP_COLUMNS(A) hipLaunchKernelGGL(table_columns_kernel<A>, grid, dim3(256), 0, st, idx_dev, (long long)M, m->w, (const A *)arr_dev, \
                                          (int)channels, index_dev, u_dev, v_dev, block_dev + 3 * M)
        if (array_dtype == ALP_U8) ALP_COLUMNS(unsigned char);
        else if (array_dtype == ALP_U16) ALP_COLUMNS(unsigned short);
        else if (array_dtype == ALP_F32) ALP_COLUMNS(float);
        else ALP_COLUMNS(double);
#undef ALP_COLUMNS
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(block_out, block_dev, block_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(index_out, index_dev, (size_t)M * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(u_out, u_dev, (size_t)M * 2, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(v_out, v_dev, (size_t)M * 2, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ALP_EHIP, "alp_render_fetch_valid_table: %s", hipGetErrorString(e));
    return ALP_OK;
}

int alp_render(alp_mesh_t *m, const double params[ALP_NPARAM], const double *offsets, double min_distance, float *out) {
    if (int rc = alp_render_enqueue(m, params, offsets, min_distance)) return rc;
    return alp_render_fetch(m, out);
}

// stand-alone distort(): the inverted coefficients of an h x w image (only they and the size matter of the view) and the
// grid of its kernels
static void distort_setup(int64_t h, int64_t w, const double coeffs[14], RemapCoef *rc, int *grid) {
    double p[ALP_NPARAM] = {0};
    for (int i = 0; i < 14; ++i) p[7 + i] = coeffs[i];
    p[3] = 60; p[21] = (double)w; p[22] = (double)h;
    View v;
    make_view(p, nullptr, &v, rc);
    const long long want = ((long long)h * w + 255) / 256;
    *grid = (int)(want < 4096 ? want : 4096);
}

int alp_distort_image(const float *img, int64_t h, int64_t w, int64_t c, const double coeffs[14], float *out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(img && out && coeffs, "NULL argument");
    ALP_REQUIRE(h >= 1 && w >= 1 && c >= 1 && h <= 32768 && w <= 32768, "bad image shape");
    RemapCoef rc;
    int grid = 0;
    distort_setup(h, w, coeffs, &rc, &grid);
    const size_t bytes = (size_t)h * w * c * sizeof(float);
    float *dev = nullptr;
    if (int e2 = scratch_reserve(2 * bytes, (void **)&dev)) return e2;
    hipError_t e = hipMemcpyAsync(dev, img, bytes, hipMemcpyHostToDevice, ctx().stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(distort_image_kernel, dim3(grid), dim3(256), 0, ctx().stream, dev, (int)w, (int)h, (int)c, rc,
                           (float *)((char *)dev + bytes));
        e = hipMemcpyAsync(out, (char *)dev + bytes, bytes, hipMemcpyDeviceToHost, ctx().stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx().stream);
    if (e != hipSuccess) return fail(ALP_EHIP, "alp_distort_image: %s", hipGetErrorString(e));
    return ALP_OK;
}

int alp_distort_map(int64_t h, int64_t w, const double coeffs[14], float *map_x, float *map_y) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(coeffs && map_x && map_y, "NULL argument");
    ALP_REQUIRE(h >= 1 && w >= 1 && h <= 32768 && w <= 32768, "bad image shape");
    RemapCoef rc;
    int grid = 0;
    distort_setup(h, w, coeffs, &rc, &grid);
    const size_t bytes = (size_t)h * w * sizeof(float);
    float *dev = nullptr;
    if (int e2 = scratch_reserve(2 * bytes, (void **)&dev)) return e2;
    hipLaunchKernelGGL(distort_map_kernel, dim3(grid), dim3(256), 0, ctx().stream, (int)w, (int)h, rc, dev, dev + (size_t)h * w);
    ALP_HIP(hipGetLastError());
    ALP_HIP(hipMemcpyAsync(map_x, dev, bytes, hipMemcpyDeviceToHost, ctx().stream));
    ALP_HIP(hipMemcpyAsync(map_y, dev + (size_t)h * w, bytes, hipMemcpyDeviceToHost, ctx().stream));
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    return ALP_OK;
}

int alp_render_load(alp_mesh_t *m, const float *image, int64_t h, int64_t w) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(m && image, "NULL argument");
    ALP_REQUIRE(h >= 1 && w >= 1 && h <= 32768 && w <= 32768, "image size w,h must be in [1, 32768]");
    if (m->unchecked) ALP_HIP(hipStreamSynchronize(ctx().stream));
    m->unchecked = false;
    if (int e = ensure_frame(m, (int)w, (int)h)) return e;
    if (int e = upload_chunked(m->image, image, (size_t)h * w * 3 * sizeof(float))) return e;
    ALP_HIP(hipMemsetAsync(m->vis, 0, (size_t)h * w * sizeof(unsigned long long), ctx().stream));   // no visibility belongs to it
    m->vis_current = false;
    m->rz_n = -1;
    m->rendered = true;
    m->valid_total = -1;
    return ALP_OK;
}

}  // extern "C"
