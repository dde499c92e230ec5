// libalproj_hip.so -- device-resident point sets and the three kernels that run on them:
//   project_kernel   forward projection of every point with ONE pose (HBM-bound stream)
//   popeval_kernel   P candidate poses x every point -> per-candidate loss sums
//                    (VALU-bound; candidates staged in LDS, wave64 DPP reductions)
//   popeval_counted_kernel  its body in float64 on a float32 set's planes: argmin confirmation and mend pass (counted_pass)
//   residual_batch_kernel  observed - projected for B poses, interleaved (least-squares path)
//   jacobian_kernel  d projected / d parameters for one pose, exact (least-squares path)
//   normal_poses_kernel  the same rows contracted to J^T J, J^T r and the cost where they are made (f64 MFMA; least-squares path),
//                    for B >= 1 poses in one launch, one workgroup per (stripe, pose) pair: every pose under the set's
//                    weights or under a row of its weight table (alp_points_set_weight_table), all B or the listed ones (alp_lm.hip)
//   residuals_assigned_kernel  observed - projected with the pose chosen per point (held-out residuals of a cross-validation)
//
// Reference arithmetic: src/alproj/optimize.py  project :122-155, _distort :98-120,
// rmse :157-178, huber_loss :181-212, compute_residuals :215-237, and the generation loop
// of CMAOptimizer.optimize :418-424.  The pose-dependent scalars are folded on the host in
// float64 (alp_core.hip: fold_pose); everything per point happens here.
//
// Data layout in HBM: structure-of-arrays planes x[], y[], z[] (local coordinates =
// absolute - origin), observed uo[], vo[] and projected u[], v[] (pixels), all of one
// element type T (float: 20 B/vertex streamed per projection pass; double: 40 B/vertex).
// Planes are padded to a multiple of 1024 elements so that 16-byte vector accesses and
// whole-workgroup tiles never leave the allocation.
// The launch shapes (popeval_kernel's stripes x tiles, the residual / Jacobian chunks, normal_poses_kernel's stripes per pose, streaming grids, RowDiv) are planned in
// host/alp_plan.h, HIP-free and checked on the CPU; this unit allocates, records events and launches what it plans.
#include "alp_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "alp_point_kernels.h"
#include "alp_points_internal.h"


using namespace alp;

// argmin confirmation of float32 point sets: CONFIRM_MAX, CONFIRM_GAP and the selection itself live in host/alp_host.h
using alp::host::CONFIRM_MAX;

namespace {

// k planes of n_pad elements in ONE zeroed allocation (n_pad is a multiple of 1024 elements: every plane starts 4 KB-aligned)
int alloc_planes(DeviceBuffer<> &slab, int k, int64_t n_pad, size_t es, void **planes[]) {
    if (int rc = slab.reserve((size_t)k * n_pad * es)) return rc;
    ALP_HIP(hipMemsetAsync(slab, 0, (size_t)k * n_pad * es, ctx().stream));
    for (int i = 0; i < k; ++i) *planes[i] = (char *)slab + (size_t)i * n_pad * es;
    return ALP_OK;
}

// One host COLUMN (n contiguous values of TIn) -> one device plane of T, minus its origin component in float64: the columns of a
// table as they lie (a pandas block is columns x rows: a DataFrame's x, y, z are three contiguous runs), no host-side
// interleaving.
template <typename TIn, typename T>
__global__ __launch_bounds__(256) void column_to_plane_kernel(const TIn *__restrict__ src, int64_t count, int64_t dst_off, double o,
                                                              T *__restrict__ plane) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
        plane[dst_off + i] = (T)((double)src[i] - o);
}

// The staged upload: each of the `nsrc` host arrays of n items x `width` values crosses PCIe in chunks of at most CH items into
// ONE device staging buffer, and launch(source, stage, count, offset, grid) spreads a chunk over the planes.
template <typename TIn, typename Launch>
int staged_upload(const void *const *srcs, int nsrc, int64_t n, int width, int64_t CH, Launch launch) {
    const int64_t ch = n < CH ? (n > 0 ? n : 1) : CH;
    DeviceBuffer<TIn> stage;
    if (int rc = stage.reserve((size_t)ch * width * sizeof(TIn))) return rc;
    int rc = ALP_OK;
    for (int c = 0; c < nsrc && !rc; ++c)
        for (int64_t off = 0; off < n; off += ch) {
            const int64_t cnt = (n - off < ch) ? (n - off) : ch;
            hipError_t e = hipMemcpyAsync(stage, (const TIn *)srcs[c] + off * width, (size_t)cnt * width * sizeof(TIn),
                                          hipMemcpyHostToDevice, ctx().stream);
            if (e != hipSuccess) { rc = fail(ALP_EHIP, "H2D upload: %s", hipGetErrorString(e)); break; }
            launch(c, stage, cnt, off, (int)((cnt + 255) / 256 < 4096 ? (cnt + 255) / 256 : 4096));
            e = hipGetLastError();                    // the staging buffer is reused in stream order: no host sync per chunk
            if (e != hipSuccess) { rc = fail(ALP_EHIP, "upload kernel: %s", hipGetErrorString(e)); break; }
        }
    if (hipStreamSynchronize(ctx().stream) != hipSuccess && !rc) rc = fail(ALP_EHIP, "upload: stream failed");
    return rc;          // (`stage` is released here, behind the synchronisation)
}

// C planes from the C columns cols[] as they lie, or (cols == NULL) from `rows`, n x C row-major; o[0..3) = the origin
template <typename TIn, typename T, int C>
int upload_t(const void *rows, const void *const *cols, int64_t n, const double *o, void *const *planes) {
    if (cols)       // values per staging chunk: 48 M (192 MB of float32)
        return staged_upload<TIn>(cols, C, n, 1, (int64_t)48 << 20, [&](int c, const TIn *stage, int64_t cnt, int64_t off, int grid) {
            hipLaunchKernelGGL((column_to_plane_kernel<TIn, T>), dim3(grid), dim3(256), 0, ctx().stream, stage, cnt, off, o[c], (T *)planes[c]);
        });
    // points per staging chunk: 16 M (192 MB of float32 triples).  Measured on the MI355X box (tools/h2d_rate.hip):
    // one pageable hipMemcpy sustains 56 GB/s at this size, 48 MB chunks with a host sync each 36 GB/s.
    return staged_upload<TIn>(&rows, 1, n, C, (int64_t)16 << 20, [&](int, const TIn *stage, int64_t cnt, int64_t off, int grid) {
        hipLaunchKernelGGL((aos_to_planes_kernel<TIn, T, C>), dim3(grid), dim3(256), 0, ctx().stream, stage, cnt, off, o[0], o[1], o[2],
                           (T *)planes[0], (T *)planes[1], (T *)planes[2]);
    });
}

template <int C>
int upload(const void *rows, const void *const *cols, int in_dtype, int64_t n, const double *o, int precision, void *const *planes) {
    if (in_dtype == ALP_F64 && precision == ALP_F64) return upload_t<double, double, C>(rows, cols, n, o, planes);
    if (in_dtype == ALP_F64 && precision == ALP_F32) return upload_t<double, float, C>(rows, cols, n, o, planes);
    if (in_dtype == ALP_F32 && precision == ALP_F64) return upload_t<float, double, C>(rows, cols, n, o, planes);
    if (in_dtype == ALP_F32 && precision == ALP_F32) return upload_t<float, float, C>(rows, cols, n, o, planes);
    return fail(ALP_EINVAL, "in_dtype must be ALP_F32 or ALP_F64");
}

int stream_grid(int64_t items) { return host::stream_grid(items, ctx().cu_count); }

// ------------------------------------------------------------------ grid recognition (K1's grid form)
// A DSM's vertex list is its raster flattened row-major (meshgrid(x, y)): x depends on the column alone and y on the row alone,
// and since the planes are float(double(in) - origin) element by element, a column's x and a row's y have the same bits in
// every point that shares them.  The check runs on the planes as uploaded, so it sees exactly what K1 reads:
//   W = the first index i with bits(y[i]) != bits(y[0]);
//   every i < n: bits(x[i]) == bits(x[i % W]) and bits(y[i]) == bits(y[(i / W) * W])  (a shorter last row is fine).
// The plane path stays when: ALP_NO_POINTS_GRID is set; n < 2 or every y equals y[0] (a single row); W > GRID_MAX_ROW (the
// column table would no longer stay in L2); n_pad > 2^31 (the kernel's row / column arithmetic is 32-bit: RowDiv).
constexpr uint32_t GRID_MAX_ROW = 64 << 10;
constexpr uint32_t GRID_NONE = 0xffffffffu;

// bits: uint32_t (float planes) or uint64_t (double planes).  flags[0] (GRID_NONE beforehand) = the first index i < n whose y
// differs from y[0]: a thread stops at its first such index, the wave takes the minimum, one atomic per wave.
template <typename B>
__global__ __launch_bounds__(256) void grid_row_length_kernel(const B *__restrict__ y, uint32_t n, uint32_t *flags) {
    const B y0 = y[0];
    uint32_t first = GRID_NONE;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (y[i] != y0) {
            first = i;
            break;
        }
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)first, m);
        first = o < first ? o : first;
    }
    if ((threadIdx.x & 63) == 0 && first != GRID_NONE) atomicMin(flags, first);
}

// flags[1] (0 beforehand) = 1 when some point is off the grid of row length rd.w
template <typename B>
__global__ __launch_bounds__(256) void grid_verify_kernel(const B *__restrict__ x, const B *__restrict__ y, uint32_t n, RowDiv rd,
                                                          uint32_t *flags) {
    bool ok = true;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t r = rd.div(i);
        ok &= (x[i] == x[i - r * rd.w]) & (y[i] == y[r * rd.w]);
    }
    if (!ok) atomicOr(flags + 1, 1u);
}

template <typename B>
int grid_detect_t(alp_points *p, uint32_t *flags, RowDiv *out) {
    hipStream_t st = ctx().stream;
    const uint32_t n = (uint32_t)p->n;
    uint32_t h[2] = {GRID_NONE, 0};
    ALP_HIP(hipMemcpyAsync(flags, h, sizeof(h), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(grid_row_length_kernel<B>, dim3(stream_grid(n)), dim3(256), 0, st, (const B *)p->y, n, flags);
    ALP_HIP(hipGetLastError());
    ALP_HIP(hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, st));
    ALP_HIP(hipStreamSynchronize(st));
    if (h[0] == GRID_NONE || h[0] > GRID_MAX_ROW) return ALP_OK;     // a single row, or too wide
    const RowDiv rd = host::row_div(h[0]);
    hipLaunchKernelGGL(grid_verify_kernel<B>, dim3(stream_grid(n)), dim3(256), 0, st, (const B *)p->x, (const B *)p->y, n, rd, flags);
    ALP_HIP(hipGetLastError());
    ALP_HIP(hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, st));
    ALP_HIP(hipStreamSynchronize(st));
    if (h[1] == 0) *out = rd;
    return ALP_OK;
}

// p->rd = the grid of the uploaded planes, or w = 0 (the plane path)
int points_grid_detect(alp_points *p) {
    p->rd = RowDiv();
    if (getenv("ALP_NO_POINTS_GRID") || p->n < 2 || p->n_pad > ((int64_t)1 << 31)) return ALP_OK;
    uint32_t *flags = nullptr;
    if (int rc = scratch_reserve(2 * sizeof(uint32_t), (void **)&flags)) return rc;
    return p->precision == ALP_F64 ? grid_detect_t<uint64_t>(p, flags, &p->rd) : grid_detect_t<uint32_t>(p, flags, &p->rd);
}

template <typename T>
int launch_project(alp_points *p, const double params[ALP_NPARAM]) {
    PoseRec<T> pose;
    fold_pose_t<T>(params, p->origin, &pose);
    const int64_t nvec = (p->n + Num<T>::VEC - 1) / Num<T>::VEC;
    const unsigned grid = (unsigned)((nvec + 255) / 256);        // one 16-byte vector per lane
    if (p->rd.w)        // a grid: z alone streams in (points_grid_detect)
        hipLaunchKernelGGL((project_kernel<T>), dim3(grid), dim3(256), 0, ctx().stream, (const T *)p->x, (const T *)p->y,
                           (const T *)p->z, (T *)p->u, (T *)p->v, nvec, p->rd, (uint32_t)(p->n - 1), pose);
    else
        hipLaunchKernelGGL((project_kernel<T>), dim3(grid), dim3(256), 0, ctx().stream,
                           (const T *)p->x, (const T *)p->y, (const T *)p->z, (T *)p->u, (T *)p->v, nvec, pose);
    ALP_HIP(hipGetLastError());
    return ALP_OK;
}

int ensure_pop_scratch(alp_points *p, int64_t P, int nblk) {
    if (P > p->cand_cap) {
        const int64_t cap = round_up(P, 256);
        p->cand_cap = 0;
        reset_all(p->cand_dev, p->cand_host, p->sums_dev, p->sums_host);
        // two records per candidate: the general one and, behind all of those, the lens-free one (enqueue_popeval)
        const size_t recs = (size_t)cap * POSE_WORDS * p->esize() * 2, sums = (size_t)(cap + 1) * sizeof(double);
        if (int rc = reserve_all({recs, recs, sums, sums}, p->cand_dev, p->cand_host, p->sums_dev, p->sums_host)) return rc;
        p->cand_cap = cap;
    }
    const size_t need = (size_t)nblk * P * sizeof(double);
    return need ? p->partials.reserve(need) : ALP_OK;
}

// the four timing events of a handle, all or none: a partial failure must not leave ev[1] .. ev[3] NULL for good
int ensure_pop_events(alp_points *p) {
    if (p->ev[0]) return ALP_OK;
    Event ev[4];
    for (auto &e : ev)
        if (int rc = e.ensure()) return rc;
    for (int k = 0; k < 4; ++k) p->ev[k] = std::move(ev[k]);
    return ALP_OK;
}

// ------------------------------------------------------------------ float64 arithmetic on the stored points of a float32 set
// The counted pass, enqueue only: the first cnt->last of the records `recs` over the planes of `p` on the grid `g`, their partial
// rows (g.stripes x count doubles) added in fixed order into out[0 .. width), zeros behind the count; `slot`: out[width] = the
// set's count slot.  The count and the records lie on the device, in stream order, before this.
int counted_pass(alp_points *p, const PoseRec<double> *recs, const MendCount *cnt, const host::PopGrid &g, int loss_kind, double f_scale,
                 double *partials, double *out, int64_t width, bool slot) {
    static const decltype(&popeval_counted_kernel<ALP_LOSS_HUBER>) kernels[2][2] = {
        {popeval_counted_kernel<ALP_LOSS_MEAN_DIST>, popeval_counted_kernel<ALP_LOSS_HUBER>},
        {popeval_counted_kernel<ALP_LOSS_MEAN_DIST, true>, popeval_counted_kernel<ALP_LOSS_HUBER, true>}};
    hipLaunchKernelGGL(kernels[p->w != nullptr][loss_kind == ALP_LOSS_HUBER], dim3(g.stripes, g.tile_cols), dim3(256), 0, ctx().stream,
                       (const float *)p->x, (const float *)p->y, (const float *)p->z, (const float *)p->uo, (const float *)p->vo, p->n, recs, cnt,
                       f_scale, partials, (const float *)p->w);
    ALP_HIP(hipGetLastError());
    hipLaunchKernelGGL(reduce_counted_kernel, dim3((unsigned)((width + 31) / 32)), dim3(256), 0, ctx().stream, (const double *)partials,
                       g.stripes, (int)width, cnt, out, slot, p->count_slot());
    ALP_HIP(hipGetLastError());
    return ALP_OK;
}

// ------------------------------------------------------------------ the mend pass (alp_points_set_mend)
// One allocation for cap candidates: the compacted indices, the mended sums, the float64 records.
int *mend_idx(const alp_points *p) { return (int *)p->mend_dev; }
double *mend_sums(const alp_points *p) { return (double *)((char *)p->mend_dev + round_up(p->mend_cap * 4, 256)); }
PoseRec<double> *mend_recs(const alp_points *p) { return (PoseRec<double> *)(mend_sums(p) + p->mend_cap); }

int ensure_mend_scratch(alp_points *p) {
    if (!p->mend_cnt) {
        if (int rc = p->mend_cnt.reserve(sizeof(MendCount))) return rc;
        ALP_HIP(hipMemsetAsync(p->mend_cnt, 0, sizeof(MendCount), ctx().stream));
    }
    if (p->mend_cap >= p->cand_cap) return ALP_OK;
    p->mend_cap = 0;
    const int64_t cap = p->cand_cap;          // a multiple of 256
    if (int rc = p->mend_dev.reserve((size_t)round_up(cap * 4, 256) + (size_t)cap * (8 + sizeof(PoseRec<double>)))) return rc;
    p->mend_cap = cap;
    return ALP_OK;
}

// Behind the all-reduce of the float32 sums in p->sums_dev (identical on every rank, so every rank selects the same candidates):
// every candidate whose sum is not finite gets the sum float64 arithmetic gives on the stored points.  No host round trip: the
// count stays on the device.  `g` = host::mend_grid for (n, P); p->partials holds g.stripes x P doubles and is free again
// (reduce_partials_kernel has read it, in stream order).  No count slot: the records start right behind the mend_cap sums.
int mend_launch(alp_points *p, int64_t P, int loss_kind, double f_scale, const double *params_dev, const host::PopGrid &g) {
    hipStream_t st = ctx().stream;
    MendCount *cnt = (MendCount *)p->mend_cnt;
    hipLaunchKernelGGL(mend_select_kernel, dim3(1), dim3(256), 0, st, (const double *)p->sums_dev, (int)P, params_dev, p->origin[0],
                       p->origin[1], p->origin[2], mend_idx(p), mend_recs(p), cnt);
    ALP_HIP(hipGetLastError());
    if (int rc = counted_pass(p, mend_recs(p), cnt, g, loss_kind, f_scale, p->partials, mend_sums(p), P, false)) return rc;
    if (int rc = comm_allreduce_sum_f64(mend_sums(p), P)) return rc;
    hipLaunchKernelGGL(mend_scatter_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, (const int *)mend_idx(p),
                       (const double *)mend_sums(p), (const MendCount *)cnt, p->sums_dev);
    ALP_HIP(hipGetLastError());
    return ALP_OK;
}

// the launch half of enqueue_popeval (alp_points_internal.h: popeval_launch): the records lie in p->cand_dev
// The weighted shared-pose variant in float64 asks for two waves per SIMD instead of three: its unweighted form sits at the 168
// VGPRs of three waves already (the hoisted coordinates), and the weight's two registers per row spilled 44 bytes per lane to
// scratch under that cap.  Its V stays PopCfg's: unit weights must add in the unweighted kernel's order, bit for bit.
template <typename T> struct PopCfgWS : PopCfg<T> {};
template <> struct PopCfgWS<double> : PopCfgT<double, POP_VD, POP_TCD, 2> {};

template <typename T>
int popeval_launch_t(alp_points *p, int64_t P, int loss_kind, double f_scale, bool lens_free, bool shared_pose, bool batched = false,
                     const double *params_dev = nullptr) {
    using Kernel = void (*)(const T *, const T *, const T *, const T *, const T *, int64_t, const PoseRec<T> *, int, T,
                            double *, const PoseRec<T> *, const T *);
    const int which = (loss_kind == ALP_LOSS_HUBER ? 3 : 0) + (lens_free ? 2 : (shared_pose ? 1 : 0));
    // a set without weights takes row 0: the kernels it always took; a weighted set the same variant with WEIGHTED
    const Kernel kernels[2][6] = {{popeval_kernel<T, ALP_LOSS_MEAN_DIST, PopCfg<T>, false>,
                                   popeval_kernel<T, ALP_LOSS_MEAN_DIST, PopCfg<T>, true>,
                                   popeval_kernel<T, ALP_LOSS_MEAN_DIST, PopCfgLF<T>, false, T, true>,
                                   popeval_kernel<T, ALP_LOSS_HUBER, PopCfg<T>, false>,
                                   popeval_kernel<T, ALP_LOSS_HUBER, PopCfg<T>, true>,
                                   popeval_kernel<T, ALP_LOSS_HUBER, PopCfgLF<T>, false, T, true>},
                                  {popeval_kernel<T, ALP_LOSS_MEAN_DIST, PopCfg<T>, false, T, false, true>,
                                   popeval_kernel<T, ALP_LOSS_MEAN_DIST, PopCfgWS<T>, true, T, false, true>,
                                   popeval_kernel<T, ALP_LOSS_MEAN_DIST, PopCfgLF<T>, false, T, true, true>,
                                   popeval_kernel<T, ALP_LOSS_HUBER, PopCfg<T>, false, T, false, true>,
                                   popeval_kernel<T, ALP_LOSS_HUBER, PopCfgWS<T>, true, T, false, true>,
                                   popeval_kernel<T, ALP_LOSS_HUBER, PopCfgLF<T>, false, T, true, true>}};
    static_assert(PopCfg<T>::TC == PopCfgLF<T>::TC, "one candidate tile size per precision: host::pop_grid takes one TC");
    // the grid rule: host/alp_plan.h.  ALP_POP_GRID = "stripes,ytiles" (a development switch) overrides it where the pair is valid:
    // one that does not parse leaves a 0, which pop_grid ignores
    int ov[2] = {0, 0};
    if (const char *e = getenv("ALP_POP_GRID")) sscanf(e, "%d,%d", &ov[0], &ov[1]);
    const host::PopGrid g = host::pop_grid(p->n, P, sizeof(T) == 8, lens_free ? PopCfgLF<T>::V : PopCfg<T>::V, PopCfg<T>::TC,
                                           ctx().cu_count, batched, ov[0], ov[1]);
    // the mend pass (float32 sets that asked for it) takes its partial rows from the same buffer, after the first pass is done with it
    const bool mend = sizeof(T) == 4 && p->mend;
    host::PopGrid mg = {0, 0};
    if (mend) {
        if (!params_dev) return fail(ALP_EINVAL, "population evaluation with mend on: the candidates' parameter rows are missing");
        mg = host::mend_grid(p->n, P, PopCfg<double>::V, PopCfg<double>::TC, ctx().cu_count);
    }
    if (int rc = ensure_pop_scratch(p, P, g.stripes > mg.stripes ? g.stripes : mg.stripes)) return rc;
    if (int rc = ensure_pop_events(p)) return rc;
    if (mend)
        if (int rc = ensure_mend_scratch(p)) return rc;
    p->last_info[0] = lens_free ? ALP_POP_LENS_FREE : (shared_pose ? ALP_POP_SHARED_POSE : ALP_POP_GENERAL);
    p->last_info[1] = g.stripes;
    p->last_info[2] = g.tile_cols;
    ALP_HIP(hipEventRecord(p->ev[0], ctx().stream));
    const PoseRec<T> *recs_general = (const PoseRec<T> *)p->cand_dev;
    hipLaunchKernelGGL(kernels[p->w != nullptr][which], dim3(g.stripes, g.tile_cols), dim3(256), 0, ctx().stream, (const T *)p->x, (const T *)p->y,
                       (const T *)p->z, (const T *)p->uo, (const T *)p->vo, p->n, lens_free ? recs_general + p->cand_cap : recs_general,
                       (int)P, (T)f_scale, p->partials, recs_general, (const T *)p->w);
    ALP_HIP(hipGetLastError());
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)((P + 31) / 32)), dim3(256), 0, ctx().stream,
                       p->partials, g.stripes, (int)P, p->count_slot(), p->sums_dev);
    ALP_HIP(hipGetLastError());
    ALP_HIP(hipEventRecord(p->ev[1], ctx().stream));
    if (int rc = comm_allreduce_sum_f64(p->sums_dev, P + 1)) return rc;
    ALP_HIP(hipEventRecord(p->ev[2], ctx().stream));
    p->mend_ran = mend;
    p->mend_info[0] = mg.stripes;
    p->mend_info[1] = mg.tile_cols;
    if (mend) {
        if (int rc = mend_launch(p, P, loss_kind, f_scale, params_dev, mg)) return rc;
        ALP_HIP(hipEventRecord(p->ev[3], ctx().stream));
    }
    p->timed = true;
    return ALP_OK;
}

template <typename T>
int enqueue_popeval(alp_points *p, const double *cand, int64_t P, int loss_kind, double f_scale) {
    // one pinned staging buffer per handle: a second enqueue would rewrite it under the first one's
    // asynchronous copy (and lose its result)
    if (p->pending_P > 0)
        return fail(ALP_ESTATE, "alp_eval_population_enqueue: the previous enqueue has not been waited for");
    if (p->loop_pending)
        return fail(ALP_ESTATE, "alp_eval_population_enqueue: a device loop on this point set has not been waited for (alp_cma_wait)");
    if (int rc = ensure_pop_scratch(p, P, 0)) return rc;
    PoseRec<T> *h = (PoseRec<T> *)p->cand_host;
    // the kernel centres the observations once per point: every candidate of a call must share
    // the image size (the reference never optimises w, h: optimize.py:240-247)
    for (int64_t i = 1; i < P; ++i)
        if (cand[i * ALP_NPARAM + 21] != cand[21] || cand[i * ALP_NPARAM + 22] != cand[22])
            return fail(ALP_EINVAL, "alp_eval_population: candidates %lld and 0 differ in w or h", (long long)i);
    // lens-free populations (no candidate has a lens coefficient other than a1, a2: the reference's first phase, example.py:51-54;
    // BASELINE config 3) take the kernel variant that runs on rows with the lens folded in: its records follow the general ones
    bool lens_free = !getenv("ALP_POP_NO_LENS_FREE");
    for (int64_t i = 0; i < P && lens_free; ++i) lens_free = pose_is_lens_free(cand + i * ALP_NPARAM);
    for (int64_t i = 0; i < P; ++i) {
        double g[POSE_WORDS], lf[POSE_WORDS];
        fold_pose(cand + i * ALP_NPARAM, p->origin, g);
        for (int k = 0; k < POSE_WORDS; ++k) h[i].v[k] = (T)g[k];
        if (lens_free) {
            lens_free_from_general(g, lf);
            for (int k = 0; k < POSE_WORDS; ++k) h[p->cand_cap + i].v[k] = (T)lf[k];
        }
    }
    ALP_HIP(hipMemcpyAsync(p->cand_dev, h, (size_t)P * sizeof(PoseRec<T>), hipMemcpyHostToDevice, ctx().stream));
    if (lens_free)
        ALP_HIP(hipMemcpyAsync((PoseRec<T> *)p->cand_dev + p->cand_cap, h + p->cand_cap, (size_t)P * sizeof(PoseRec<T>), hipMemcpyHostToDevice,
                               ctx().stream));
    // distortion-only populations (the reference's second phase, example.py:75-78) share the
    // folded 3x4 matrix: its 12 words are identical in every record, and the kernel then
    // computes the normalised coordinates once per point instead of once per candidate
    bool shared_pose = P > 1 && !lens_free;
    for (int64_t i = 1; i < P && shared_pose; ++i)
        shared_pose = memcmp(h[i].v, h[0].v, 12 * sizeof(T)) == 0;
    // (float32 sets keep the call's parameter vectors: the argmin confirmation folds them again in float64, and so does the
    // mend pass, on the device, from a copy uploaded beside the records)
    if (sizeof(T) == 4) p->cand_copy.assign(cand, cand + P * ALP_NPARAM);
    const double *params_dev = nullptr;
    if (sizeof(T) == 4 && p->mend) {
        if (p->mend_params.capacity() < (size_t)P * ALP_NPARAM * sizeof(double))
            if (int rc = p->mend_params.reserve((size_t)p->cand_cap * ALP_NPARAM * sizeof(double))) return rc;
        ALP_HIP(hipMemcpyAsync(p->mend_params, p->cand_copy.data(), (size_t)P * ALP_NPARAM * sizeof(double), hipMemcpyHostToDevice,
                               ctx().stream));
        params_dev = p->mend_params;
    }
    if (int rc = popeval_launch_t<T>(p, P, loss_kind, f_scale, lens_free, shared_pose, false, params_dev)) return rc;
    ALP_HIP(hipMemcpyAsync(p->sums_host, p->sums_dev, (size_t)(P + 1) * sizeof(double),
                           hipMemcpyDeviceToHost, ctx().stream));
    p->pending_P = P;
    p->pending_loss = loss_kind;
    p->pending_f_scale = f_scale;
    return ALP_OK;
}

// float64 re-evaluation of K <= CONFIRM_MAX candidates of a float32 point set (same stored
// coordinates, double arithmetic, same fixed-order reduction and the same all-reduce): the counted pass with a count the host
// knows.  sums_out[0..K) = loss sums, sums_out[K] = vertex count (the sum of the weights on a weighted set).  Synchronous.
int confirm_losses(alp_points *p, const double *cand, const int64_t *which, int K, int loss_kind, double f_scale, double *sums_out) {
    const host::PopGrid g = {host::confirm_grid(p->n, ctx().cu_count), 1};
    // the count word {K, 0} and, 256 bytes behind it, the K records: one copy, which the stream runs before the kernels
    struct Upload { MendCount cnt; char pad[256 - sizeof(MendCount)]; PoseRec<double> recs[CONFIRM_MAX]; } up = {};
    if (int rc = p->conf_dev.reserve(sizeof(Upload) + (size_t)(g.stripes + 2) * CONFIRM_MAX * sizeof(double))) return rc;
    if (int rc = p->conf_host.reserve((CONFIRM_MAX + 1) * sizeof(double))) return rc;
    up.cnt.last = K;
    for (int k = 0; k < K; ++k) fold_pose_t<double>(cand + which[k] * ALP_NPARAM, p->origin, &up.recs[k]);
    const Upload *up_dev = (const Upload *)p->conf_dev;
    double *partials = (double *)(up_dev + 1);
    double *sums_dev = partials + (size_t)g.stripes * CONFIRM_MAX;
    ALP_HIP(hipMemcpyAsync(p->conf_dev, &up, (const char *)&up.recs[K] - (const char *)&up, hipMemcpyHostToDevice, ctx().stream));
    if (int rc = counted_pass(p, up_dev->recs, &up_dev->cnt, g, loss_kind, f_scale, partials, sums_dev, K, true)) return rc;
    if (int rc = comm_allreduce_sum_f64(sums_dev, K + 1)) return rc;
    ALP_HIP(hipMemcpyAsync(p->conf_host, sums_dev, (size_t)(K + 1) * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    ALP_HIP(hipStreamSynchronize(ctx().stream));      // `up` (stack) must outlive the H2D copy too
    memcpy(sums_out, p->conf_host, (size_t)(K + 1) * sizeof(double));
    return ALP_OK;
}

// The chunk loop of alp_residuals* and alp_jacobian: launch(offset, count) fills the staging buffer with the output of `count`
// points (host::stage_chunk_points of them: at most RES_CHUNK_BYTES per launch), copy(offset, count) sends it to the host.
template <typename Launch, typename Copy>
int staged_chunks(int64_t n, int64_t chunk, Launch launch, Copy copy) {
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t cnt = n - off < chunk ? n - off : chunk;
        ktime_begin();
        launch(off, cnt);
        ktime_end();
        ALP_HIP(hipGetLastError());
        ALP_HIP(copy(off, cnt));
        ALP_HIP(hipStreamSynchronize(ctx().stream));       // the staging buffer is reused; the records / the plan must outlive their copy
    }
    return ALP_OK;
}

template <typename T>
int residuals_impl(alp_points *p, const double *cand, int64_t B, double *out) {
    // B pose records (kernel argument for B == 1 would save the copy; one path keeps it simple)
    const size_t rec_bytes = round_up((int64_t)(B * sizeof(PoseRec<T>)), 256);
    const int64_t chunk = host::stage_chunk_points(p->n, B);
    char *dev = nullptr;
    if (int rc = scratch_reserve(rec_bytes + (size_t)B * chunk * sizeof(double2), (void **)&dev)) return rc;
    PoseRec<T> *poses_dev = (PoseRec<T> *)dev;
    double2 *res_dev = (double2 *)(dev + rec_bytes);
    std::vector<PoseRec<T>> poses((size_t)B);
    for (int64_t b = 0; b < B; ++b) fold_pose_t<T>(cand + b * ALP_NPARAM, p->origin, &poses[b]);
    hipStream_t st = ctx().stream;
    ALP_HIP(hipMemcpyAsync(poses_dev, poses.data(), (size_t)B * sizeof(PoseRec<T>), hipMemcpyHostToDevice, st));
    return staged_chunks(p->n, chunk, [&](int64_t off, int64_t cnt) {
        hipLaunchKernelGGL(residual_batch_kernel<T>, dim3(stream_grid(cnt)), dim3(256), 0, st, (const T *)p->x + off,
                           (const T *)p->y + off, (const T *)p->z + off, (const T *)p->uo + off, (const T *)p->vo + off,
                           res_dev, cnt, poses_dev, (int)B);
    }, [&](int64_t off, int64_t cnt) {
        // row b of the chunk -> out[b][off .. off + cnt); a chunk that holds whole rows is one contiguous run (a pitched copy of
        // the same bytes took 2-3 x as long)
        if (cnt == p->n) return hipMemcpyAsync(out, res_dev, (size_t)B * cnt * sizeof(double2), hipMemcpyDeviceToHost, st);
        return hipMemcpy2DAsync(out + 2 * off, (size_t)p->n * sizeof(double2), res_dev, (size_t)cnt * sizeof(double2),
                                (size_t)cnt * sizeof(double2), (size_t)B, hipMemcpyDeviceToHost, st);
    });
}

// alp_residuals_assigned: float64 records of the B poses, then per chunk of points the assignments in and the pairs out
template <typename TS>
int residuals_assigned_impl(alp_points *p, const double *cand, int64_t B, const int32_t *assign, double *out) {
    const size_t rec_bytes = round_up((int64_t)(B * sizeof(PoseRec<double>)), 256);
    const int64_t chunk = host::stage_chunk_points(p->n, 1);
    const size_t idx_bytes = round_up(chunk * 4, 256);
    char *dev = nullptr;
    if (int rc = scratch_reserve(rec_bytes + idx_bytes + (size_t)chunk * sizeof(double2), (void **)&dev)) return rc;
    PoseRec<double> *poses_dev = (PoseRec<double> *)dev;
    int *assign_dev = (int *)(dev + rec_bytes);
    double2 *res_dev = (double2 *)(dev + rec_bytes + idx_bytes);
    std::vector<PoseRec<double>> poses((size_t)B);
    for (int64_t b = 0; b < B; ++b) fold_pose_t<double>(cand + b * ALP_NPARAM, p->origin, &poses[b]);
    hipStream_t st = ctx().stream;
    ALP_HIP(hipMemcpyAsync(poses_dev, poses.data(), (size_t)B * sizeof(PoseRec<double>), hipMemcpyHostToDevice, st));
    using Kernel = void (*)(const TS *, const TS *, const TS *, const TS *, const TS *, const int *, double2 *, int64_t, const PoseRec<double> *, int);
    const Kernel kernel = B <= RA_LDS_POSES ? residuals_assigned_kernel<TS, true> : residuals_assigned_kernel<TS, false>;
    return staged_chunks(p->n, chunk, [&](int64_t off, int64_t cnt) {
        if (hipMemcpyAsync(assign_dev, assign + off, (size_t)cnt * 4, hipMemcpyHostToDevice, st) != hipSuccess) return;      // (hipGetLastError reports it)
        hipLaunchKernelGGL(kernel, dim3(stream_grid(cnt)), dim3(256), 0, st, (const TS *)p->x + off, (const TS *)p->y + off, (const TS *)p->z + off, (const TS *)p->uo + off,
                           (const TS *)p->vo + off, (const int *)assign_dev, res_dev, cnt, (const PoseRec<double> *)poses_dev, (int)B);
    }, [&](int64_t off, int64_t cnt) {
        return hipMemcpyAsync(out + 2 * off, res_dev, (size_t)cnt * sizeof(double2), hipMemcpyDeviceToHost, st);
    });
}

// alp_jacobian: chunks of whole points (a chunk's rows are one contiguous block of the output: one copy each)
template <typename TS>
int jacobian_impl(alp_points *p, const JacPlan &plan, double *out) {
    const int64_t D = plan.D;
    const size_t plan_bytes = round_up((int64_t)sizeof(JacPlan), 256);
    const int64_t chunk = host::stage_chunk_points(p->n, D);
    char *dev = nullptr;
    if (int rc = scratch_reserve(plan_bytes + (size_t)chunk * D * sizeof(double2), (void **)&dev)) return rc;
    JacPlan *plan_dev = (JacPlan *)dev;
    double2 *jac_dev = (double2 *)(dev + plan_bytes);
    hipStream_t st = ctx().stream;
    ALP_HIP(hipMemcpyAsync(plan_dev, &plan, sizeof(JacPlan), hipMemcpyHostToDevice, st));
    return staged_chunks(p->n, chunk, [&](int64_t off, int64_t cnt) {
        hipLaunchKernelGGL(jacobian_kernel<TS>, dim3(stream_grid(cnt)), dim3(256), 0, st, (const TS *)p->x + off,
                           (const TS *)p->y + off, (const TS *)p->z + off, jac_dev, cnt, (const JacPlan *)plan_dev);
    }, [&](int64_t off, int64_t cnt) {
        return hipMemcpyAsync(out + 2 * D * off, jac_dev, (size_t)cnt * D * sizeof(double2), hipMemcpyDeviceToHost, st);
    });
}

// The kernel of the multi-pose K3n for a loss and a weighted / unweighted launch
template <typename TS>
using NormalPosesKernel = void (*)(const TS *, const TS *, const TS *, const TS *, const TS *, int64_t, int64_t, double, const JacPlan *,
                                   const int *, const long long *, int, double *, const TS *, int64_t, const int *);
template <typename TS>
NormalPosesKernel<TS> normal_poses_kernel_for(int loss, bool weighted) {
    static const NormalPosesKernel<TS> kernels[2][4] = {
        {normal_poses_kernel<TS, ALP_NORMAL_LINEAR>, normal_poses_kernel<TS, ALP_NORMAL_SOFT_L1>,
         normal_poses_kernel<TS, ALP_NORMAL_HUBER>, normal_poses_kernel<TS, ALP_NORMAL_CAUCHY>},
        {normal_poses_kernel<TS, ALP_NORMAL_LINEAR, true>, normal_poses_kernel<TS, ALP_NORMAL_SOFT_L1, true>,
         normal_poses_kernel<TS, ALP_NORMAL_HUBER, true>, normal_poses_kernel<TS, ALP_NORMAL_CAUCHY, true>}};
    return kernels[weighted][loss];
}

// What varies between the launches of the multi-pose K3n (device pointers; alp_point_kernels.h: normal_poses_kernel):
struct NormalPosesLaunch {
    const int *list = nullptr;           // the device loop: the running starts, their count and a flag per start
    const long long *count = nullptr;
    const int *running = nullptr;
    int pose_in_x = NORMAL_BATCH_POSE_IN_X;
    bool table = false;                  // the poses run under rows of the set's weight table, not under its weight plane
    const int *row_of_pose = nullptr;    // with `table`: the row of each pose; NULL: pose k under row k
    bool timed = false;                  // the two launches are a kernel section (alp_kernel_timing)
};

// normal_poses_kernel over the stripes of `g` x the K poses under plans[], reduce_normal_poses_kernel over each pose's rows (or
// zeros for an empty shard, which still joins the all-reduce: a row of no weights sums to 0), one all-reduce of the K x (T + 1)
// sums.  Enqueue only.  partials: K * g.blocks * T doubles.
template <typename TS>
int normal_poses_enqueue(alp_points *p, const JacPlan *plans, int K, int D, const host::NormalGrid &g, int loss, double f_scale,
                         const NormalPosesLaunch &l, double *partials, double *sums) {
    const int T = D * (D + 1) / 2 + D + 1;
    hipStream_t st = ctx().stream;
    if (g.blocks > 0) {
        const TS *wts = (const TS *)(l.table ? p->wt : p->w);
        const dim3 grid = l.pose_in_x ? dim3((unsigned)K, (unsigned)g.blocks) : dim3((unsigned)g.blocks, (unsigned)K);
        if (l.timed) ktime_begin();
        hipLaunchKernelGGL(normal_poses_kernel_for<TS>(loss, wts != nullptr), grid, dim3(256), 0, st, (const TS *)p->x, (const TS *)p->y,
                           (const TS *)p->z, (const TS *)p->uo, (const TS *)p->vo, p->n, g.groups_per, 1.0 / f_scale, plans, l.list, l.count,
                           l.pose_in_x, partials, wts, l.table ? p->n : (int64_t)0, l.row_of_pose);
        hipLaunchKernelGGL(reduce_normal_poses_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)K), dim3(256), 0, st, (const double *)partials,
                           g.blocks, T, p->count_slot(), l.table ? (const double *)p->wt_sums : nullptr, l.row_of_pose, l.running, sums);
        if (l.timed) ktime_end();
        ALP_HIP(hipGetLastError());
    } else {
        ALP_HIP(hipMemsetAsync(sums, 0, (size_t)K * (T + 1) * sizeof(double), st));
    }
    return comm_allreduce_sum_f64(sums, (int64_t)K * (T + 1));
}

// alp_normal_equations (B = 1), alp_normal_equations_batch (both: row_of_pose NULL) and alp_normal_equations_batch_rows: the
// scratch holds the B plans, on the row path the B row indices, the partial rows and the sums; one copy of the B x (T + 1) sums
// comes back.
// ALP_NORMAL_BATCH_ORDER = "stripe" | "pose" (a development switch, tools/probe_normal_batch.py) names the grid index that runs
// fastest; the sums do not depend on it, and with one pose the two orders launch the same stripes in the same order.
template <typename TS>
int normal_batch_impl(alp_points *p, const std::vector<JacPlan> &plans, int loss, double f_scale, double *out, const int32_t *row_of_pose) {
    const int64_t B = (int64_t)plans.size();
    const int D = plans[0].D, T = D * (D + 1) / 2 + D + 1;
    const host::NormalGrid g = host::normal_batch_grid(p->n, B, ctx().cu_count);
    const size_t plans_bytes = round_up((int64_t)(B * sizeof(JacPlan)), 256), rows_bytes = row_of_pose ? round_up(B * 4, 256) : 0;
    char *dev = nullptr;
    if (int rc = scratch_reserve(plans_bytes + rows_bytes + ((size_t)B * g.blocks * T + (size_t)B * (T + 1)) * sizeof(double), (void **)&dev)) return rc;
    JacPlan *plans_dev = (JacPlan *)dev;
    int *rows_dev = (int *)(dev + plans_bytes);
    double *partials = (double *)(dev + plans_bytes + rows_bytes), *sums = partials + (size_t)B * g.blocks * T;
    hipStream_t st = ctx().stream;
    NormalPosesLaunch l;
    l.timed = true;
    if (g.blocks > 0) {
        const char *order = getenv("ALP_NORMAL_BATCH_ORDER");
        if (order) l.pose_in_x = !strcmp(order, "pose");
        ALP_HIP(hipMemcpyAsync(plans_dev, plans.data(), (size_t)B * sizeof(JacPlan), hipMemcpyHostToDevice, st));
        if (row_of_pose) {
            ALP_HIP(hipMemcpyAsync(rows_dev, row_of_pose, (size_t)B * 4, hipMemcpyHostToDevice, st));
            l.table = true;
            l.row_of_pose = rows_dev;
        }
    }
    if (int rc = normal_poses_enqueue<TS>(p, plans_dev, (int)B, D, g, loss, f_scale, l, partials, sums)) return rc;
    ALP_HIP(hipMemcpyAsync(out, sums, (size_t)B * (T + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    ALP_HIP(hipStreamSynchronize(st));           // the plans must outlive their copy too
    return ALP_OK;
}

}  // namespace

namespace alp {
// The evaluation of a round of the least-squares device loop (alp_lm.hip), over the grid of all K starts; the buffers are the loop's own.
int normal_listed_launch(alp_points *p, const JacPlan *plans, const int *list, const long long *count, const int *running, int K, int D,
                         const host::NormalGrid &g, int loss, double f_scale, double *partials, double *sums, bool weight_rows) {
    NormalPosesLaunch l;
    l.list = list, l.count = count, l.running = running, l.pose_in_x = 1, l.table = weight_rows;
    return p->precision == ALP_F64 ? normal_poses_enqueue<double>(p, plans, K, D, g, loss, f_scale, l, partials, sums)
                                   : normal_poses_enqueue<float>(p, plans, K, D, g, loss, f_scale, l, partials, sums);
}
int popeval_launch(alp_points *p, int64_t P, int loss_kind, double f_scale, bool lens_free, bool shared_pose, bool batched,
                   const double *params_dev) {
    return p->precision == ALP_F64 ? popeval_launch_t<double>(p, P, loss_kind, f_scale, lens_free, shared_pose, batched, params_dev)
                                   : popeval_launch_t<float>(p, P, loss_kind, f_scale, lens_free, shared_pose, batched, params_dev);
}
int points_pop_reserve(alp_points *p, int64_t P) { return ensure_pop_scratch(p, P, 0); }
}  // namespace alp

// ---- fetch with a change of element type (float32 set -> float64 arrays, the reference's type; or the reverse)
// The planes are converted ON THE HOST while they arrive: a chunk crosses PCIe in its stored type (a float32 set moves 4 bytes
// per value, not 8) into one of two pinned staging buffers, and host threads widen / narrow the previous chunk into the
// caller's array meanwhile -- the copy engine and the host cores overlap, nothing of the size of the result is allocated.
// The reverse (a float64 set fetched as float32) is cast on the device into the scratch area first, so that again the narrow
// type crosses PCIe.  ALP_FETCH_CONVERT=host|device forces either way (tests, tools/probe_fetch.py).
namespace {
constexpr int64_t FETCH_CHUNK = (int64_t)8 << 20;         // values per chunk: 32 MB of float32, 64 MB of float64
void *g_fetch_stage[2] = {nullptr, nullptr};               // pinned, FETCH_CHUNK * 8 bytes each; lives until the process ends
hipEvent_t g_fetch_ev[2] = {nullptr, nullptr};

using alp::host::convert_threads;      // the widening / narrowing workers: host/alp_host.h (HIP-free, run under the sanitizers)
using alp::host::fetch_threads;

template <typename S, typename D>
__global__ __launch_bounds__(256) void cast_plane_kernel(const S *__restrict__ src, D *__restrict__ dst, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = (D)src[i];
}

template <typename S, typename D>
int fetch_converted_t(alp_points *p, D *u_out, D *v_out) {
    hipStream_t st = ctx().stream;
    const S *planes[2] = {(const S *)p->u, (const S *)p->v};
    D *outs[2] = {u_out, v_out};
    // the NARROWER type crosses PCIe: widening happens on the host (measured, 100 M points: 17 ms against 30 ms through the device
    // cast and 14 ms for the plain float32 fetch), narrowing on the device (15 ms against 33 ms; the plain float64 fetch: 28 ms)
    const char *mode = getenv("ALP_FETCH_CONVERT");
    const bool on_device = mode ? !strcmp(mode, "device") : sizeof(D) < sizeof(S);
    if (on_device) {
        D *tmp = nullptr;
        if (int rc = scratch_reserve((size_t)FETCH_CHUNK * sizeof(D), (void **)&tmp)) return rc;
        for (int pl = 0; pl < 2; ++pl)
            for (int64_t off = 0; off < p->n; off += FETCH_CHUNK) {
                const int64_t cnt = std::min(FETCH_CHUNK, p->n - off);
                hipLaunchKernelGGL((cast_plane_kernel<S, D>), dim3(stream_grid(cnt)), dim3(256), 0, st, planes[pl] + off, tmp, (long long)cnt);
                ALP_HIP(hipMemcpyAsync(outs[pl] + off, tmp, (size_t)cnt * sizeof(D), hipMemcpyDeviceToHost, st));   // in stream order: the next cast waits
            }
        ALP_HIP(hipStreamSynchronize(st));
        return ALP_OK;
    }
    for (auto &b : g_fetch_stage)
        if (!b) ALP_HIP(hipHostMalloc(&b, (size_t)FETCH_CHUNK * 8, hipHostMallocDefault));
    const int T = fetch_threads();
    for (auto &e : g_fetch_ev)
        if (!e) ALP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hipEvent_t *ev = g_fetch_ev;
    struct Job { int pl; int64_t off, cnt; };
    std::vector<Job> jobs;
    for (int pl = 0; pl < 2; ++pl)
        for (int64_t off = 0; off < p->n; off += FETCH_CHUNK) jobs.push_back({pl, off, std::min(FETCH_CHUNK, p->n - off)});
    for (size_t k = 0; k <= jobs.size(); ++k) {
        if (k < jobs.size()) {       // chunk k is on its way into stage[k & 1] (chunk k - 2, its last user, was converted in round k - 1)
            const Job &j = jobs[k];
            ALP_HIP(hipMemcpyAsync(g_fetch_stage[k & 1], planes[j.pl] + j.off, (size_t)j.cnt * sizeof(S), hipMemcpyDeviceToHost, st));
            ALP_HIP(hipEventRecord(ev[k & 1], st));
        }
        if (k > 0) {                 // ... while the host cores convert chunk k - 1
            const Job &j = jobs[k - 1];
            ALP_HIP(hipEventSynchronize(ev[(k - 1) & 1]));
            convert_threads((const S *)g_fetch_stage[(k - 1) & 1], outs[j.pl] + j.off, j.cnt, T);
        }
    }
    return ALP_OK;
}

}  // namespace
namespace alp {
void points_release_staging() {
    for (auto &b : g_fetch_stage) {
        if (b) hipHostFree(b);
        b = nullptr;
    }
    for (auto &e : g_fetch_ev) {
        if (e) hipEventDestroy(e);
        e = nullptr;
    }
}
}  // namespace alp
namespace {
int fetch_converted(alp_points *p, void *u_out, void *v_out, int out_dtype) {
    return out_dtype == ALP_F64 ? fetch_converted_t<float, double>(p, (double *)u_out, (double *)v_out)
                                : fetch_converted_t<double, float>(p, (float *)u_out, (float *)v_out);
}
}  // namespace

namespace {
// the n weights as the set stores them (rounded to T), validated; *sum = their float64 sum in index order
template <typename TIn, typename T>
int weights_stored(const void *w, int64_t n, std::vector<T> &out, double *sum) {
    const TIn *src = (const TIn *)w;
    out.resize((size_t)n);
    double s = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double v = (double)src[i];
        if (!(v >= 0.0) || !std::isfinite(v))
            return fail(ALP_EINVAL, "alp_points_set_weights: weight %lld is negative, NaN or infinite", (long long)i);
        const T t = (T)v;
        if (!std::isfinite((double)t)) return fail(ALP_EINVAL, "alp_points_set_weights: weight %lld does not fit the set's element type", (long long)i);
        out[(size_t)i] = t;
        s += (double)t;
    }
    *sum = s;
    return ALP_OK;
}

template <typename T>
int set_weights_t(alp_points *p, const void *w, int in_dtype) {
    std::vector<T> stored;
    double sum = 0;
    if (int rc = in_dtype == ALP_F64 ? weights_stored<double, T>(w, p->n, stored, &sum) : weights_stored<float, T>(w, p->n, stored, &sum)) return rc;
    // (nothing of the set has changed so far: a refused call leaves the previous weights in force)
    if (!p->w) {
        DeviceBuffer<> plane;
        if (int rc = plane.reserve((size_t)p->n_pad * sizeof(T))) return rc;
        hipError_t e = hipMemsetAsync(plane, 0, (size_t)p->n_pad * sizeof(T), ctx().stream);
        if (e != hipSuccess) return fail(ALP_EHIP, "alp_points_set_weights: %s", hipGetErrorString(e));
        p->w = std::move(plane);
        p->w_sum = 0;           // until the copy below is through, the plane is all zeros
    }
    if (p->n > 0) ALP_HIP(hipMemcpyAsync(p->w, stored.data(), (size_t)p->n * sizeof(T), hipMemcpyHostToDevice, ctx().stream));
    ALP_HIP(hipStreamSynchronize(ctx().stream));      // `stored` must outlive its copy
    p->w_sum = sum;
    return ALP_OK;
}

// alp_points_set_weight_table: validate everything (nothing of the set has changed until then), build the new table beside
// the old one -- the rows rounded to T in chunks of at most WT_STAGE values on the host, the row sums by
// weight_table_sums_kernel -- and only then let it take the old one's place.
constexpr int64_t WT_STAGE = (int64_t)8 << 20;

template <typename T>
int weight_table_sums_launch(const T *table, int64_t n, int R, double *sums) {
    hipStream_t st = ctx().stream;
    if (n == 0) {
        ALP_HIP(hipMemsetAsync(sums, 0, (size_t)R * sizeof(double), st));
        return ALP_OK;
    }
    const int64_t C = (n + WT_SUM_CHUNK - 1) / WT_SUM_CHUNK;
    double *partials = sums;
    if (C > 1)
        if (int rc = scratch_reserve((size_t)R * C * sizeof(double), (void **)&partials)) return rc;
    hipLaunchKernelGGL(weight_table_sums_kernel<T>, dim3((unsigned)C, (unsigned)R), dim3(256), 0, st, table, n, n, WT_SUM_CHUNK, partials);
    if (C > 1)
        hipLaunchKernelGGL(weight_table_sums_kernel<double>, dim3(1, (unsigned)R), dim3(256), 0, st, (const double *)partials, C, C, C, sums);
    ALP_HIP(hipGetLastError());
    return ALP_OK;
}

template <typename TIn, typename T>
int set_weight_table_t(alp_points *p, const void *w, int R) {
    const TIn *src = (const TIn *)w;
    const int64_t n = p->n, total = (int64_t)R * n;
    for (int64_t i = 0; i < total; ++i) {
        const double v = (double)src[i];
        if (!(v >= 0.0) || !std::isfinite(v))
            return fail(ALP_EINVAL, "alp_points_set_weight_table: weight %lld of row %lld is negative, NaN or infinite", (long long)(i % n),
                        (long long)(i / n));
        if (!std::isfinite((double)(T)v))
            return fail(ALP_EINVAL, "alp_points_set_weight_table: weight %lld of row %lld does not fit the set's element type", (long long)(i % n),
                        (long long)(i / n));
    }
    const size_t table_bytes = (size_t)round_up((total > 0 ? total : 1) * (int64_t)sizeof(T), 256);
    DeviceBuffer<> fresh;
    if (int rc = fresh.reserve(table_bytes + (size_t)R * sizeof(double))) return rc;
    T *table = (T *)fresh;
    double *sums = (double *)((char *)table + table_bytes);
    hipStream_t st = ctx().stream;
    std::vector<T> stage((size_t)(total < WT_STAGE ? total : WT_STAGE));
    for (int64_t off = 0; off < total; off += WT_STAGE) {
        const int64_t cnt = total - off < WT_STAGE ? total - off : WT_STAGE;
        for (int64_t i = 0; i < cnt; ++i) stage[(size_t)i] = (T)(double)src[off + i];
        ALP_HIP(hipMemcpyAsync(table + off, stage.data(), (size_t)cnt * sizeof(T), hipMemcpyHostToDevice, st));
        ALP_HIP(hipStreamSynchronize(st));      // `stage` is rewritten by the next chunk
    }
    if (int rc = weight_table_sums_launch<T>(table, n, R, sums)) return rc;
    ALP_HIP(hipStreamSynchronize(st));          // nothing enqueued reads the old table any more either
    p->wt = std::move(fresh);
    p->wt_rows = R;
    p->wt_sums = sums;
    return ALP_OK;
}

}  // namespace

extern "C" {

// xyz: n x 3 row-major (cols == NULL), or cols[0..2]: the three columns as they lie
static int points_create(const void *xyz, const void *const *cols, int in_dtype, int64_t n, const double origin[3], int precision,
                         alp_points_t **out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(out, "out is NULL");
    *out = nullptr;
    ALP_REQUIRE(n >= 0, "n is negative");
    ALP_REQUIRE(n == 0 || xyz || (cols && cols[0] && cols[1] && cols[2]), "coordinates are NULL");
    ALP_REQUIRE(origin, "origin is NULL");
    ALP_REQUIRE(precision == ALP_F32 || precision == ALP_F64, "precision must be ALP_F32 or ALP_F64");
    ALP_REQUIRE(in_dtype == ALP_F32 || in_dtype == ALP_F64, "in_dtype must be ALP_F32 or ALP_F64");
    alp_points *p = new alp_points();
    p->n = n;
    p->n_pad = round_up(n > 0 ? n : 1, 1024);
    p->precision = precision;
    memcpy(p->origin, origin, sizeof(p->origin));
    void **xyz_planes[3] = {&p->x, &p->y, &p->z};
    int rc = alloc_planes(p->slab_xyz, 3, p->n_pad, p->esize(), xyz_planes);
    if (!rc && n > 0) {
        void *const planes[3] = {p->x, p->y, p->z};
        rc = upload<3>(xyz, cols, in_dtype, n, origin, precision, planes);
    }
    if (!rc) {
        hipError_t e = hipStreamSynchronize(ctx().stream);
        if (e != hipSuccess) rc = fail(ALP_EHIP, "points upload: %s", hipGetErrorString(e));
    }
    if (!rc) rc = points_grid_detect(p);
    if (rc) {
        alp_points_destroy(p);
        return rc;
    }
    *out = p;
    return ALP_OK;
}

int alp_points_create(const void *xyz, int in_dtype, int64_t n, const double origin[3], int precision,
                      alp_points_t **out) {
    return points_create(xyz, nullptr, in_dtype, n, origin, precision, out);
}

int alp_points_create_columns(const void *x, const void *y, const void *z, int in_dtype, int64_t n, const double origin[3],
                              int precision, alp_points_t **out) {
    const void *const cols[3] = {x, y, z};
    return points_create(nullptr, cols, in_dtype, n, origin, precision, out);
}

int alp_points_destroy(alp_points_t *p) {
    if (!p) return ALP_OK;
    for (alp_cma_t *h : p->loops) cma_points_gone(h);
    for (alp_lm_t *h : p->lm_loops) lm_points_gone(h);
    if (ctx().ready) hipStreamSynchronize(ctx().stream);
    delete p;
    return ALP_OK;
}

int alp_points_count(const alp_points_t *p, int64_t *n) {
    ALP_REQUIRE(p && n, "NULL argument");
    *n = p->n;
    return ALP_OK;
}

int alp_points_layout(const alp_points_t *p, int64_t *row_length) {
    ALP_REQUIRE(p && row_length, "NULL argument");
    *row_length = p->rd.w;
    return ALP_OK;
}

// uv: n x 2 row-major (cols == NULL), or cols[0..1]: the u and v columns as they lie
static int set_observed(alp_points_t *p, const void *uv, const void *const *cols, int in_dtype) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p, "points handle is NULL");
    ALP_REQUIRE(p->n == 0 || uv || (cols && cols[0] && cols[1]), "observed pixels are NULL");
    ALP_REQUIRE(in_dtype == ALP_F32 || in_dtype == ALP_F64, "in_dtype must be ALP_F32 or ALP_F64");
    if (!p->uo) {
        void **obs_planes[2] = {&p->uo, &p->vo};
        if (int rc = alloc_planes(p->slab_obs, 2, p->n_pad, p->esize(), obs_planes)) return rc;
    }
    const double zero[3] = {0, 0, 0};
    void *const planes[3] = {p->uo, p->vo, nullptr};
    if (p->n > 0)
        if (int rc = upload<2>(uv, cols, in_dtype, p->n, zero, p->precision, planes)) return rc;
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    return ALP_OK;
}

int alp_points_set_observed(alp_points_t *p, const void *uv, int in_dtype) { return set_observed(p, uv, nullptr, in_dtype); }

int alp_points_set_observed_columns(alp_points_t *p, const void *u, const void *v, int in_dtype) {
    const void *const cols[2] = {u, v};
    return set_observed(p, nullptr, cols, in_dtype);
}

int alp_points_set_weights(alp_points_t *p, const void *w, int in_dtype) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p, "points handle is NULL");
    if (p->pending_P > 0 || p->loop_pending)
        return fail(ALP_ESTATE, "alp_points_set_weights: an evaluation or a device loop on this point set has not been waited for");
    for (alp_lm_t *h : p->lm_loops)
        if (lm_loop_pending(h))
            return fail(ALP_ESTATE, "alp_points_set_weights: a least-squares device loop on this point set has not been waited for");
    if (!w) {
        if (p->w) ALP_HIP(hipStreamSynchronize(ctx().stream));
        p->w.reset();
        p->w_sum = 0;
        return ALP_OK;
    }
    ALP_REQUIRE(in_dtype == ALP_F32 || in_dtype == ALP_F64, "in_dtype must be ALP_F32 or ALP_F64");
    return p->precision == ALP_F64 ? set_weights_t<double>(p, w, in_dtype) : set_weights_t<float>(p, w, in_dtype);
}

int alp_points_weight_sum(const alp_points_t *p, double *W) {
    ALP_REQUIRE(p && W, "NULL argument");
    *W = p->count_slot();
    return ALP_OK;
}

int alp_points_set_weight_table(alp_points_t *p, const void *w, int R, int in_dtype) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p, "points handle is NULL");
    if (p->pending_P > 0 || p->loop_pending)
        return fail(ALP_ESTATE, "alp_points_set_weight_table: an evaluation or a device loop on this point set has not been waited for");
    for (alp_lm_t *h : p->lm_loops)
        if (lm_loop_pending(h))
            return fail(ALP_ESTATE, "alp_points_set_weight_table: a least-squares device loop on this point set has not been waited for");
    if (!w) {
        if (p->wt) ALP_HIP(hipStreamSynchronize(ctx().stream));
        p->wt.reset();
        p->wt_rows = 0;
        p->wt_sums = nullptr;
        return ALP_OK;
    }
    ALP_REQUIRE(in_dtype == ALP_F32 || in_dtype == ALP_F64, "in_dtype must be ALP_F32 or ALP_F64");
    ALP_REQUIRE(R >= 1 && R <= host::NORMAL_BATCH_MAX, "R must be 1..1024");
    if ((int64_t)R * p->n * (int64_t)p->esize() > ALP_WEIGHT_TABLE_MAX_BYTES)
        return fail(ALP_EINVAL, "alp_points_set_weight_table: %d rows of %lld weights exceed ALP_WEIGHT_TABLE_MAX_BYTES", R, (long long)p->n);
    if (p->precision == ALP_F64)
        return in_dtype == ALP_F64 ? set_weight_table_t<double, double>(p, w, R) : set_weight_table_t<float, double>(p, w, R);
    return in_dtype == ALP_F64 ? set_weight_table_t<double, float>(p, w, R) : set_weight_table_t<float, float>(p, w, R);
}

int alp_points_weight_table_sums(alp_points_t *p, double *out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p && out, "NULL argument");
    if (!p->wt) return fail(ALP_ESTATE, "alp_points_weight_table_sums: no weight table set");
    ALP_HIP(hipMemcpyAsync(out, p->wt_sums, (size_t)p->wt_rows * sizeof(double), hipMemcpyDeviceToHost, ctx().stream));
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    return ALP_OK;
}

int alp_project(alp_points_t *p, const double params[ALP_NPARAM]) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p && params, "NULL argument");
    if (!p->u) {
        void **uv_planes[2] = {&p->u, &p->v};
        if (int rc = alloc_planes(p->slab_uv, 2, p->n_pad, p->esize(), uv_planes)) return rc;
    }
    p->projected = true;
    if (p->n == 0) return ALP_OK;
    return p->precision == ALP_F64 ? launch_project<double>(p, params) : launch_project<float>(p, params);
}

int alp_projected_fetch(alp_points_t *p, void *u_out, void *v_out, int out_dtype) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p, "points handle is NULL");
    ALP_REQUIRE(out_dtype == ALP_F32 || out_dtype == ALP_F64, "out_dtype must be ALP_F32 or ALP_F64");
    if (!p->projected) return fail(ALP_ESTATE, "alp_projected_fetch: nothing projected yet");
    if (p->n == 0) return ALP_OK;
    ALP_REQUIRE(u_out && v_out, "output is NULL");
    const size_t es = p->esize();
    if ((out_dtype == ALP_F64) == (p->precision == ALP_F64)) {
        ALP_HIP(hipMemcpyAsync(u_out, p->u, (size_t)p->n * es, hipMemcpyDeviceToHost, ctx().stream));
        ALP_HIP(hipMemcpyAsync(v_out, p->v, (size_t)p->n * es, hipMemcpyDeviceToHost, ctx().stream));
        ALP_HIP(hipStreamSynchronize(ctx().stream));
        return ALP_OK;
    }
    return fetch_converted(p, u_out, v_out, out_dtype);
}

int alp_projected_fetch_strided(alp_points_t *p, int64_t first, int64_t stride, int64_t count,
                                double *u_out, double *v_out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p && u_out && v_out, "NULL argument");
    if (!p->projected) return fail(ALP_ESTATE, "alp_projected_fetch_strided: nothing projected yet");
    ALP_REQUIRE(count >= 0 && first >= 0 && stride >= 1, "bad range");
    if (count == 0) return ALP_OK;
    ALP_REQUIRE(first + (count - 1) * stride < p->n, "range exceeds the point count");
    double *tmp = nullptr;
    if (int rc = scratch_reserve((size_t)count * 2 * sizeof(double), (void **)&tmp)) return rc;
    const unsigned grid = (unsigned)((count + 255) / 256);
    if (p->precision == ALP_F64)
        hipLaunchKernelGGL(gather_strided_kernel<double>, dim3(grid), dim3(256), 0, ctx().stream,
                           (const double *)p->u, (const double *)p->v, first, stride, count, tmp);
    else
        hipLaunchKernelGGL(gather_strided_kernel<float>, dim3(grid), dim3(256), 0, ctx().stream,
                           (const float *)p->u, (const float *)p->v, first, stride, count, tmp);
    hipError_t e = hipMemcpyAsync(u_out, tmp, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx().stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(v_out, tmp + count, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx().stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx().stream);
    if (e != hipSuccess) return fail(ALP_EHIP, "strided fetch: %s", hipGetErrorString(e));
    return ALP_OK;
}

int alp_residuals(alp_points_t *p, const double params[ALP_NPARAM], double *out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p && params, "NULL argument");
    if (!p->uo) return fail(ALP_ESTATE, "alp_residuals: observed uv not set");
    if (p->n == 0) return ALP_OK;
    ALP_REQUIRE(out, "out is NULL");
    return p->precision == ALP_F64 ? residuals_impl<double>(p, params, 1, out) : residuals_impl<float>(p, params, 1, out);
}

int alp_residuals_batch(alp_points_t *p, const double *cand, int64_t B, double *out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p && cand, "NULL argument");
    ALP_REQUIRE(B >= 1 && B <= 4096, "B out of range");
    if (!p->uo) return fail(ALP_ESTATE, "alp_residuals_batch: observed uv not set");
    if (p->n == 0) return ALP_OK;
    ALP_REQUIRE(out, "out is NULL");
    return p->precision == ALP_F64 ? residuals_impl<double>(p, cand, B, out) : residuals_impl<float>(p, cand, B, out);
}

int alp_residuals_assigned(alp_points_t *p, const double *cand, int64_t B, const int32_t *assign, double *out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p && cand, "NULL argument");
    ALP_REQUIRE(B >= 1 && B <= 4096, "B out of range");
    if (!p->uo) return fail(ALP_ESTATE, "alp_residuals_assigned: observed uv not set");
    if (p->n == 0) return ALP_OK;
    ALP_REQUIRE(assign && out, "NULL argument");
    for (int64_t i = 0; i < p->n; ++i)          // before the launch: the kernel indexes the records with it
        if (assign[i] >= B) return fail(ALP_EINVAL, "alp_residuals_assigned: assign[%lld] = %d names no pose of the %lld", (long long)i, (int)assign[i], (long long)B);
    return p->precision == ALP_F64 ? residuals_assigned_impl<double>(p, cand, B, assign, out)
                                   : residuals_assigned_impl<float>(p, cand, B, assign, out);
}

int alp_jacobian(alp_points_t *p, const double params[ALP_NPARAM], const int32_t *target_idx, int D, int of_residuals,
                 double *out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p && params, "NULL argument");
    JacPlan plan;
    if (int rc = jacobian_plan(params, p->origin, target_idx, D, of_residuals, &plan)) return rc;
    if (p->n == 0) return ALP_OK;
    ALP_REQUIRE(out, "out is NULL");
    return p->precision == ALP_F64 ? jacobian_impl<double>(p, plan, out) : jacobian_impl<float>(p, plan, out);
}

// alp_normal_equations (one pose), alp_normal_equations_batch (both: rows = false) and alp_normal_equations_batch_rows under their
// own names
static int normal_equations_batch_entry(const char *name, alp_points_t *p, const double *params, int64_t B, bool rows, const int32_t *row_of_pose,
                                        const int32_t *target_idx, int D, int loss, double f_scale, double *out) {
    if (int rc = require_init()) return rc;
    const auto refuse = [&](bool ok, const char *msg) { return ok ? ALP_OK : fail(ALP_EINVAL, "%s: %s", name, msg); };
    if (int rc = refuse(p && params && out && (row_of_pose || !rows), "NULL argument")) return rc;
    if (int rc = refuse(B >= 1 && B <= host::NORMAL_BATCH_MAX, "B must be 1..1024")) return rc;
    if (int rc = refuse(loss >= ALP_NORMAL_LINEAR && loss <= ALP_NORMAL_CAUCHY, "unknown loss")) return rc;
    if (int rc = refuse(f_scale > 0 && std::isfinite(f_scale), "f_scale must be a positive finite number")) return rc;
    std::vector<JacPlan> plans((size_t)B);
    for (int64_t b = 0; b < B; ++b)
        if (int rc = jacobian_plan(params + b * ALP_NPARAM, p->origin, target_idx, D, 1, &plans[(size_t)b])) return rc;
    if (!p->uo) return fail(ALP_ESTATE, "%s: observed uv not set", name);
    if (rows) {
        if (!p->wt) return fail(ALP_ESTATE, "%s: no weight table set", name);
        for (int64_t b = 0; b < B; ++b)             // before the launch: the kernel indexes the table with it
            if (row_of_pose[b] < 0 || row_of_pose[b] >= p->wt_rows)
                return fail(ALP_EINVAL, "%s: row_of_pose[%lld] = %d is no row of the table of %d", name, (long long)b, (int)row_of_pose[b], p->wt_rows);
    }
    return p->precision == ALP_F64 ? normal_batch_impl<double>(p, plans, loss, f_scale, out, row_of_pose)
                                   : normal_batch_impl<float>(p, plans, loss, f_scale, out, row_of_pose);
}

int alp_normal_equations(alp_points_t *p, const double params[ALP_NPARAM], const int32_t *target_idx, int D, int loss, double f_scale,
                         double *out) {
    return normal_equations_batch_entry(__func__, p, params, 1, false, nullptr, target_idx, D, loss, f_scale, out);
}

int alp_normal_equations_batch(alp_points_t *p, const double *params, int64_t B, const int32_t *target_idx, int D, int loss,
                               double f_scale, double *out) {
    return normal_equations_batch_entry(__func__, p, params, B, false, nullptr, target_idx, D, loss, f_scale, out);
}

int alp_normal_equations_batch_rows(alp_points_t *p, const double *params, int64_t B, const int32_t *row_of_pose, const int32_t *target_idx,
                                    int D, int loss, double f_scale, double *out) {
    return normal_equations_batch_entry(__func__, p, params, B, true, row_of_pose, target_idx, D, loss, f_scale, out);
}

// obs_b / prj_b NULL: that array is interleaved (n x 2 row-major); else a = the u column, b = the v column
static int loss_uv_any(const double *obs_a, const double *obs_b, const double *prj_a, const double *prj_b, int64_t n, int loss_kind,
                       double f_scale, double *loss_out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(loss_out, "loss_out is NULL");
    ALP_REQUIRE(n >= 0, "n is negative");
    ALP_REQUIRE(loss_kind == ALP_LOSS_MEAN_DIST || loss_kind == ALP_LOSS_HUBER, "unknown loss_kind");
    if (n == 0) {                      // np.mean of an empty array
        *loss_out = NAN;
        return ALP_OK;
    }
    ALP_REQUIRE(obs_a && prj_a, "NULL input");
    const int grid = stream_grid(n);
    char *dev = nullptr;
    const size_t col = (size_t)n * sizeof(double);
    if (int rc = scratch_reserve(4 * col + (size_t)(grid + 2) * sizeof(double), (void **)&dev)) return rc;
    double *d_obs = (double *)dev, *d_prj = (double *)(dev + 2 * col);
    double *partials = (double *)(dev + 4 * col);
    hipStream_t st = ctx().stream;
    hipError_t e = hipMemcpyAsync(d_obs, obs_a, obs_b ? col : 2 * col, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && obs_b) e = hipMemcpyAsync(d_obs + n, obs_b, col, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_prj, prj_a, prj_b ? col : 2 * col, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && prj_b) e = hipMemcpyAsync(d_prj + n, prj_b, col, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        using Kernel = void (*)(const double *, const double *, const double *, const double *, int64_t, double, double *);
        static const Kernel kernels[2][2][2] = {
            {{loss_uv_kernel<ALP_LOSS_MEAN_DIST, false, false>, loss_uv_kernel<ALP_LOSS_MEAN_DIST, false, true>},
             {loss_uv_kernel<ALP_LOSS_MEAN_DIST, true, false>, loss_uv_kernel<ALP_LOSS_MEAN_DIST, true, true>}},
            {{loss_uv_kernel<ALP_LOSS_HUBER, false, false>, loss_uv_kernel<ALP_LOSS_HUBER, false, true>},
             {loss_uv_kernel<ALP_LOSS_HUBER, true, false>, loss_uv_kernel<ALP_LOSS_HUBER, true, true>}}};
        hipLaunchKernelGGL(kernels[loss_kind == ALP_LOSS_HUBER][obs_b != nullptr][prj_b != nullptr], dim3(grid), dim3(256), 0, st,
                           d_obs, d_obs + n, d_prj, d_prj + n, n, f_scale, partials);
        hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, st, partials, grid, 1, (double)n, partials + grid);
        e = hipGetLastError();
    }
    double res[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(res, partials + grid, 2 * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ALP_EHIP, "alp_loss_uv: %s", hipGetErrorString(e));
    *loss_out = res[0] / (double)n;
    return ALP_OK;
}

int alp_loss_uv(const double *observed, const double *projected, int64_t n, int loss_kind, double f_scale,
                double *loss_out) {
    return loss_uv_any(observed, nullptr, projected, nullptr, n, loss_kind, f_scale, loss_out);
}

int alp_loss_uv_columns(const double *obs_u, const double *obs_v, const double *prj_u, const double *prj_v, int64_t n,
                        int loss_kind, double f_scale, double *loss_out) {
    return loss_uv_any(obs_u, obs_v, prj_u, prj_v, n, loss_kind, f_scale, loss_out);
}

int alp_eval_population_enqueue(alp_points_t *p, const double *cand, int64_t P, int loss_kind,
                                double f_scale) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p && cand, "NULL argument");
    ALP_REQUIRE(P >= 1 && P <= (1 << 20), "P out of range");
    ALP_REQUIRE(loss_kind == ALP_LOSS_MEAN_DIST || loss_kind == ALP_LOSS_HUBER, "unknown loss_kind");
    if (!p->uo) return fail(ALP_ESTATE, "alp_eval_population: observed uv not set");
    if (p->precision == ALP_F64) return enqueue_popeval<double>(p, cand, P, loss_kind, f_scale);
    return enqueue_popeval<float>(p, cand, P, loss_kind, f_scale);
}

int alp_eval_population_wait(alp_points_t *p, double *loss_out, int64_t *argmin_out) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p, "points handle is NULL");
    if (p->pending_P <= 0) return fail(ALP_ESTATE, "alp_eval_population_wait: nothing enqueued");
    const int64_t P = p->pending_P;
    p->pending_P = 0;                  // before the sync: a failed wait must not lock the handle (every later enqueue refused)
    ALP_HIP(hipStreamSynchronize(ctx().stream));
    const double n_total = p->sums_host[P];
    std::vector<double> local;
    double *loss = loss_out;
    if (!loss) {
        local.resize((size_t)P);
        loss = local.data();
    }
    // (the selection below is host/alp_host.h: NaN never wins, first index on ties, the CONFIRM_MAX smallest of a band)
    double best_v = 0;
    int64_t best = host::losses_and_argmin(p->sums_host, P, n_total, loss, &best_v);
    // (a caller that passes no argmin_out wants the losses only: no confirmation -- CMAOptimizer needs the argmin of its LAST
    // generation alone, optimize.py:427, and the confirmation costs a float64 pass over every point)
    if (argmin_out && best >= 0 && p->precision == ALP_F32 && P > 1 && best_v < INFINITY) {
        // candidates whose float32 loss lies within CONFIRM_GAP of the smallest one: if there is
        // more than one, float32 cannot order them -- evaluate (up to CONFIRM_MAX of) them again in
        // float64 arithmetic and take the argmin of those; identical on every rank (the sums are
        // all-reduced, so every rank sees the same band and joins the same second all-reduce)
        int64_t which[CONFIRM_MAX];
        int K = 0;
        if (host::confirm_band(loss, P, best_v, which, &K) > 1) {
            double sums[CONFIRM_MAX + 1];
            if (int rc = confirm_losses(p, p->cand_copy.data(), which, K, p->pending_loss, p->pending_f_scale, sums)) return rc;
            best = host::merge_confirmed(loss, which, K, sums);
        }
    }
    if (argmin_out) *argmin_out = best < 0 ? 0 : best;
    return ALP_OK;
}

int alp_eval_population_timing(alp_points_t *p, float *kernel_ms, float *allreduce_ms) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p, "points handle is NULL");
    if (!p->timed) return fail(ALP_ESTATE, "alp_eval_population_timing: no population evaluation yet");
    if (p->pending_P > 0) return fail(ALP_ESTATE, "alp_eval_population_timing: wait for the pending evaluation first");
    float a = 0, b = 0;
    ALP_HIP(hipEventElapsedTime(&a, p->ev[0], p->ev[1]));
    ALP_HIP(hipEventElapsedTime(&b, p->ev[1], p->ev[2]));
    if (p->mend_ran) {                 // the mend pass runs behind the all-reduce: its kernels (and its own all-reduce) count as kernel time
        float m = 0;
        ALP_HIP(hipEventElapsedTime(&m, p->ev[2], p->ev[3]));
        a += m;
    }
    if (kernel_ms) *kernel_ms = a;
    if (allreduce_ms) *allreduce_ms = b;
    return ALP_OK;
}

int alp_eval_population_info(alp_points_t *p, int64_t info[3]) {
    ALP_REQUIRE(p && info, "NULL argument");
    if (!p->timed) return fail(ALP_ESTATE, "alp_eval_population_info: no population evaluation yet");
    for (int k = 0; k < 3; ++k) info[k] = p->last_info[k];
    return ALP_OK;
}

int alp_points_set_mend(alp_points_t *p, int enable) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p, "points handle is NULL");
    if (p->pending_P > 0 || p->loop_pending)
        return fail(ALP_ESTATE, "alp_points_set_mend: an evaluation or a device loop on this point set has not been waited for");
    const bool on = enable != 0;
    // (a float64 set takes the setting and never runs the pass: its second walk gives the reference's values already)
    if (on && !p->mend && p->mend_cnt) ALP_HIP(hipMemsetAsync(p->mend_cnt, 0, sizeof(MendCount), ctx().stream));
    p->mend = on;
    return ALP_OK;
}

int alp_eval_population_mended(alp_points_t *p, int64_t info[4]) {
    if (int rc = require_init()) return rc;
    ALP_REQUIRE(p && info, "NULL argument");
    if (!p->timed) return fail(ALP_ESTATE, "alp_eval_population_mended: no population evaluation yet");
    if (p->pending_P > 0 || p->loop_pending)
        return fail(ALP_ESTATE, "alp_eval_population_mended: wait for the pending evaluation or device loop first");
    MendCount c = {0, 0};
    if (p->mend_cnt) {
        ALP_HIP(hipMemcpyAsync(&c, p->mend_cnt, sizeof(c), hipMemcpyDeviceToHost, ctx().stream));
        ALP_HIP(hipStreamSynchronize(ctx().stream));
    }
    info[0] = p->mend_ran ? c.last : 0;
    info[1] = c.total;
    info[2] = p->mend_ran ? p->mend_info[0] : 0;
    info[3] = p->mend_ran ? p->mend_info[1] : 0;
    return ALP_OK;
}

int alp_eval_population(alp_points_t *p, const double *cand, int64_t P, int loss_kind, double f_scale,
                        double *loss_out, int64_t *argmin_out) {
    if (int rc = alp_eval_population_enqueue(p, cand, P, loss_kind, f_scale)) return rc;
    return alp_eval_population_wait(p, loss_out, argmin_out);
}

}  // extern "C"
